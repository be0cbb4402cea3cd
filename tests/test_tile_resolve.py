"""GPU (-m gpu): owned tiles of the stage-queued path kernel.  A workgroup claims whole 8x8 tiles and the
wave that retires a tile's last work item sums it inside the path kernel; resolve_kernel sums what is left.  Both run one
device function, so the film must not change by a bit whichever of them sums a tile: PINE_GPU_OWNED_TILES=0 (every tile
left to resolve_kernel), the automatic split, and every tile owned are compared bit for bit, with each other and -- where a
fixture exists -- with the reference's film; the radiance() invocation counts must agree too."""
import pytest

from conftest import assert_bit_equal, load_film
from film_scenes import film_scene

pytestmark = pytest.mark.gpu

MODES = {"off": "0", "auto": None, "all": "1000000"}  # (a count above the shard's tiles: all of them)
KNOBS = ("PINE_GPU_OWNED_TILES", "PINE_GPU_TEST_TILE_SLOTS", "PINE_GPU_KERNEL", "PINE_GPU_TEST_VARIANT", "PINE_GPU_POOL_ITEMS", "PINE_GPU_SPECIALIZE")


def _set_mode(mp, mode, slots=None):
    for k in KNOBS:
        mp.delenv(k, raising=False)
    if MODES[mode] is not None:
        mp.setenv("PINE_GPU_OWNED_TILES", MODES[mode])
    if slots is not None:
        mp.setenv("PINE_GPU_TEST_TILE_SLOTS", str(slots))


def _render(scene, spp, depth, packed=False, **kw):
    """-> film (or this rank's slab), plan statistics."""
    import torch
    import pine_amd as pa
    w, h = scene.camera.film().size
    kw.setdefault("specialize", False)
    plan = pa.Plan(scene, spp, depth, **kw)
    stream = torch.cuda.current_stream().cuda_stream
    if packed:
        out = torch.full((plan.slab_floats(),), -7.0, dtype=torch.float32, device="cuda")
        plan.launch_packed(out.data_ptr(), stream)
    else:
        out = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
        plan.launch(out.data_ptr(), stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    assert st.block_threads == 1024, "the stage-queued kernel renders these scenes"
    assert (st.specialized >= 1) if kw["specialize"] else (st.specialized == 0)
    res = out.cpu().numpy()
    plan.close()
    return res, st


def _tiles(size, world=1, rank=0):
    total = ((size[0] + 7) // 8) * ((size[1] + 7) // 8)
    return len(range(rank, total, world))


def _three_modes(mp, scene, spp, depth, tiles, golden=None, slots=None, **kw):
    """Renders in the three modes; returns {mode: stats}."""
    films, stats = {}, {}
    for mode in MODES:
        _set_mode(mp, mode, slots)
        films[mode], stats[mode] = _render(scene, spp, depth, **kw)
        print(f"{mode}: tiles_in_kernel={stats[mode].tiles_in_kernel} of {tiles} vertices={stats[mode].vertices} grid={stats[mode].grid_blocks}")
    for mode in ("auto", "all"):
        assert_bit_equal(films[mode], films["off"], f"owned tiles {mode} vs off")
        assert stats[mode].vertices == stats["off"].vertices, f"vertices, {mode} vs off"
    if golden is not None:
        assert_bit_equal(films["off"], golden, "against the reference's film")
    assert stats["off"].tiles_in_kernel == 0
    assert 0 <= stats["auto"].tiles_in_kernel <= tiles
    if slots is None:
        # a workgroup's first claim always finds a slot; with more tiles than slots, how many find none depends on timing
        assert (stats["all"].tiles_in_kernel == tiles) if tiles <= 4 else (0 < stats["all"].tiles_in_kernel <= tiles)
    return stats


@pytest.mark.parametrize("name", ["cbox_readme_64_s16_d4", "mats_zoo_64_s32_d6"])
def test_golden_films_in_every_mode(monkeypatch, name):
    """cbox 64x64 at 16 spp: about 22 workgroups with about 3 tiles each, a workgroup has two tiles in flight."""
    ref, _, spp, depth = load_film(name)
    st = _three_modes(monkeypatch, film_scene(name), spp, depth, 64, golden=ref)
    assert st["off"].serial_tiles == 0  # (a plain variant: no tile classes -- and "all" above summed every tile in the kernel)


@pytest.mark.parametrize("size, spp, depth", [((8, 8), 16, 4),      # a single tile
                                              ((24, 16), 16, 4),    # fewer tiles than workgroups could take
                                              ((20, 12), 16, 5),    # border tiles: pixels outside the film are counted off at hand-out
                                              ((45, 37), 8, 3),
                                              ((32, 24), 1, 4),     # one chunk per pixel: a tile is 64 items
                                              ((32, 24), 2, 4),
                                              ((16, 16), 256, 6)])  # many chunks, few tiles
def test_shapes(monkeypatch, size, spp, depth):
    from pine_amd import scenes
    _three_modes(monkeypatch, scenes.cbox(size, "readme"), spp, depth, _tiles(size))


def test_automatic_split(monkeypatch):
    """A film with more tiles than twice the workgroups, each tile more items than a workgroup has contexts: the automatic mode
    owns the tiles beyond two per workgroup (here 575 - 2 * grid), the fine claims behind them go to resolve_kernel."""
    from pine_amd import scenes
    size = (200, 184)
    st = _three_modes(monkeypatch, scenes.cbox(size, "readme"), 64, 3, _tiles(size))
    owned = _tiles(size) - 2 * st["auto"].grid_blocks
    assert owned > 0 and 0 < st["auto"].tiles_in_kernel <= owned


@pytest.mark.parametrize("packed", [False, True])
def test_two_shards(monkeypatch, packed):
    """shard_world = 2, both ranks: the film (zeros outside the shard) and the packed slab."""
    from pine_amd import scenes
    size = (44, 28)
    for rank in (0, 1):
        _three_modes(monkeypatch, scenes.cbox(size, "readme"), 16, 4, _tiles(size, 2, rank), packed=packed, shard_rank=rank, shard_world=2)


@pytest.mark.parametrize("slots", [1, 0])
def test_no_free_slot_falls_back_to_the_resolve_kernel(monkeypatch, slots):
    """The table of a workgroup's tiles in flight forced to one slot (and to none): a claim that finds none is rendered as
    before and summed by resolve_kernel -- the same film."""
    ref, _, spp, depth = load_film("cbox_readme_64_s16_d4")
    st = _three_modes(monkeypatch, film_scene("cbox_readme_64_s16_d4"), spp, depth, 64, golden=ref, slots=slots)
    if slots == 0:
        assert st["all"].tiles_in_kernel == 0
    else:
        assert 0 < st["all"].tiles_in_kernel <= 64


def test_scene_kernel(monkeypatch):
    """The scene's own kernel (compiled for this scene from the same body) in the three modes, against the fixture."""
    ref, _, spp, depth = load_film("cbox_readme_64_s16_d4")
    _three_modes(monkeypatch, film_scene("cbox_readme_64_s16_d4"), spp, depth, 64, golden=ref, specialize=True)
