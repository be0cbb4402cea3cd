"""Noise nodes on the device: material_params and whole films against fixtures made by the real reference
(tools/make_golden_noise.py), bit for bit -- both path kernels, the scene's own kernel (baked and not), sample passes, every
precompiled variant that runs node programs, the PRL example, the guide images."""
import os

import numpy as np
import pytest

import noise_scenes as X
from test_kernel_variants import F, VARIANTS
from test_noise import GOLDEN, _lib, check_records, pa, zoo, zoo_fixture  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
ROOM = "noise_room_48x32_s8_d4"
SCRIPT_ROOM = "noise_script_room_48x32_s8_d4"
KNOBS = ("PINE_GPU_TEST_VARIANT", "PINE_GPU_TEST_LDS_NODES", "PINE_GPU_KERNEL", "PINE_GPU_NO_LDS_SCENE", "PINE_GPU_XSTAGE", "PINE_GPU_LDS_TRIS",
         "PINE_GPU_SPECIALIZE", "PINE_GPU_SPECIALIZE_FORCE", "PINE_GPU_SPECIALIZE_EXTRA")
REFUSED = "pinned kernel variant does not cover this scene"
# the precompiled variants that run node programs in pine's order: F_NODES, neither F_EMBREE nor F_VLOG
NODE_VARIANTS = [(kind, order) for kind, table in VARIANTS.items() for order, (features, _) in sorted(table.items())
                 if features & F["NODES"] and not features & (F["EMBREE"] | F["VLOG"])]


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def golden_film(name):
    return np.load(os.path.join(GOLDEN, f"noise_film_{name}.npz"))["film"]


def render(name, **kw):
    size, spp, depth = X.FILMS[name]
    passes = kw.pop("pass_samples", None)
    integ = pa.PathIntegrator(pa.BlueSampler(spp), depth, device=0, **kw)
    return integ.render(X.film_scene(name), pass_samples=passes).pixels


def assert_film(got, name, what):
    want = golden_film(name)
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2)
    assert not bad.any(), f"{name} ({what}): {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"


def test_device_records_equal_the_references(zoo, zoo_fixture):  # noqa: F811
    check_records(0, zoo, zoo_fixture)


def test_the_fixtures_are_the_scenes_the_tests_render():
    for name in X.FILMS:
        want = bytes(np.load(os.path.join(GOLDEN, f"noise_film_{name}.npz"))["pscene"]).decode()
        assert X.film_scene(name).describe() == want
        assert np.isfinite(golden_film(name)).all()


@pytest.mark.parametrize("kernel", ["queue", "mega"])
def test_room_film_equals_the_references(kernel, monkeypatch):
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    assert_film(render(ROOM, specialize=False), ROOM, kernel)


@pytest.mark.parametrize("bake", [True, False])
def test_room_with_the_scenes_own_kernel(bake, monkeypatch, tmp_path):
    import torch
    monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
    (w, h), spp, depth = X.FILMS[ROOM]
    # (plan creation waits for the compiler: the launch below runs the scene's own kernel)
    plan = pa.Plan(X.room((w, h)), pa.BlueSampler(spp), depth, specialize=True, flags=0 if bake else _lib.FLAG_SPECIALIZE_NO_BAKE)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    plan.close()
    assert st.specialized == (2 if bake else 1)  # (2: feature set + baked scene)
    assert_film(film.cpu().numpy(), ROOM, "baked" if bake else "not baked")


def test_room_in_four_passes():
    assert_film(render(ROOM, specialize=False, pass_samples=2), ROOM, "4 passes")


def test_node_variants_are_the_expected_ones():
    assert NODE_VARIANTS == [("queue", o) for o in (5, 6, 7, 8, 11, 12, 13, 14, 15)] + [("mega", 3), ("mega", 4)]


@pytest.mark.parametrize("kind,order", NODE_VARIANTS)
def test_room_under_every_variant_that_runs_node_programs(kind, order, monkeypatch):
    """PINE_GPU_TEST_VARIANT makes plan creation consider that variant alone.  A variant may refuse the room as not covered
    (by name; the fallbacks never do); one that takes it renders the reference's film."""
    import torch
    monkeypatch.setenv("PINE_GPU_TEST_VARIANT", f"{kind}:{order}")
    (w, h), spp, depth = X.FILMS[ROOM]
    try:
        plan = pa.Plan(X.room((w, h)), pa.BlueSampler(spp), depth, specialize=False)
    except pa.PineError as e:
        assert REFUSED in str(e) and (kind, order) not in (("queue", 15), ("mega", 4)), str(e)
        return
    try:
        film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
        plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        plan.check()
        st = plan.stats()
    finally:
        plan.close()
    assert (st.kernel_features, st.specialized) == (VARIANTS[kind][order][0], 0)
    assert_film(film.cpu().numpy(), ROOM, f"{kind}:{order}")


def test_room_fast_build_is_refused_like_every_node_scene():
    """PINE_GPU_FLAG_FAST covers the BASELINE scenes' feature sets, none of which has node programs (pine_kernels_fast.hip): the
    noise room is refused by name like any other scene with node-driven materials, never rendered by another kernel."""
    size, spp, depth = X.FILMS[ROOM]
    with pytest.raises(pa.PineError, match="PINE_GPU_FLAG_FAST: no declared-tolerance kernel variant covers this scene"):
        pa.PathIntegrator(pa.BlueSampler(spp), depth, device=0, specialize=False, flags=_lib.FLAG_FAST).render(X.room(size))


def test_script_room_film_equals_the_references():
    assert_film(render(SCRIPT_ROOM, specialize=False), SCRIPT_ROOM, "queue")


def test_prl_example_renders_the_script_rooms_film():
    """examples/noise.pine as it stands (it names BVH(): the fixtures are PathIntegrator(BVH(), ...)), but for the PNG it saves."""
    from pine_amd import prl
    root = os.path.dirname(os.path.dirname(GOLDEN))
    src = open(os.path.join(root, "examples", "noise.pine")).read()
    cut = src.replace('world.camera.film().save("noise.png");', "")
    assert cut != src and "PathIntegrator(BVH(), BlueSampler(8), UniformLightSampler(), 4)" in cut
    prl.interpret(cut)
    assert_film(np.ascontiguousarray(prl.last_film(), dtype=np.float32), SCRIPT_ROOM, "PRL script")


def test_room_guides_equal_the_references():
    fx = np.load(os.path.join(GOLDEN, "noise_guides_room.npz"))
    scene = X.room(X.GUIDES_SIZE)
    assert scene.describe() == bytes(fx["pscene"]).decode()
    albedo, normal = pa.guides(scene)
    for got, want, what in ((albedo, fx["albedo"], "albedo"), (normal, fx["normal"], "normal")):
        bad = (np.ascontiguousarray(got, np.float32).view(np.uint32) != want.view(np.uint32)).any(axis=2)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}"
