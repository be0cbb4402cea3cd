"""GPU: one-mesh scenes under the baked top level (BakedForm::kTop, scene_traverse_baked_top) with the mesh
at every place in pine's order (tests/baked_top_scenes.py).  Every film must be the oracle's bit for bit, the precompiled
kernel's, and the feature-set kernel's; a second build of the scene's kernel with the case ledger (-DPINE_TOP_CASES) renders
the same bits and says which branches of the protocol its rays took -- the condition under which a scene counts as a test of
the branch it was built for.  The ledger comes from the code under test: it is never compared with an expected film, only
with the plan's own counts of the same rays and with the floor of 32 rays per named case."""
import ctypes as C
import functools

import numpy as np
import pytest

import baked_top_scenes as B
from conftest import assert_bit_equal, load_film

FLOOR = 32  # rays per named case: a scene that reaches its case with fewer is moved, never the floor
F_XSTAGE = 0x8000
CASES = [(name, cam) for name in B.SCENES for cam in B.CAMERAS]


def _render(scene, spp, depth, ledger=False, passes=None, **kw):
    """-> (film, stats, ledger counts or None).  `ledger`: the scene's kernel is built with -DPINE_TOP_CASES."""
    import torch
    import pine_amd as pa
    from pine_amd import _lib
    w, h = scene.camera.film().size
    # The flag is read when the kernel is requested, and specialize=True makes plan creation wait for the compiler: the variable
    # needs to be set around the constructor only.  (Were the compile ever deferred, the ledger would read all zeros and the
    # sum checks below would fail, not pass.)  A context, not the fixture: the cached renders below outlive a single test.
    with pytest.MonkeyPatch.context() as mp:
        if ledger:
            mp.setenv("PINE_GPU_SPECIALIZE_EXTRA", "-DPINE_TOP_CASES")
        plan = pa.Plan(scene, spp, depth, **({"pass_samples": passes} if passes else {}), **kw)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if passes:
        assert plan.pass_count > 1
        for j in range(plan.pass_count):
            plan.launch_pass(j, film.data_ptr(), stream)
    else:
        plan.launch(film.data_ptr(), stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    counts = None
    if ledger:
        raw = (C.c_uint64 * 16)()
        _lib.check(_lib.lib.pine_gpu_plan_debug_sections(plan._h, raw), "debug sections")
        counts = dict(zip(B.SLOTS, (int(v) for v in raw)))
    out = film.cpu().numpy()
    plan.close()
    return out, st, counts


@functools.lru_cache(maxsize=None)
def _want(name, cam):
    from oracle import oracle
    oracle.build()
    case = B.SCENES[name]
    ref, _ = oracle.render(B.build(name, cam).describe(), case.size, case.spp, case.depth)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _ledger(name, cam):
    """The ledger build's film, stats and counts for one (scene, camera): rendered once, shared by the tests below."""
    case = B.SCENES[name]
    film, st, counts = _render(B.build(name, cam), case.spp, case.depth, ledger=True, specialize=True)
    film.setflags(write=False)
    return film, st, counts


@pytest.mark.gpu
@pytest.mark.parametrize("name, cam", CASES)
def test_film_is_the_oracles_under_every_kernel(name, cam):
    from pine_amd import _lib
    case, want = B.SCENES[name], _want(name, cam)
    scene = B.build(name, cam)
    film, st, _ = _render(scene, case.spp, case.depth, specialize=True)
    assert st.specialized == 2 and (st.kernel_features & F_XSTAGE), (st.specialized, hex(st.kernel_features))
    assert_bit_equal(film, want, f"{name}/{cam}: top level baked vs the oracle")
    film, st, _ = _render(scene, case.spp, case.depth, specialize=False)
    assert st.specialized == 0
    assert_bit_equal(film, want, f"{name}/{cam}: the precompiled kernel vs the oracle")
    film, st, _ = _render(scene, case.spp, case.depth, flags=_lib.FLAG_SPECIALIZE | _lib.FLAG_SPECIALIZE_NO_BAKE)
    assert st.specialized in (0, 1)  # (0: the scene's feature set is a precompiled variant's already)
    assert_bit_equal(film, want, f"{name}/{cam}: FLAG_SPECIALIZE_NO_BAKE vs the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("name, cam", CASES)
def test_ledger_build_renders_the_same_bits_and_reaches_its_cases(name, cam):
    case = B.SCENES[name]
    film, st, n = _ledger(name, cam)
    print(f"ledger {name}/{cam} place {case.place} spp {case.spp} depth {case.depth} size {case.size[0]}: " + " ".join(f"{k}={v}" for k, v in n.items()))
    assert st.specialized == 2 and (st.kernel_features & F_XSTAGE)
    assert_bit_equal(film, _want(name, cam), f"{name}/{cam}: the ledger build vs the oracle")
    # the sums the plan counts itself: every radiance() invocation traces one closest-hit ray; every shadow ray ends in one of
    # the four shadow slots; every vertex that parked its shadow ray is one of the rays stage XS retired
    w, h = case.size
    closest = sum(n[k] for k in B.CLOSEST)
    assert st.camera_samples == w * h * case.spp
    assert closest == st.vertices, (closest, st.vertices)
    if case.depth == 1:
        assert closest == w * h * case.spp and sum(n[k] for k in B.SHADOW + B.PARKED) == 0
    assert sum(n[k] for k in B.SHADOW) == st.shadow_rays, (n, st.shadow_rays)
    assert sum(n[k] for k in B.PARKED) == n["shadow_xs_occluded"] + n["shadow_xs_clear"]
    assert n["tri_tie"] <= n["tri_in_front"]
    assert n["reached_with_hit"] <= closest - n["settled"]
    # (text order is visiting order unless a two-pass node above the mesh swaps its children)
    if case.place.startswith("M") and not case.two_pass:
        assert n["reached_with_hit"] == 0  # (nothing is tested before the mesh)
    if case.place.endswith("M") and not case.two_pass:
        assert n["tri_in_front"] == n["replay_camera"] == n["replay_spawned"] == 0  # (nothing is stored after it: r_pb == 0)
    if "kBakedTopPlainRects = false" in B.source(B.build(name, cam)):
        assert n["tri_none_after"] == n["tri_in_front"] == 0  # (a primitive whose t depends on its bound: every triangle is replayed)
    # the cases this scene exists for
    short = {k: n[k] for k in case.reach if n[k] < FLOOR}
    assert not short, f"{name}/{cam}: fewer than {FLOOR} rays took {short}"


@pytest.mark.gpu
def test_every_slot_is_reached_somewhere():
    total = dict.fromkeys(B.SLOTS, 0)
    replays = {"replay_camera": set(), "replay_spawned": set()}
    for name, cam in CASES:
        n = _ledger(name, cam)[2]
        for k, v in n.items():
            total[k] += v
        for k in replays:
            if n[k] >= FLOOR:
                replays[k].add(name)
    print("ledger total: " + " ".join(f"{k}={v}" for k, v in total.items()))
    print("ledger ties:", {f"{name}/{cam}": _ledger(name, cam)[2]["tri_tie"] for name, cam in CASES if _ledger(name, cam)[2]["tri_tie"]})
    assert not [k for k, v in total.items() if v == 0 and k != "tri_tie"], total
    assert all(len(v) >= 2 for v in replays.values()), replays


@pytest.mark.gpu
def test_shards_and_passes_of_a_scene_with_the_mesh_in_the_middle():
    name, cam = "inner_b_glossy", "off"
    case, want = B.SCENES[name], _want(name, cam)
    assert "M" in case.place[1:-1]
    scene = B.build(name, cam)
    total = np.zeros_like(want)
    for rank in range(2):
        part, st, _ = _render(scene, case.spp, case.depth, specialize=True, shard_rank=rank, shard_world=2)
        assert st.specialized == 2
        total += part
    assert_bit_equal(total, want, "two shards sum to the whole film")
    film, st, _ = _render(scene, case.spp, case.depth, specialize=True, passes=case.spp // 2)
    assert st.specialized == 2
    assert_bit_equal(film, want, "two passes leave the whole film")


@pytest.mark.gpu
@pytest.mark.parametrize("golden", list(B.GOLDEN_FILMS))
def test_film_is_the_real_references(golden):
    """Not only the restatement: the film the REAL reference rendered of the scene (tools/make_golden.py --baked-top)."""
    ref, ps, spp, depth = load_film(golden)
    name = B.GOLDEN_FILMS[golden]
    scene = B.build(name, "axis", (24, 24))
    assert scene.describe() == ps and (spp, depth) == (B.SCENES[name].spp, B.SCENES[name].depth)
    film, st, _ = _render(scene, spp, depth, specialize=True)
    assert st.specialized == 2
    assert_bit_equal(film, ref, f"{golden}: top level baked vs the reference's film")
