"""GPU (-m gpu): every device handle the library takes -- device blocks, pinned memory, events, streams -- has an owner that
gives it back (pine_amd/csrc/pine_device_buffer.h).  pine_gpu_test_live_device_blocks counts what the owners hold and what the
memory pool caches; every case here reads the count, does its work and finds the count where it was: plans of every kind that
holds a different set of resources, plan creation that fails after device memory was taken, every device test hook with good
and with rejected arguments, the builders, the one-shot renders."""
import ctypes as C
import gc
import os
from contextlib import contextmanager

import numpy as np
import pytest

import atmosphere_scenes as A
import envsky_scenes as E
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
F32 = np.float32
P_U32 = C.POINTER(C.c_uint32)


def live():
    """(handles the library's owners hold, blocks the pool caches)"""
    from pine_amd import _lib
    out = (C.c_int64 * 2)()
    _lib.check(_lib.lib.pine_gpu_test_live_device_blocks(out), "pine_gpu_test_live_device_blocks")
    return int(out[0]), int(out[1])


@contextmanager
def nothing_left_behind():
    gc.collect()  # (a plan an earlier test dropped without closing goes now, not in the middle of the count)
    before = live()[0]
    yield before
    gc.collect()
    assert live()[0] == before, "handles were left behind"


def fp(a):
    from pine_amd import _lib
    return a.ctypes.data_as(_lib.c_f_p)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for name in ("PINE_GPU_TEST_VARIANT", "PINE_GPU_AO_VARIANT", "PINE_GPU_KERNEL", "PINE_GPU_SPECIALIZE", "PINE_GPU_POOL_MB"):
        monkeypatch.delenv(name, raising=False)


# ---- 1. plans ---------------------------------------------------------------------------------------------------------------
def _plan_cases():
    import pine_amd as pa
    from pine_amd import _lib, scenes
    cbox = lambda: scenes.cbox((32, 32))  # noqa: E731
    return {
        "timing_progress": (cbox, dict(spp=8, max_path_length=3, timing=True, flags=_lib.FLAG_PROGRESS)),      # events, the pinned word
        "passes": (cbox, dict(spp=16, max_path_length=3, pass_samples=4)),                                     # running sum, carried RNG states
        "vertex_log": (cbox, dict(spp=8, max_path_length=3, flags=_lib.FLAG_VERTEX_LOG)),
        "sss_mesh": (lambda: scenes.sss((24, 24), 1), dict(spp=8, max_path_length=4)),                          # tokens, tile order, triangles
        "halton": (cbox, dict(spp=pa.HaltonSampler(8), max_path_length=3)),                                    # Halton tables
        "image_sky": (lambda: E.film_scene("const_24_s8_d3"), dict(spp=8, max_path_length=3)),                 # env buffer
        "ao": (cbox, dict(spp=pa.BlueSampler(16), max_path_length=1, integrator="ao")),
    }


PLAN_CASES = ["timing_progress", "passes", "vertex_log", "sss_mesh", "halton", "image_sky", "ao"]


@pytest.mark.parametrize("case", PLAN_CASES)
def test_a_plan_gives_back_what_it_took(case):
    import torch
    import pine_amd as pa
    from pine_amd import _lib
    make_scene, kw = _plan_cases()[case]
    sc = make_scene()
    w, h = sc.camera.film().size
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    with nothing_left_behind() as before:
        if case != "ao":
            kw["specialize"] = False  # (no compiler child: the precompiled kernel)
        plan = pa.Plan(sc, **kw)
        assert live()[0] > before, "the plan's buffers are not counted"
        if case == "vertex_log":
            n = _lib.check(_lib.lib.pine_gpu_plan_vertex_log(plan._h, None, 0), "vertex log")
        if case == "passes":
            assert plan.pass_count > 1
        plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
        plan.check()
        if case == "vertex_log":
            log = np.zeros(n, F32)
            assert _lib.lib.pine_gpu_plan_vertex_log(plan._h, fp(log), n) == n, _lib.last_error()
        if case == "timing_progress":
            assert plan.stats().timed_launches == 1
        plan.close()
    assert np.isfinite(film.cpu().numpy()).all()


def test_sharded_plans_give_back_what_they_took():
    import torch
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((32, 32))
    with nothing_left_behind():
        for rank in (0, 1):
            plan = pa.Plan(sc, 8, 3, shard_rank=rank, shard_world=2, specialize=False)
            slab = torch.zeros(plan.slab_floats(), dtype=torch.float32, device="cuda")
            plan.launch_packed(slab.data_ptr(), torch.cuda.current_stream().cuda_stream)
            plan.check()
            plan.close()


# ---- 2. creation that fails after device memory was taken ----------------------------------------------------------------------
def test_failed_plan_creation_gives_everything_back(monkeypatch):
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((32, 32))
    with nothing_left_behind():
        monkeypatch.setenv("PINE_GPU_TEST_VARIANT", "queue:9999")
        with pytest.raises(pa.PineError, match="PINE_GPU_TEST_VARIANT=queue:9999: no such kernel variant"):
            pa.Plan(sc, 8, 3)
        monkeypatch.delenv("PINE_GPU_TEST_VARIANT")
        monkeypatch.setenv("PINE_GPU_AO_VARIANT", "9999")
        with pytest.raises(pa.PineError, match="PINE_GPU_AO_VARIANT names no AO kernel variant that covers this scene"):
            pa.Plan(sc, pa.BlueSampler(16), 1, integrator="ao")


# ---- 3. the device test hooks ----------------------------------------------------------------------------------------------------
def _one_material_scene():
    import pine_amd as pa
    s = pa.Scene()
    s.add("d", pa.Diffuse([0.8, 0.7, 0.6]))
    s.add(pa.Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], True), "d")
    s.add(pa.Rect([0, 2, 1], [1, 0, 0], [0, 0, 1], False), pa.Emissive([4, 4, 4]))
    s.set(pa.ThinLenCamera(pa.Film([16, 16], pa.Uncharted2()), [0, 1, -4], [0, 1, 0], 0.5))
    return s


RAYS = np.ascontiguousarray([[0, 1, -4, 0, 0, 1, 0, 1e30], [0, 1, -4, 0.1, -0.2, 1, 0, 1e30], [0, 1, -4, 0, 1, 0, 0, 1e30]], F32)


def test_hooks_give_back_what_they_took():
    import pine_amd as pa
    from pine_amd import _lib, scenes
    from test_frame_table import frame_table
    from test_node_fixtures import choose_lobe
    from test_sampling_fixtures import product_bxdf
    lib, ok = _lib.lib, _lib.check
    x = np.float32([0.0, 0.5, 1.0, 2.5, 100.0])
    a, b = np.zeros_like(x), np.zeros_like(x)
    cbox, one = scenes.cbox((32, 32)), _one_material_scene()
    sky = pa.Scene()
    sky.set(E.image_sky("sun"))
    bxdf_cases = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "bxdf_lobes.npz"))["cases"][:8])
    lobe_case = np.zeros((1, 16), F32)
    lobe_case[0, 4:7], lobe_case[0, 9:12] = (0, 1, 0), (0, 1, 0)  # material 0 (Diffuse), n and wi up, pixel (0, 0), sample 0
    big = np.zeros(1 << 16, F32)
    with nothing_left_behind():
        ok(lib.pine_gpu_test_sincos(0, fp(x), x.size, fp(a), fp(b)), "sincos")
        ok(lib.pine_gpu_test_powlog(0, fp(x), fp(x), x.size, fp(a), fp(b)), "powlog")
        ok(lib.pine_gpu_test_atan(0, fp(x), fp(x), x.size, fp(a), fp(b)), "atan")
        args, got = x.view(np.uint32), np.zeros(x.size, np.uint32)
        ok(lib.pine_gpu_test_math_eval(0, 13, args.ctypes.data_as(P_U32), None, None, args.size, got.ctypes.data_as(P_U32)), "math_eval")
        stats, ex = np.zeros(4, np.int64), np.zeros((8, 5), np.uint32)
        ok(lib.pine_gpu_test_math_sweep(0, 13, 0, 0, 0x3f000000, 64, 1, stats.ctypes.data_as(C.POINTER(C.c_int64)), ex.ctypes.data_as(P_U32), 8), "math_sweep")
        assert stats[0] == 64 and stats[1] == 0
        stream = np.zeros(6 * 530, F32)
        ok(lib.pine_gpu_test_sampler(0, 1, fp(stream), stream.size), "sampler")
        for kind, mode in ((2, 0), (1, 0), (0, 1)):  # HaltonSampler's table block; BlueSampler through the LDS form
            draw = np.int32([[kind, 16, 300, 200, 129, 130, 15, 1, 8]])
            ok(lib.pine_gpu_test_sampler_draws(0, kind, 16, 300, 200, mode, draw.ctypes.data_as(C.POINTER(C.c_int32)), 1, fp(big), big.size), "sampler_draws")
        words = np.zeros(6 * 19, np.uint64)
        ok(lib.pine_gpu_test_rng(0, words.ctypes.data_as(C.POINTER(C.c_uint64)), words.size), "rng")
        for flat in (0, 1):
            trav = np.zeros((len(RAYS), 2 * 64 + 5), np.uint32)
            ok(lib.pine_gpu_test_traverse(cbox._h, 0, fp(RAYS), len(RAYS), flat, 64, trav.ctypes.data_as(P_U32)), "traverse")
        ok(lib.pine_gpu_test_shapes(scenes.shapes_zoo((48, 48))._h, 0, fp(RAYS), len(RAYS), fp(big), big.size), "shapes")
        product_bxdf(0, bxdf_cases)
        queries = np.ascontiguousarray([[0, 1, 0, 0.25, 0.75, 0.5], [0.3, 0.2, 0.1, 0.5, 0.5, 0.1]], F32)
        ok(lib.pine_gpu_test_light_samples(cbox._h, 0, fp(queries), len(queries), fp(big)), "light_samples")
        env_q = np.ascontiguousarray([[0.25, 0.75, 0, 1, 0], [0.5, 0.5, 1, 0, 0]], F32)
        ok(lib.pine_gpu_test_env_light(sky._h, 0, fp(env_q), len(env_q), fp(big)), "env_light")
        ok(lib.pine_gpu_test_env_light_sample(sky._h, 0, fp(env_q), len(env_q), fp(big)), "env_light_sample")
        colour_q = np.ascontiguousarray([[0, 1, 0, 0.3, 1.0, 0.2, 1.0]], F32)
        ok(lib.pine_gpu_test_atmosphere_color(0, fp(colour_q), 1, fp(big)), "atmosphere_color")
        point = np.ascontiguousarray([[0, 0, 1, 0, 1, 0, 0.5, 0.5]], F32)
        ok(lib.pine_gpu_test_material_params(one._h, 0, fp(point), 1, fp(big)), "material_params")
        choose_lobe(one, lobe_case)
        plan = pa.Plan(cbox, 8, 3, specialize=False)
        frame_table(cbox, plan)
        plan.close()
        # the builders: the Atmosphere light's tables and the BVH, both on the device
        sun = pa.Scene()
        sun.set(A.light("tall", 0))
        ok(lib.pine_gpu_scene_build_accel_device(scenes.cbox((32, 32))._h, 0), "device BVH build")


def test_hooks_that_reject_their_arguments_give_back_what_they_took():
    import pine_amd as pa
    from pine_amd import _lib, scenes
    lib = _lib.lib
    cbox, one = scenes.cbox((32, 32)), _one_material_scene()
    x, big = np.zeros(4, F32), np.zeros(4096, F32)

    def rejected(rc, message):
        assert rc < 0 and message in _lib.last_error(), _lib.last_error()

    with nothing_left_behind():
        rejected(lib.pine_gpu_test_math_eval(0, 13, None, None, None, 4, x.view(np.uint32).ctypes.data_as(P_U32)), "bad argument")
        rejected(lib.pine_gpu_test_sampler(0, 1, fp(big), 10), "capacity too small")
        draw = np.int32([[2, 16, 300, 200, 129, 130, 15, 1, 8]])
        rejected(lib.pine_gpu_test_sampler_draws(0, 2, 16, 300, 200, 0, draw.ctypes.data_as(C.POINTER(C.c_int32)), 1, fp(big), 11), "capacity too small")
        draw[0, 4] = 300
        rejected(lib.pine_gpu_test_sampler_draws(0, 2, 16, 300, 200, 0, draw.ctypes.data_as(C.POINTER(C.c_int32)), 1, fp(big), big.size),
                 "pine_gpu_test_sampler_draws: a case's pixel lies outside the film")
        rejected(lib.pine_gpu_test_rng(0, np.zeros(4, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), 4), "capacity too small")
        rejected(lib.pine_gpu_test_traverse(cbox._h, 0, fp(RAYS), len(RAYS), 0, 1, big.view(np.uint32).ctypes.data_as(P_U32)), "bad argument")
        rejected(lib.pine_gpu_test_shapes(cbox._h, 0, fp(RAYS), len(RAYS), fp(big), 1), "capacity too small")
        bad_lobe = np.full((1, 16), 9.0, F32)
        rejected(lib.pine_gpu_test_bxdf(0, fp(bad_lobe), 1, fp(big)), "pine_gpu_test_bxdf: unknown lobe")
        rejected(lib.pine_gpu_test_light_samples(cbox._h, 0, fp(big), -1, fp(big)), "bad argument")
        rejected(lib.pine_gpu_test_env_light(cbox._h, 0, fp(big), 1, fp(big)), "pine_gpu_test_env_light: the scene's environment light is no ImageSky and no Atmosphere")
        rejected(lib.pine_gpu_test_env_light_sample(cbox._h, 0, fp(big), 1, fp(big)),
                 "pine_gpu_test_env_light_sample: the scene's environment light is no ImageSky and no Atmosphere")
        rejected(lib.pine_gpu_test_atmosphere_color(0, fp(big), -1, fp(big)), "bad argument")
        rejected(lib.pine_gpu_test_material_params(one._h, 0, fp(big), -1, fp(big)), "bad argument")
        emissive = np.zeros((1, 16), F32)
        emissive[0, 0] = 1.0  # (the lamp's material)
        rejected(lib.pine_gpu_test_choose_lobe(one._h, 0, fp(emissive), 1, fp(big)), "pine_gpu_test_choose_lobe: a case names no material that has a lobe")
        rejected(lib.pine_gpu_test_frame_table(cbox._h, None, 0, fp(big), None, 4, None, 4, None, 0, None), "pine_gpu_test_frame_table: bad argument")
        with pytest.raises(pa.PineError):
            pa.Plan(cbox, 0, 3)  # (samples per pixel must be positive: nothing was taken yet)


# ---- 4. the one-shot renders ---------------------------------------------------------------------------------------------------
def test_one_shot_renders_leave_blocks_in_the_pool_only():
    import pine_amd as pa
    from pine_amd import _lib, scenes
    sc = scenes.cbox((32, 32))
    with nothing_left_behind() as before:
        a = pa.PathIntegrator(pa.BlueSampler(8), 3, specialize=False).render(sc).pixels
        assert live()[0] == before
        b = pa.AOIntegrator(pa.BlueSampler(16)).render(sc).pixels
        assert live()[0] == before
        assert np.isfinite(a).all() and np.isfinite(b).all()
        _lib.lib.pine_gpu_release_cached_memory()
        assert live() == (before, 0)
