"""The steps the small hosts share (pine_plan_steps.h, pine_scene_steps.h), on the GPU: the exact texts of the variant refusals
of every family; the dynamic-LDS limit of a kernel, which a second, smaller object on the same kernel must never lower under a
live larger one; two accels on two devices."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE = ("cbox", {}), ("cbox_clutter", {"extra": 24})
# Path plans: the 24 extra primitives bring Spheres, which the Cornell box's path kernel (features 0x102) does not take -- the two
# plans would run different kernels (0x205f / 0x102) and show nothing.  With one extra primitive, a rotated Box, both run the
# kernel 0x102, on 137 600 and 132 752 bytes of LDS.
LARGE_PATH = ("cbox_clutter", {"extra": 1})
KNOBS = ("PINE_GPU_TEST_VARIANT", "PINE_GPU_AO_VARIANT", "PINE_GPU_AO_KERNEL", "PINE_GPU_GUIDES_VARIANT", "PINE_GPU_ACCEL_VARIANT",
         "PINE_GPU_SHADER_VARIANT", "PINE_GPU_KERNEL", "PINE_GPU_SPECIALIZE")


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _scene(which):
    from pine_amd import scenes
    name, kw = which
    return getattr(scenes, name)((16, 16), **kw)


# ---- 1. the variant refusals, whole ---------------------------------------------------------------------------------------------
def test_variant_refusals_word_for_word(monkeypatch):
    import pine_amd as pa
    from pine_amd import scenes
    mesh = scenes.sss((16, 16), 1)
    pinned = "$PINE_GPU_%s_VARIANT names no %s kernel variant that covers this scene"
    cases = [("AO", "9999", "AOIntegrator: " + pinned % ("AO", "AO"), lambda: pa.Plan(scenes.cbox((16, 16)), pa.BlueSampler(4), 1, integrator="ao")),
             # (variant 0 of each of these takes analytic shapes only / no Uber material and no node program)
             ("GUIDES", "0", "guides: " + pinned % ("GUIDES", "guide"), lambda: pa.guides(mesh)),
             ("ACCEL", "0", "Accel: " + pinned % ("ACCEL", "Accel"), lambda: pa.Accel(mesh)),
             ("SHADER", "0", "Shader: " + pinned % ("SHADER", "Shader"), lambda: pa.Shader(scenes.materials_zoo((16, 16)), pa.BlueSampler(4), 3)),
             # (variant 3 covers every shape kind -- in EmbreeAccel's order)
             ("ACCEL", "3", "Accel: $PINE_GPU_ACCEL_VARIANT names a variant of the other traversal order", lambda: pa.Accel(scenes.cbox((16, 16))))]
    for family, index, text, create in cases:
        monkeypatch.setenv(f"PINE_GPU_{family}_VARIANT", index)
        with pytest.raises(pa.PineError) as e:
            create()
        monkeypatch.delenv(f"PINE_GPU_{family}_VARIANT")
        assert str(e.value) == text


# ---- 2. the LDS limit is never lowered ---------------------------------------------------------------------------------------------
def _launch_plan(plan):
    import torch
    film = torch.full((16, 16, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    plan.check()  # (raises if the launch was refused or the kernel gave up)
    st = plan.stats()
    return film.cpu().numpy().view(np.uint32), (st.camera_samples, st.vertices, st.shadow_rays, st.walk_steps)


def _query_accel(accel):
    import torch
    hits = accel.intersect(accel.camera_rays(tensor=True)).records
    torch.cuda.synchronize()
    return hits.cpu().numpy().view(np.uint32), None


def _shared_kernel(larger, smaller, of):
    """The preconditions: one kernel under both objects, the larger one's dynamic LDS the larger."""
    (fl, ll), (fs, ls) = of(larger), of(smaller)
    print(f"kernel_features {fl:#x} / {fs:#x}, lds_bytes {ll} / {ls}")
    assert fl == fs, "the two objects do not share a kernel"
    assert ll > ls, "the larger object does not ask for more LDS"


def _plan_kernel(plan):
    st = plan.stats()
    return int(st.kernel_features), int(st.lds_bytes)


# (a path plan keeps to the precompiled kernel, specialize=False: the scene's own kernel is another function)
FAMILIES = {"path": (lambda pa, sc: pa.Plan(sc, pa.BlueSampler(4), 3, specialize=False), _launch_plan, _plan_kernel, LARGE_PATH),
            "ao": (lambda pa, sc: pa.Plan(sc, pa.BlueSampler(4), 1, integrator="ao"), _launch_plan, _plan_kernel, LARGE),
            "accel": (lambda pa, sc: pa.Accel(sc), _query_accel, lambda a: (a.kernel_features, a.lds_bytes), LARGE)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_smaller_object_does_not_lower_the_lds_limit_of_a_live_larger_one(family):
    import pine_amd as pa
    create, run, kernel_of, large = FAMILIES[family]
    larger = create(pa, _scene(large))
    first, first_stats = run(larger)
    smaller = create(pa, _scene(SMALL))
    _shared_kernel(larger, smaller, kernel_of)
    run(smaller)
    again, again_stats = run(larger)
    assert np.array_equal(again, first) and again_stats == first_stats
    smaller.close(), larger.close()


# ---- 3. two devices -----------------------------------------------------------------------------------------------------------------
def test_an_accel_on_each_of_two_devices():
    import torch
    import pine_amd as pa
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two devices")
    try:
        with pa.Accel(_scene(LARGE), device=0) as a0, pa.Accel(_scene(LARGE), device=1) as a1:
            answers = []
            for device, accel in enumerate((a0, a1)):
                hits = accel.intersect(accel.camera_rays(tensor=True)).records
                assert hits.device.index == device
                answers.append(hits.cpu().numpy().view(np.uint32))
        assert np.array_equal(answers[0], answers[1])
    finally:
        torch.cuda.set_device(0)  # (the library made device 1 the thread's current one)
