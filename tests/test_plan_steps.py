"""What the shared build steps of path plans, AOIntegrator plans, the guide pass, Accel and Shader (pine_plan_steps.h) promise a
caller on a machine without a device: each hot path's own "no HIP device available" text, and an integrator's refusals before it."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from pine_amd import scenes
    return scenes.cbox((16, 16))


def _params(flags=0, shard_rank=0, shard_world=1):
    from pine_amd import _lib
    return _lib.RenderParams(16, 4, 0, shard_rank, shard_world, 0, flags, 0)


def _guides(scene, prm, device_pointers):
    """pine_gpu_guides_render into host images, or pine_gpu_guides_render_device (its refusals come before anything touches
    the pointers, which are host memory here)."""
    from pine_amd import _lib
    albedo, normal = np.zeros((16, 16, 3), np.float32), np.zeros((16, 16, 3), np.float32)
    if device_pointers:
        return _lib.lib.pine_gpu_guides_render_device(scene._h, C.byref(prm), C.c_void_p(albedo.ctypes.data), C.c_void_p(normal.ctypes.data), None)
    return _lib.lib.pine_gpu_guides_render(scene._h, C.byref(prm), albedo.ctypes.data_as(_lib.c_f_p), normal.ctypes.data_as(_lib.c_f_p))


def test_each_hot_path_names_itself_when_there_is_no_device(no_device):
    from pine_amd import _lib
    lib, scene = _lib.lib, no_device
    text = "no HIP device available: %s requires an AMD GPU (no CPU fallback)"
    assert not lib.pine_gpu_plan_create(scene._h, C.byref(_params()))
    assert _lib.last_error() == text % "the PathIntegrator hot path"
    assert not lib.pine_gpu_ao_plan_create(scene._h, C.byref(_params()))
    assert _lib.last_error() == text % "the AOIntegrator hot path"
    for device_pointers in (False, True):
        assert _guides(scene, _params(), device_pointers) < 0
        assert _lib.last_error() == text % "the guide images' hot path"
    assert not lib.pine_gpu_accel_create(scene._h, 0, 0)
    assert _lib.last_error() == text % "Accel's ray queries"
    assert not lib.pine_gpu_shader_create(scene._h, C.byref(_params()))
    assert _lib.last_error() == text % "Shader's vertex queries"


def test_refusals_come_before_the_device_check(no_device):
    from pine_amd import _lib
    lib, scene = _lib.lib, no_device
    ao = {_lib.FLAG_ORDER_EMBREE: "AOIntegrator renders in pine-BVH order only, AOIntegrator(BVH(), sampler): EmbreeAccel answers hit8 with Embree's "
                                  "packet traversal, which is not restated (PINE_GPU_FLAG_ORDER_EMBREE refused)",
          _lib.FLAG_FAST: "AOIntegrator: PINE_GPU_FLAG_FAST / _VERTEX_LOG / _SPECIALIZE are not available (exact arithmetic, precompiled kernels only)"}
    for flags, why in ao.items():
        assert not lib.pine_gpu_ao_plan_create(scene._h, C.byref(_params(flags)))
        assert _lib.last_error() == why
    guides = [(_params(_lib.FLAG_ORDER_EMBREE), "DenoiseIntegrator's guide images are rendered in pine-BVH order only, DenoiseIntegrator(BVH(), ...): "
                                                "EmbreeAccel's order would need fixtures of the Embree build and its tie pixels (PINE_GPU_FLAG_ORDER_EMBREE refused)"),
              (_params(_lib.FLAG_FAST), "guide images: PINE_GPU_FLAG_FAST is not available (the guide images are exact; there is no declared-tolerance kernel)"),
              (_params(0, 1, 2), "guide images: sharded films are not supported (shard_world must be 1)")]
    for prm, why in guides:
        assert _guides(scene, prm, True) < 0
        assert _lib.last_error() == why
    # (parameters every integrator checks alike, check_params: before the device too)
    assert not lib.pine_gpu_plan_create(scene._h, C.byref(_params(0, 2, 2)))
    assert _lib.last_error() == "bad shard rank/world"
