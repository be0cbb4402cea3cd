"""DenoiseIntegrator's guide images on the GPU: the albedo and normal images the real reference's DenoiseIntegrator hands to its
denoise() (tests/golden/denoise_*.npz, written by a driver that defines that function), bit for bit and without a tolerance,
from the library's choice of kernel and from every precompiled guide variant that covers the scene; a 1x1 and an 8x1 film; the
device-output entry point; the refusals.  No fixture carries a tie pixel: the pass runs in pine-BVH order only."""
import ctypes as C

import numpy as np
import pytest

import denoise_scenes as S
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

FIXTURES = list(S.DENOISE_FILMS) + list(S.GUIDES_ONLY)
F_LDS_SCENE, F_NODES, F_MESH, F_XSHAPES = 1 << 8, 1 << 9, 1 << 5, 1 << 11
# what a scene needs of a guide kernel beyond the analytic shapes (pine_guides_kernel.h)
NEEDS = {"mats_zoo_64": F_NODES, "xshapes_48": F_NODES | F_XSHAPES, "sss_48": F_MESH}


def variants_of(name):
    """None (the library's choice) and the index of every variant that covers the scene."""
    import pine_amd as pa
    need = NEEDS.get(name, 0)
    return [None] + [i for i, f in enumerate(pa.api.guides_variants()) if need & ~f == 0]


def test_the_variant_table():
    import pine_amd as pa
    table = pa.api.guides_variants()
    assert len(table) == 4 and len(set(table)) == 4
    assert [bool(f & F_LDS_SCENE) for f in table] == [True, True, False, False]
    assert [bool(f & F_NODES) for f in table] == [False, True, False, True]
    assert all(table[i] & F_MESH and table[i] & F_XSHAPES for i in (2, 3))
    # every fixture is rendered by at least one pinned variant, and all four are used
    used = set()
    for name in FIXTURES:
        v = variants_of(name)[1:]
        assert len(v) >= 1
        used.update(v)
    assert used == {0, 1, 2, 3}


@pytest.mark.parametrize("name", FIXTURES)
def test_guides_are_the_reference_guides(name, monkeypatch):
    import pine_amd as pa
    want = S.load(name)
    assert want["tie_pixels"].shape[0] == 0
    scene = S.denoise_scene(name)
    assert scene.describe() == want["pscene"]
    for variant in variants_of(name):
        if variant is None:
            monkeypatch.delenv("PINE_GPU_GUIDES_VARIANT", raising=False)
        else:
            monkeypatch.setenv("PINE_GPU_GUIDES_VARIANT", str(variant))
        albedo, normal = pa.guides(scene)
        assert_bit_equal(albedo, want["albedo"], f"{name} albedo, variant {variant}")
        assert_bit_equal(normal, want["normal"], f"{name} normal, variant {variant}")


def test_a_pinned_variant_that_does_not_cover_the_scene_is_refused(monkeypatch):
    import pine_amd as pa
    monkeypatch.setenv("PINE_GPU_GUIDES_VARIANT", "0")
    with pytest.raises(pa.PineError, match="PINE_GPU_GUIDES_VARIANT"):
        pa.guides(S.denoise_scene("sss_48"))


def test_device_entry_point_writes_the_same_bytes():
    import torch
    import pine_amd as pa
    from pine_amd import _lib
    name = "cbox_ragged_45x37"
    want = S.load(name)
    scene = S.denoise_scene(name)
    h, w = want["albedo"].shape[:2]
    albedo = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
    normal = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
    prm = _lib.RenderParams(1, 1, 0, 0, 1, 0, 0, 0)
    _lib.check(_lib.lib.pine_gpu_guides_render_device(scene._h, C.byref(prm), C.c_void_p(albedo.data_ptr()), C.c_void_p(normal.data_ptr()),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "guides")
    host_albedo, host_normal = pa.guides(scene)
    assert_bit_equal(albedo.cpu().numpy(), host_albedo, "albedo: device output against host output")
    assert_bit_equal(normal.cpu().numpy(), host_normal, "normal: device output against host output")
    assert_bit_equal(host_albedo, want["albedo"], name)


def test_refusals():
    import pine_amd as pa
    from pine_amd import _lib
    scene = S.denoise_scene("cbox_8x1")
    with pytest.raises(pa.PineError, match="PINE_GPU_FLAG_ORDER_EMBREE refused"):
        pa.guides(scene, order="embree")
    with pytest.raises(pa.PineError, match="PINE_GPU_FLAG_FAST is not available"):
        pa.guides(scene, flags=_lib.FLAG_FAST)
    with pytest.raises(pa.PineError, match="_SPECIALIZE"):
        pa.guides(scene, flags=_lib.FLAG_SPECIALIZE)
    albedo = np.zeros((1, 8, 3), np.float32)
    normal = np.zeros((1, 8, 3), np.float32)
    prm = _lib.RenderParams(1, 1, 0, 1, 2, 0, 0, 0)  # shard 1 of 2
    rc = _lib.lib.pine_gpu_guides_render(scene._h, C.byref(prm), albedo.ctypes.data_as(_lib.c_f_p), normal.ctypes.data_as(_lib.c_f_p))
    assert rc < 0 and "sharded films are not supported" in _lib.last_error()
    with pytest.raises(pa.PineError, match="no camera"):
        pa.guides(pa.Scene())
