"""Accel, the batched ray queries (include/pine_gpu.h pine_gpu_accel_*): what can be said without a GPU -- the argument checks of
the C entry points and of the Python wrapper, the refusals, and the new fixtures against the committed ones of the same scenes
(two runs of the real reference, by two drivers)."""
import ctypes as C
import os

import numpy as np
import pytest

from accel_scenes import CROSS_RAYS, NUM_RAYS, ORDERS, SAME_AS_BVH_FIXTURE, SEEDS, accel_rays, accel_scene, load_fixture
from conftest import GOLDEN
from test_bvh_fixtures import _parse_trav


def _lib():
    from pine_amd import _lib
    return _lib


def _err(rc):
    assert rc < 0
    return _lib().last_error()


def test_ray_count_and_pointers_are_checked_before_anything_else():
    """n < 0, n > 2^31 - 1, null and misaligned buffers fail with a message -- before the accel is looked at, so no device is
    needed to see it; a null accel fails too, whatever n is."""
    lib = _lib().lib
    buf = (C.c_float * 64)()
    base = C.addressof(buf)
    aligned = C.c_void_p((base + 15) & ~15)
    odd = C.c_void_p(((base + 15) & ~15) + 4)
    for n in (-1, 2 ** 31, 2 ** 40):
        assert "[0, 2^31 - 1]" in _err(lib.pine_gpu_accel_intersect_device(None, aligned, n, aligned, None))
        assert "[0, 2^31 - 1]" in _err(lib.pine_gpu_accel_hit_device(None, aligned, n, aligned, None))
        assert "[0, 2^31 - 1]" in _err(lib.pine_gpu_accel_intersect(None, buf, n, aligned))
        assert "[0, 2^31 - 1]" in _err(lib.pine_gpu_accel_hit(None, buf, n, C.cast(aligned, C.POINTER(C.c_uint8))))
    assert "null" in _err(lib.pine_gpu_accel_intersect_device(None, None, 4, aligned, None))
    assert "null" in _err(lib.pine_gpu_accel_intersect_device(None, aligned, 4, None, None))
    assert "16-byte aligned" in _err(lib.pine_gpu_accel_intersect_device(None, odd, 4, aligned, None))
    assert "16-byte aligned" in _err(lib.pine_gpu_accel_intersect_device(None, aligned, 4, odd, None))
    assert "16-byte aligned" in _err(lib.pine_gpu_accel_hit_device(None, odd, 4, aligned, None))
    assert "16-byte aligned" in _err(lib.pine_gpu_accel_camera_rays_device(None, odd, None))
    for n in (0, 4, 2 ** 31 - 1):  # (n == 0 launches nothing, but a null accel is no accel)
        assert "null" in _err(lib.pine_gpu_accel_intersect_device(None, aligned, n, aligned, None))
        assert "null" in _err(lib.pine_gpu_accel_hit_device(None, aligned, n, odd, None))  # (the bytes need no alignment)
    assert "null" in _err(lib.pine_gpu_accel_camera_rays_device(None, aligned, None))
    assert "null" in _err(lib.pine_gpu_accel_info(None, (C.c_int32 * 4)()))
    lib.pine_gpu_accel_destroy(None)  # (a no-op)
    assert not lib.pine_gpu_accel_create(None, 0, 0) and "null" in _lib().last_error()


def test_refused_flags_are_refused_by_name():
    """PINE_GPU_FLAG_FAST, _SPECIALIZE, _VERTEX_LOG and every bit that is not _ORDER_EMBREE: no accel, a message that names the
    flag -- checked before the device is asked for."""
    L = _lib()
    from pine_amd import scenes
    sc = scenes.cbox((16, 16))
    for flag, word in ((L.FLAG_FAST, "PINE_GPU_FLAG_FAST"), (L.FLAG_SPECIALIZE, "_SPECIALIZE"), (L.FLAG_VERTEX_LOG, "_VERTEX_LOG"),
                       (L.FLAG_FAST | L.FLAG_ORDER_EMBREE, "PINE_GPU_FLAG_FAST"), (L.FLAG_TIMING, "0 or PINE_GPU_FLAG_ORDER_EMBREE"),
                       (L.FLAG_DEVICE_BVH, "0 or PINE_GPU_FLAG_ORDER_EMBREE"), (0x80000000, "0 or PINE_GPU_FLAG_ORDER_EMBREE")):
        assert not L.lib.pine_gpu_accel_create(sc._h, 0, flag)
        assert word in L.last_error(), (hex(flag), L.last_error())
    import pine_amd as pa
    with pytest.raises(pa.PineError, match="unknown traversal order"):
        pa.Accel(sc, order="morton")


def test_no_device_means_loud_failure():
    """No CPU path behind Accel: where there is no GPU, creation raises; where there is one, a device that does not exist does."""
    import torch
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((16, 16))
    if torch.cuda.is_available():
        with pytest.raises(pa.PineError, match="(?i)device|hip"):
            pa.Accel(sc, device=4096)
        return
    for order in ("pine", "embree"):
        with pytest.raises(pa.PineError, match="no HIP device"):
            pa.Accel(sc, order=order)


def test_wrapper_refuses_rays_of_the_wrong_kind():
    """dtype, shape, contiguity and (for tensors) the device are checked in Python, before any call into the library."""
    import torch
    from pine_amd import api
    ok = np.zeros((5, 8), np.float32)
    assert api._check_rays(ok) is False
    assert api._check_rays(np.zeros((0, 8), np.float32)) is False
    for bad in (ok.astype(np.float64), np.zeros((5, 7), np.float32), np.zeros((40,), np.float32), np.zeros((5, 8, 1), np.float32),
                np.zeros((5, 16), np.float32)[:, ::2], np.asfortranarray(np.zeros((5, 8), np.float32)), ok.tolist(), None):
        with pytest.raises(ValueError, match="Accel: rays"):
            api._check_rays(bad)
    for bad in (torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 7)), torch.zeros((40,)), torch.zeros((5, 8))):  # (the last: a CPU tensor)
        with pytest.raises(ValueError, match="Accel: "):
            api._check_rays(bad, 0)
    assert api.HIT_DTYPE.itemsize == 48 and api.HIT_DTYPE.names == ("t", "geometry", "triangle", "material", "p", "n", "uv")
    assert [api.HIT_DTYPE.fields[k][1] for k in api.HIT_DTYPE.names] == [0, 4, 8, 12, 16, 28, 40]


@pytest.mark.parametrize("name", list(SEEDS))
def test_fixture_is_of_this_scene_and_these_rays(name):
    """Each fixture describes the scene the tests build and holds the rays the generator's seed gives -- a sample is regenerated
    seed for seed --, in both orders alike; a record is well formed: a miss keeps its tmax and holds -1 -1 -1 and zeros, a hit
    has indices of the scene and is seen by the any-hit query."""
    sc = accel_scene(name)
    want = accel_rays(sc, name)
    for order in ORDERS:
        fx = load_fixture(name, order)
        assert fx["pscene"] == sc.describe()
        rays, rec, occ = fx["rays"], fx["records"], fx["occluded"]
        assert rays.shape == (NUM_RAYS, 8) and rec.shape == (NUM_RAYS, 12) and rec.dtype == np.uint32 and occ.shape == (NUM_RAYS,)
        assert os.path.getsize(os.path.join(GOLDEN, f"accel_{name}_{order}.npz")) < 100 * 1024
        sample = np.r_[0:40, 480:520, 960:1000]
        assert np.array_equal(rays[sample].view(np.uint32), want[sample].view(np.uint32))
        geom = rec[:, 1].view(np.int32)
        hit = geom >= 0
        assert 0.1 * NUM_RAYS <= hit.sum() <= 0.95 * NUM_RAYS
        assert (geom[~hit] == -1).all() and (rec[~hit, 2:4].view(np.int32) == -1).all() and (rec[~hit, 4:] == 0).all()
        assert np.array_equal(rec[~hit, 0], rays[~hit, 7].view(np.uint32))
        assert (rec[hit, 0].view(np.float32) < rays[hit, 7]).all() and (rec[hit, 0].view(np.float32) > rays[hit, 6]).all()
        assert (rec[hit, 3].view(np.int32) >= 0).all()
        assert (occ[hit] == 1).all() and set(np.unique(occ)) <= {0, 1}
        n = rec[hit, 7:10].view(np.float32).astype(np.float64)
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)  # (it.n is a unit vector, interpolated or not)


@pytest.mark.parametrize("name", list(SAME_AS_BVH_FIXTURE))
def test_driver_agrees_with_the_committed_bvh_fixture(name):
    """One run of the reference against another: on the first rays of tests/golden/bvh_<scene>.npz the accel driver's hit,
    geometry, triangle (on mesh hits), t bits and any-hit byte equal the words `pine_ref bvh` wrote."""
    z = np.load(os.path.join(GOLDEN, f"bvh_{SAME_AS_BVH_FIXTURE[name]}.npz"))
    a = np.load(os.path.join(GOLDEN, f"accel_{name}_bvh.npz"))
    assert str(z["pscene"]) == a["pscene"].tobytes().decode()
    rec, occ = a["cross_records"], a["cross_occluded"]
    assert rec.shape == (CROSS_RAYS, 12)
    ref = _parse_trav(z["trav"], len(z["rays"]))[:CROSS_RAYS]
    pscene = str(z["pscene"])
    mesh_hits = 0
    for r, (_, (hit, geom, tri, tbits), _, any_hit) in enumerate(ref):
        assert (int(rec[r, 1].view(np.int32)) >= 0) == bool(hit), f"ray {r}: hit"
        assert int(rec[r, 0]) == tbits, f"ray {r}: t"
        assert int(occ[r]) == any_hit, f"ray {r}: any hit"
        if hit:
            assert int(rec[r, 1]) == geom, f"ray {r}: geometry"
            if int(rec[r, 2].view(np.int32)) >= 0:  # (a mesh hit: elsewhere the reference's triangle word means nothing)
                assert int(rec[r, 2]) == tri, f"ray {r}: triangle"
                mesh_hits += 1
    if "mesh" in name:
        assert mesh_hits > 0 and "mesh" in pscene
