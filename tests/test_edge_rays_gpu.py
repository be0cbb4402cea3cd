"""GPU (-m gpu): the device shape tests, both traversal orders of Accel, the generic walks and the baked walk against the REAL
reference's answers to the edge rays (tests/edge_rays.py, tests/golden/*_edge.npz): tmin > 0, scaled and axis-parallel directions
with signed zeros, origins on a surface, spans that end exactly at a hit.  Bit for bit; the cap on mismatching rays is zero."""
import ctypes as C

import numpy as np
import pytest

from accel_scenes import ORDERS, accel_scene, records_as_words
from conftest import assert_bit_equal
from edge_rays import ACCEL_SCENES, CLASSES, SHAPE_FILES, TRAV_SCENES, class_of, load_edge, shape_scene
from test_bvh_fixtures import _parse_trav
from test_edge_rays import shape_differences

pytestmark = pytest.mark.gpu
ORDER_NAME = {"bvh": "pine", "embree": "embree"}
# Classes whose answers are unspecified under PINE_GPU_FLAG_ORDER_EMBREE (include/pine_gpu.h): whole classes only, at
# most three, each with the place in the reference's Embree that decides them.  Pine-BVH order leaves nothing out.
EMBREE_UNSPECIFIED = {
    # the class holds the rays with a negative tmin.  Embree requires tnear >= 0 (src/contrib/embree/kernels/bvh/bvh_intersector1.cpp:61),
    # clamps it to 0 for its node boxes (:65) and compares the unclamped value in its triangle test
    # (kernels/geometry/triangle_intersector_moeller.h:104): a triangle behind the origin is hit where Embree's own hierarchy happens
    # to reach its leaf (sss_mesh ray 631 and mesh_attrs ray 616 of the fixtures report t < 0), and that hierarchy is not restated.
    "span_degenerate": "negative tmin: bvh_intersector1.cpp:61-65 against triangle_intersector_moeller.h:104",
}


def _first(bad, cls):
    r = int(np.nonzero(bad)[0][0])
    per_class = {name: int(bad[class_of(cls, name)].sum()) for name in CLASSES if bad[class_of(cls, name)].any()}
    return r, f"{int(bad.sum())} of {len(bad)} rays differ, per class {per_class}; first ray {r} ({CLASSES[cls[r]]})"


@pytest.mark.parametrize("which", list(SHAPE_FILES))
def test_device_shape_records_on_edge_rays(which):
    """pine_gpu_test_shapes against `pine_ref shapes`, by the rules of tests/test_gpu_parity.py::test_device_shape_records: hit,
    intersect and tmax for every (shape, ray), p, n and uv on hits."""
    from pine_amd import _lib
    fx = load_edge(SHAPE_FILES[which])
    rec, rays = fx["shape_records"], fx["rays"]
    sc = shape_scene(which)
    assert sc.describe() == fx["pscene"]
    out = np.zeros_like(rec)
    _lib.check(_lib.lib.pine_gpu_test_shapes(sc._h, 0, rays.ctypes.data_as(_lib.c_f_p), len(rays), out.ctypes.data_as(_lib.c_f_p), out.size))
    kinds = [line.split()[1] for line in fx["pscene"].splitlines() if line.startswith("shape ")]
    msg = shape_differences(out, rec, fx["cls"], kinds)
    assert not msg, msg
    hit = rec[..., 1] == 1
    assert_bit_equal(out[..., :3], rec[..., :3], "hit / intersect / tmax")
    assert_bit_equal(out[hit][:, 3:9], rec[hit][:, 3:9], "surface p, n")
    assert_bit_equal(out[hit][:, 9:], rec[hit][:, 9:], "surface uv")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ACCEL_SCENES)
def test_accel_records_equal_the_references_on_edge_rays(name, order):
    """All 12 words of intersect and the byte of hit for every edge ray, under Accel(BVH()) and under Accel(EmbreeAccel())."""
    import pine_amd as pa
    fx = load_edge(f"accel_{name}_{order}_edge")
    sc = accel_scene(name)
    assert sc.describe() == fx["pscene"]
    rays, cls = fx["rays"], fx["cls"]
    with pa.Accel(sc, order=ORDER_NAME[order]) as accel:
        got, occ = records_as_words(accel.intersect(rays)).copy(), accel.hit(rays).view(np.uint8).copy()
    judged = np.ones(len(rays), bool)
    if order == "embree":
        for cname in EMBREE_UNSPECIFIED:
            judged &= ~class_of(cls, cname)
    bad = (got != fx["records"]).any(axis=1) & judged
    if bad.any():
        r, msg = _first(bad, cls)
        raise AssertionError(f"{name}, {order}: intersect: {msg}: ray {rays[r].tolist()} gives {got[r].tolist()}, the reference {fx['records'][r].tolist()}")
    bad = (occ != fx["occluded"]) & judged
    if bad.any():
        r, msg = _first(bad, cls)
        raise AssertionError(f"{name}, {order}: hit: {msg}: ray {rays[r].tolist()} gives {occ[r]}, the reference {fx['occluded'][r]}")


def _trav_words(fx):
    """-> per ray (hit, geometry or 0, t bits, any hit) of the fixture's `pine_ref bvh` stream, and the parsed stream."""
    ref = _parse_trav(fx["trav"], len(fx["rays"]))
    return np.array([[res[0], res[1], res[3], h] for _, res, _, h in ref], dtype=np.uint32), ref


@pytest.mark.parametrize("flat", [0, 1])
@pytest.mark.parametrize("name", TRAV_SCENES)
def test_device_traversal_order_on_edge_rays(name, flat):
    """pine_gpu_test_traverse, nested (flat = 0) and flat (flat = 1), against `pine_ref bvh` on the edge rays of the scenes with
    order-dependent scaled boxes: every primitive test in order, the winner, its t bits and the any-hit answer."""
    from pine_amd import _lib
    fx = load_edge(f"accel_{name}_bvh_edge")
    sc = accel_scene(name)
    assert sc.describe() == fx["pscene"]
    rays, cls = fx["rays"], fx["cls"]
    _, ref = _trav_words(fx)
    cap = 2 + max(max(len(c), len(a)) for c, _, a, _ in ref)
    out = np.zeros((len(rays), 2 * cap + 5), np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_traverse(sc._h, 0, rays.ctypes.data_as(_lib.c_f_p), len(rays), flat, cap, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    for r, (c, res, a, h) in enumerate(ref):  # (no meshes in these scenes: the triangle word means nothing)
        o = out[r]
        where = f"ray {r} ({CLASSES[cls[r]]}) {rays[r].tolist()}"
        assert int(o[0]) == len(c) and np.array_equal(o[1:1 + len(c)], c), f"{where}: closest-hit test order {o[1:1 + int(o[0])].tolist()} vs {c.tolist()}"
        assert (int(o[cap]), int(o[cap + 1]), int(o[cap + 3])) == (res[0], res[1], res[3]), f"{where}: closest-hit result"
        assert int(o[2 * cap + 4]) == h, f"{where}: any-hit result"
        assert int(o[cap + 4]) == len(a) and np.array_equal(o[cap + 5:cap + 5 + len(a)], a), f"{where}: any-hit test order"


def test_baked_traversal_equals_the_reference_on_edge_rays():
    """The walk compiled into the specialised Cornell box against the reference's words directly (elsewhere it is compared with
    the generic walk): the rays inside its documented precondition, tmin >= 0 and |d| <= 1 (pine_device.h box_slabs_minmax) --
    of scaled_dir the factors below 1, of span_degenerate all but the negative tmin."""
    import pine_amd as pa
    from pine_amd import _lib
    fx = load_edge("accel_cbox_bvh_edge")
    sc = accel_scene("cbox")
    assert sc.describe() == fx["pscene"]
    cls = fx["cls"]
    want, _ = _trav_words(fx)
    norm = np.linalg.norm(fx["rays"][:, 3:6].astype(np.float64), axis=1)
    keep = ~(class_of(cls, "scaled_dir") & (norm > 1.5)) & ~(class_of(cls, "span_degenerate") & (fx["rays"][:, 6] < 0))
    assert (norm[keep] < 1 + 1e-6).all() and (fx["rays"][keep, 6] >= 0).all() and keep.sum() > 0.9 * len(keep)
    assert all((keep & class_of(cls, name)).any() for name in CLASSES)
    rays = np.ascontiguousarray(fx["rays"][keep])
    plan = pa.Plan(sc, 1, 1, specialize=True)
    assert plan.stats().specialized == 2
    baked = np.zeros((len(rays), 4), dtype=np.uint32)
    _lib.check(_lib.lib.pine_gpu_plan_test_traverse_baked(plan._h, rays.ctypes.data_as(_lib.c_f_p), len(rays), baked.ctypes.data_as(C.POINTER(C.c_uint32))))
    plan.close()
    bad = (baked != want[keep]).any(axis=1)
    if bad.any():
        r, msg = _first(bad, cls[keep])
        raise AssertionError(f"{msg}: ray {rays[r].tolist()} gives {baked[r].tolist()}, the reference {want[keep][r].tolist()}")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", ["cbox", "mesh_attrs"])
def test_classes_together_answer_as_each_class_alone(name, order):
    """No effect across lanes from a lane that leaves the walk early (a degenerate span, a miss of the root box): the scene-in-LDS
    variant and the global-memory one, both orders."""
    import pine_amd as pa
    fx = load_edge(f"accel_{name}_{order}_edge")
    rays, cls = fx["rays"], fx["cls"]
    with pa.Accel(accel_scene(name), order=ORDER_NAME[order]) as accel:
        whole, occ = records_as_words(accel.intersect(rays)).copy(), accel.hit(rays).view(np.uint8).copy()
        for cname in CLASSES:
            m = class_of(cls, cname)
            if not m.any():
                continue
            part = np.ascontiguousarray(rays[m])
            assert np.array_equal(records_as_words(accel.intersect(part)), whole[m]), cname
            assert np.array_equal(accel.hit(part).view(np.uint8), occ[m]), cname
