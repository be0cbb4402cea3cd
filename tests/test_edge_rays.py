"""The edge-ray fixtures (tests/golden/*_edge.npz, tools/make_golden_edge.py: the REAL reference's answers to tmin > 0, scaled and
axis-parallel directions, origins on a surface, spans that end exactly at a hit) -- what can be said without a GPU: every fixture
is of the scene and the rays the tests build, its `info` meets the generator's conditions, its records are well formed, two runs
of the reference agree, and the oracle restatement (oracle/pine_oracle.cpp) equals the per-shape records bit for bit."""
import json
import os

import numpy as np
import pytest

from accel_scenes import ORDERS, accel_scene
from edge_rays import (ACCEL_SCENES, CLASSES, EDGE_SEEDS, FLT_MAX, NUM_BASE, PER_CLASS, SHAPE_FILES, TRAV_SCENES, at_hit_values, base_rays, class_of,
                       edge_rays, fixture_parts, load_edge, regenerate, shape_scene)
from test_bvh_fixtures import _parse_trav

HITS_ONLY = ("on_surface", "inside")
# shape kinds whose t the reference itself reports outside [tmin, tmax] on some edge rays, and where
OUT_OF_SPAN = {
    "obb": "OBB::intersect returns the box's far t where the near one is not above tmin, in units of the normalised direction (bbox.cpp:164-166)",
    "cylinder": "the second root is taken where the first is below tmin and is not compared with tmin again (geometry.cpp:505-506)",
    "plane": "a ray inside the plane divides by zero; an infinite t passes `t < tmin || t > tmax` only as NaN does not (geometry.cpp:41-43)",
}


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_rays(sc, seed, fx):
    """The stored rays are the generator's, seed for seed; the one-pass rays need no first pass; each two-pass word is the stated
    function of the stored first-pass record."""
    rays, cls, fp = fx["rays"], fx["cls"], fx["first_pass"]
    want, wcls, two = regenerate(sc, seed, fx)
    assert rays.dtype == np.float32 and rays.shape == want.shape and len(rays) <= 2000 and fp.shape == (NUM_BASE, 12)
    assert np.array_equal(cls, wcls) and np.array_equal(_u32(rays), _u32(want))
    assert np.isfinite(rays).all() and (rays[:, 3:6] != 0).any(axis=1).all()
    for ci, name in enumerate(CLASSES):
        k = int((cls == ci).sum())
        assert k == PER_CLASS or (name == "inside" and k == 0), (name, k)
    assert int((fx["redraw"] > 0).sum()) <= 0.02 * PER_CLASS * len(CLASSES)
    # without the first pass: the same one-pass rays (a redrawn ray is its class drawn anew: compared above)
    alone, acls = edge_rays(sc, seed)
    keep = ~two
    assert np.array_equal(acls, cls[keep])
    same = fx["redraw"][keep] == 0
    assert np.array_equal(_u32(alone)[same], _u32(rays[keep])[same])
    # the two-pass words, straight from the stored first pass
    base = base_rays(sc, seed)
    hit_t = {int(t) for t in fp[fp[:, 1].view(np.int32) >= 0, 0]}
    hit_p = {tuple(int(x) for x in p) for p in fp[fp[:, 1].view(np.int32) >= 0, 4:7]}
    for name, word in (("tmin_at_hit", 6), ("tmax_at_hit", 7)):
        r = rays[class_of(cls, name)].reshape(-1, 5, 8)
        whole = (fx["redraw"][class_of(cls, name)].reshape(-1, 5) == 0).all(axis=1)  # (a redrawn ray belongs to another five: compared above)
        assert whole.sum() >= 0.9 * len(r)
        for group in r[whole]:
            assert int(_u32(group[0, word:word + 1])[0]) in hit_t, name  # (the first of five: the first pass's t, bit for bit)
            assert np.array_equal(_u32(group[:, word]), _u32(at_hit_values(group[0, word]))), name
            rest = [c for c in range(8) if c != word]
            assert (_u32(group[:, rest]) == _u32(group[:1, rest])).all()
            assert (_u32(base[:, rest]) == _u32(group[0, rest])).all(axis=1).any(), name  # (the rest: a base ray)
    r = rays[class_of(cls, "on_surface")]
    assert all(tuple(int(x) for x in _u32(o)) in hit_p for o in r[:, 0:3])
    assert set(np.unique(r[:, 6]).tolist()) == {0.0, float(np.float32(1e-4))} and (r[:, 7] == FLT_MAX).all()
    r = rays[class_of(cls, "span_degenerate") & two]
    assert len(r) == PER_CLASS // 8 and all(int(t) in hit_t for t in _u32(r[:, 6])) and np.array_equal(_u32(r[:, 6]), _u32(r[:, 7]))
    return two


def _check_info(info, cls):
    for name in CLASSES:
        if not class_of(cls, name).any():
            assert name == "inside" and name not in info["classes"]
            continue
        c = info["classes"][name]
        assert c["rays"] == PER_CLASS and c["hits"] >= 0.10 * c["rays"], (name, c)
        assert name in HITS_ONLY or c["rays"] - c["hits"] >= 0.05 * c["rays"], (name, c)


@pytest.mark.parametrize("which", list(SHAPE_FILES))
def test_shape_fixture_is_of_this_scene_and_these_rays(which):
    fx = load_edge(SHAPE_FILES[which])
    sc = shape_scene(which)
    assert fx["pscene"] == sc.describe()
    for p in fixture_parts(SHAPE_FILES[which]):
        assert os.path.getsize(p) < 100 * 1024
    _check_rays(sc, EDGE_SEEDS[which], fx)
    rec, cls, info = fx["shape_records"], fx["cls"], json.loads(fx["info"])
    kinds = [line.split()[1] for line in fx["pscene"].splitlines() if line.startswith("shape ")]
    assert rec.shape == (len(kinds), len(cls), 11) and set(np.unique(rec[..., :2])) <= {0.0, 1.0}
    _check_info(info, cls)
    # the classes' counts and the boundary pairs, counted again from the records
    any_hit = (rec[..., 1] == 1).any(axis=0)
    for name, c in info["classes"].items():
        assert c["hits"] == int(any_hit[class_of(cls, name)].sum()), name
    at = class_of(cls, "tmin_at_hit") | class_of(cls, "tmax_at_hit")
    differ = {}
    for s, kind in enumerate(kinds):
        differ[kind] = differ.get(kind, 0) + int((rec[s, at, 0] != rec[s, at, 1]).sum())
    assert differ == info["hit_differs_from_intersect"]
    for kind, k in differ.items():
        assert k >= 5 or (k == 0 and len(info["never_differ"][kind]) > 20), (kind, k)
    assert sum(k >= 5 for k in differ.values()) >= 2


@pytest.mark.parametrize("name", ACCEL_SCENES)
def test_accel_fixture_is_of_this_scene_and_these_rays(name):
    """As tests/test_accel.py::test_fixture_is_of_this_scene_and_these_rays, with t >= tmin where that test has t > tmin (the
    boundary classes reach equality) and t <= tmax likewise."""
    sc = accel_scene(name)
    ps = sc.describe()
    n_geoms = sum(line.startswith("shape ") for line in ps.splitlines())
    both = {}
    for order in ORDERS:
        stem = f"accel_{name}_{order}_edge"
        fx = both[order] = load_edge(stem)
        assert fx["pscene"] == ps
        for p in fixture_parts(stem):
            assert os.path.getsize(p) < 100 * 1024
        rays, cls, rec, occ, info = fx["rays"], fx["cls"], fx["records"], fx["occluded"], json.loads(fx["info"])
        if order == "bvh":
            _check_rays(sc, EDGE_SEEDS[name], fx)
        n = len(rays)
        assert rec.shape == (n, 12) and rec.dtype == np.uint32 and occ.shape == (n,) and set(np.unique(occ)) <= {0, 1}
        _check_info(info, cls)
        geom = rec[:, 1].view(np.int32)
        hit = geom >= 0
        for cname, c in info["classes"].items():
            assert c["hits"] == int(hit[class_of(cls, cname)].sum()), cname
        for cname, k in info["redraws"].items():
            assert k == int((fx["redraw"][class_of(cls, cname)] > 0).sum()) and k <= 0.02 * PER_CLASS
        t = info["tmin_random"]
        assert t["other_t_or_primitive"] >= 0.10 * t["hit_at_tmin_0"] > 0
        s = info["scaled_dir"]
        assert s["hits"] == int(hit[class_of(cls, "scaled_dir")].sum())
        assert s["same_geometry_off_sphere_and_obb"] >= 0.90 * s["hits_off_sphere_and_obb"] and s["hits_off_sphere_and_obb"] >= 10
        assert (geom[~hit] == -1).all() and (rec[~hit, 2:4].view(np.int32) == -1).all() and (rec[~hit, 4:] == 0).all()
        assert np.array_equal(rec[~hit, 0], _u32(rays[~hit, 7]))
        assert (geom[hit] < n_geoms).all() and (rec[hit, 3].view(np.int32) >= 0).all()
        # t within the span, ends included (the boundary classes reach equality) -- for the kinds whose test in the reference
        # keeps it there.  OUT_OF_SPAN names the others with the reference's line; a scaled direction adds the Sphere.
        kinds = np.array([line.split()[1] for line in ps.splitlines() if line.startswith("shape ")])
        loose = np.zeros(n, bool)
        loose[hit] = np.isin(kinds[geom[hit]], list(OUT_OF_SPAN)) | (kinds[geom[hit]] == "sphere") & class_of(cls, "scaled_dir")[hit]
        th = rec[:, 0].view(np.float32)
        ok = hit & ~loose
        with np.errstate(over="ignore"):
            above = np.nextafter(rays[:, 7], np.float32(np.inf)) if order == "embree" else rays[:, 7]  # (Embree's own triangle test: one ulp)
        assert (th[ok] <= above[ok]).all() and (th[ok] >= rays[ok, 6]).all()
        assert ok.sum() >= 100
        assert (occ[hit & ~loose] == 1).sum() >= 0.95 * (hit & ~loose).sum()  # (hit() and intersect() differ at the ends: not all)
        nrm = rec[ok, 7:10].view(np.float32).astype(np.float64)  # (a unit vector wherever t is an ordinary number)
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    for k in ("rays", "cls", "redraw", "first_pass"):
        assert np.array_equal(_u32(both["bvh"][k]) if both["bvh"][k].dtype == np.float32 else both["bvh"][k],
                              _u32(both["embree"][k]) if both["embree"][k].dtype == np.float32 else both["embree"][k]), k
    b, e = both["bvh"]["records"], both["embree"]["records"]
    hb = (b[:, 1].view(np.int32) >= 0) & (e[:, 1].view(np.int32) >= 0)
    assert not (hb & (b[:, 0] == e[:, 0]) & ((b[:, 1] != e[:, 1]) | (b[:, 2] != e[:, 2]))).any()  # (the tie rule: none in a fixture)
    # the first pass is the reference's answer to the base rays: where the plain class repeats a base ray, the records agree
    base, fp = base_rays(sc, EDGE_SEEDS[name]), both["bvh"]["first_pass"]
    plain = np.nonzero(class_of(both["bvh"]["cls"], "plain"))[0]
    index = {_u32(r).tobytes(): i for i, r in enumerate(base)}
    seen = 0
    for i in plain:
        j = index.get(_u32(both["bvh"]["rays"][i]).tobytes())
        if j is not None:
            assert np.array_equal(b[i], fp[j]), i
            seen += 1
    assert seen >= 0.98 * PER_CLASS


@pytest.mark.parametrize("name", TRAV_SCENES)
def test_trav_stream_agrees_with_the_accel_records(name):
    """Two runs of the reference on the same rays -- `pine_ref bvh` and the accel driver --: hit, geometry, t bits, any-hit."""
    fx = load_edge(f"accel_{name}_bvh_edge")
    rec, occ = fx["records"], fx["occluded"]
    ref = _parse_trav(fx["trav"], len(rec))
    for r, (_, (hit, geom, _, tbits), _, any_hit) in enumerate(ref):
        assert (int(rec[r, 1].view(np.int32)) >= 0) == bool(hit), f"ray {r}: hit"
        assert int(rec[r, 0]) == tbits, f"ray {r}: t"
        assert int(occ[r]) == any_hit, f"ray {r}: any hit"
        if hit:
            assert int(rec[r, 1]) == geom, f"ray {r}: geometry"


def shape_differences(got, rec, cls, kinds, words=slice(0, 11)):
    """'' if the per-shape records agree bit for bit (hit / intersect / tmax everywhere, p n uv on hits), else the count of
    differing (shape, ray) pairs per class and per shape kind."""
    g, w = _u32(got), _u32(rec)
    bad = (g[..., :3] != w[..., :3]).any(axis=2)
    hit = rec[..., 1] == 1
    bad |= hit & (g[..., 3:] != w[..., 3:]).any(axis=2)
    if not bad.any():
        return ""
    per_class = {name: int(bad[:, class_of(cls, name)].sum()) for name in CLASSES if bad[:, class_of(cls, name)].any()}
    per_kind = {}
    for s, kind in enumerate(kinds):
        if bad[s].any():
            per_kind[kind] = per_kind.get(kind, 0) + int(bad[s].sum())
    s, r = (int(x) for x in np.argwhere(bad)[0])
    return f"{int(bad.sum())} (shape, ray) pairs differ; per class {per_class}; per shape kind {per_kind}; first: shape {s} ({kinds[s]}) ray {r} " \
           f"({CLASSES[cls[r]]}) {got[s, r].tolist()} vs the reference's {rec[s, r].tolist()}"


@pytest.mark.parametrize("which", list(SHAPE_FILES))
def test_oracle_shape_records_match_reference_on_edge_rays(oracle, which):
    """oracle.shapes, as tests/test_oracle_golden.py::test_shape_records_match_reference, at the ends of the range."""
    fx = load_edge(SHAPE_FILES[which])
    rec = fx["shape_records"]
    kinds = [line.split()[1] for line in fx["pscene"].splitlines() if line.startswith("shape ")]
    got = oracle.shapes(fx["pscene"], fx["rays"], rec.shape[0])
    assert (rec[..., 1] == 1).sum() > 500
    msg = shape_differences(got, rec, fx["cls"], kinds)
    assert not msg, msg
