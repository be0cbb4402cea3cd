#!/usr/bin/env python3
"""Generate tests/golden/*_edge.npz: the REAL reference's answers to the edge rays of tests/edge_rays.py (tmin > 0, scaled and
axis-parallel directions, origins on a surface, spans that end exactly at a hit ...).

Runs only where the reference's sources and oracle/_ref are (make -C oracle ref embree); the accel driver is the one of
tools/make_golden_accel.py, built into a scratch directory.  No test calls this tool; it writes under tests/golden/ only and
nothing of the reference enters the tree.

    python tools/make_golden_edge.py

  shapes_zoo_edge.npz, shapes_xzoo_edge.npz     `pine_ref shapes`: every non-mesh geometry against every edge ray (hit, intersect,
                                                tmax, p, n, uv).  The first pass of a base ray is its answer from ONE target shape
                                                it hits, the shapes taken in turn.
  accel_<scene>_<bvh|embree>_edge.npz           Accel::intersect / Accel::hit under both orders: rays, cls, redraw, the 12-word
                                                records, the occlusion bytes, the first-pass records (BVH order, tmin = 0); for
                                                cbox and zoo the bvh file also holds `trav`, the stream of `pine_ref bvh` on the
                                                same rays.
A file that would pass 100 KB is split by ray into <stem>_a.npz, <stem>_b.npz (tests/edge_rays.py load_edge joins them).

Asserted here, and written into each file as `info` (JSON), so that no test passes on a fixture that says nothing:
  * every class has at least 10 % hits and 5 % misses in the closest-hit query (on_surface, inside: hits only);
  * per shape kind, tmin_at_hit + tmax_at_hit hold at least 5 (shape, ray) pairs whose hit and intersect flags differ; a kind
    that never differs is named in NEVER_DIFFER with the reason read from the reference's code;
  * at least 10 % of the tmin_random rays that hit at tmin = 0 report another t or primitive now;
  * the geometry word of at least 90 % of the scaled_dir hits is the unscaled ray's; the others are counted.  Hits on a Sphere
    or an OBB, scaled or unscaled, are counted apart: the reference answers those in a mix of units (see accel_files);
  * a ray on which the two orders report the same t bits on different primitives is replaced by its redraw (the class drawn
    anew, edge_rays_full(redraw=k)); at most 2 % of a class.

What was chosen so that these hold (tests/edge_rays.py): tmin_random takes three quarters of its base rays from the camera rays
(the open scenes leave too few hits otherwise).  The seeds of the two shape files (EDGE_SEEDS) are ones whose tmin_random class
holds a ray with tmin between a Sphere's two roots -- about one seed in four does --, so that the class reaches the second-root
switch; the seed of cbox is one where the scaled_dir share holds over all hits too (OBB hits included it is 80 ... 93 % over
twelve seeds).  The reference's own hit() and intersect() agree at the ends for more kinds than one would guess: NEVER_DIFFER.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from accel_scenes import accel_scene  # noqa: E402
from edge_rays import (ACCEL_SCENES, CLASSES, EDGE_SEEDS, NUM_BASE, SHAPE_FILES, TRAV_SCENES, base_rays, class_of, edge_rays_full,  # noqa: E402
                       shape_scene)
from make_golden_accel import ARCHIVE, EMB_LIBS, REF_SRC, build_driver  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "pine_ref")
OUT = os.path.join(ROOT, "tests", "golden")
LIMIT = 100 * 1024
HITS_ONLY = ("on_surface", "inside")
SCALE_LOOSE = ("sphere", "obb")
# shape kinds whose hit() and intersect() never disagree, and why (the reference's code)
NEVER_DIFFER = {
    "cylinder": "Cylinder::hit and Cylinder::intersect are the same statements up to the result (geometry.cpp:480-482, 504-506)",
    "line": "Line::hit and Line::intersect clamp the same z into [tmin + thickness, tmax] and compare the same distance (geometry.cpp:190-194, 206-210)",
    "cone": "Cone::hit and Cone::intersect both call intersect_quadratic with the ray's tmin and tmax (geometry.cpp:422, 435); they differ "
            "in the apex-side test only (<= 0 against < 0), which no end of the span decides",
    "rect": "Rect::hit and Rect::intersect both refuse t <= tmin and t >= tmax (geometry.cpp:284, 296)",
    "box": "AABB::hit and AABB::intersect(Ray&) run the same slab loop with the same comparisons (bbox.cpp:86-111, 113-139); intersect only "
           "picks tmin or tmax afterwards",
    "obb": "OBB::hit and OBB::intersect transform the ray alike and call those two AABB functions (bbox.cpp:141-171)",
}


def shape_kinds(pscene):
    return [line.split()[1] for line in pscene.splitlines() if line.startswith("shape ") and not line.split()[1].startswith("mesh")]


def save(stem, per_ray, whole, n):
    """One file, or as many parts (split by ray) as keep each under the limit; stale files of the other layout are removed."""
    for c in ("", "_a", "_b", "_c", "_d", "_e", "_f"):
        p = os.path.join(OUT, stem + c + ".npz")
        if os.path.exists(p):
            os.remove(p)
    for parts in range(1, 7):
        cuts = [n * i // parts for i in range(parts + 1)]
        paths = []
        for i in range(parts):
            p = os.path.join(OUT, stem + ("" if parts == 1 else "_" + "abcdef"[i]) + ".npz")
            np.savez_compressed(p, **{k: np.take(v, range(cuts[i], cuts[i + 1]), axis=ax) for k, (v, ax) in per_ray.items()}, **whole)
            paths.append(p)
        if all(os.path.getsize(p) < LIMIT for p in paths):
            return [os.path.getsize(p) for p in paths]
        for p in paths:
            os.remove(p)
    raise AssertionError(stem + ": does not fit")


def class_counts(cls, hit, name_of):
    out = {}
    for ci, name in enumerate(CLASSES):
        m = cls == ci
        if not m.any():
            continue
        h, k = int(hit[m].sum()), int(m.sum())
        out[name] = {"rays": k, "hits": h}
        assert h >= 0.10 * k, f"{name_of} {name}: {h} of {k} rays hit"
        assert name in HITS_ONLY or k - h >= 0.05 * k, f"{name_of} {name}: {k - h} of {k} rays miss"
    return out


def shape_files(tmp):
    sp, rp, op = (os.path.join(tmp, x) for x in ("z.pscene", "rays.bin", "shapes.bin"))

    def run(rays):
        rays.tofile(rp)
        subprocess.run([REF, "shapes", sp, rp, op], check=True, capture_output=True)
        return np.fromfile(op, dtype=np.float32).reshape(-1, len(rays), 11)

    for which, stem in SHAPE_FILES.items():
        sc = shape_scene(which)
        ps = sc.describe()
        open(sp, "w").write(ps)
        kinds = shape_kinds(ps)
        seed = EDGE_SEEDS[which]
        base = base_rays(sc, seed)
        first = run(base)
        S = first.shape[0]
        assert S == len(kinds)
        fp = np.zeros((NUM_BASE, 12), np.uint32)
        fp[:, 0], fp[:, 1:4] = base[:, 7].view(np.uint32), np.uint32(0xFFFFFFFF)  # (a miss, until a shape is hit)
        for i in range(NUM_BASE):  # the target shape: the first that the ray hits, starting at another shape for every ray
            for s in [(i + j) % S for j in range(S)]:
                if first[s, i, 1] == 1:
                    fp[i, 0] = first[s, i, 2:3].view(np.uint32)[0]
                    fp[i, 1], fp[i, 2], fp[i, 3] = s, 0xFFFFFFFF, 0
                    fp[i, 4:12] = first[s, i, 3:11].view(np.uint32)
                    break
        rays, cls, _ = edge_rays_full(sc, seed, fp)
        rec = run(rays)
        at = class_of(cls, "tmin_at_hit") | class_of(cls, "tmax_at_hit")
        differ = {}
        for s, kind in enumerate(kinds):
            differ[kind] = differ.get(kind, 0) + int((rec[s, at, 0] != rec[s, at, 1]).sum())
        print(which, "hit != intersect at the ends:", differ, flush=True)
        for kind, k in differ.items():
            if kind in NEVER_DIFFER:
                assert k == 0, f"{which}: {kind} differs after all ({k})"
            else:
                assert k >= 5, f"{which}: only {k} (shape, ray) pairs of {kind} have hit != intersect at the ends"
        any_hit = (rec[..., 1] == 1).any(axis=0)
        info = {"classes": class_counts(cls, any_hit, which), "hit_differs_from_intersect": differ,
                "never_differ": {k: v for k, v in NEVER_DIFFER.items() if k in differ}}
        sizes = save(stem, {"rays": (rays, 0), "cls": (cls, 0), "redraw": (np.zeros(len(rays), np.uint8), 0), "shape_records": (rec, 1)},
                     {"pscene": np.frombuffer(ps.encode(), dtype=np.uint8), "first_pass": fp, "info": np.frombuffer(json.dumps(info).encode(), dtype=np.uint8)},
                     len(rays))
        print(stem, sizes, json.dumps(info), flush=True)


def accel_files(tmp, exes):
    sp, rp, op, bp, tp, vp = (os.path.join(tmp, x) for x in ("s.pscene", "r.bin", "o.records", "o.occluded", "tree.bin", "trav.bin"))

    def run(order, rays):
        rays.tofile(rp)
        subprocess.run([exes[order], order, sp, rp, op, bp], capture_output=True, text=True, check=True)
        return np.fromfile(op, dtype=np.uint32).reshape(len(rays), 12), np.fromfile(bp, dtype=np.uint8)

    for name in ACCEL_SCENES:
        sc = accel_scene(name)
        ps = sc.describe()
        open(sp, "w").write(ps)
        seed = EDGE_SEEDS[name]
        kinds = np.array([line.split()[1] for line in ps.splitlines() if line.startswith("shape ")])
        fp, _ = run("bvh", base_rays(sc, seed))
        rays, cls, _ = edge_rays_full(sc, seed, fp)
        redraw = np.zeros(len(rays), np.uint8)
        for k in range(1, 9):
            got = {order: run(order, rays) for order in ("bvh", "embree")}
            b, e = got["bvh"][0], got["embree"][0]
            both = (b[:, 1].view(np.int32) >= 0) & (e[:, 1].view(np.int32) >= 0)
            ties = both & (b[:, 0] == e[:, 0]) & ((b[:, 1] != e[:, 1]) | (b[:, 2] != e[:, 2]))
            if not ties.any():
                break
            rays[ties] = edge_rays_full(sc, seed, fp, redraw=k)[0][ties]
            redraw[ties] = k
        else:
            raise AssertionError(f"{name}: ties after 8 redraws")
        redraws = {CLASSES[ci]: int((redraw[cls == ci] > 0).sum()) for ci in np.unique(cls)}
        for cname, k in redraws.items():
            assert k <= 0.02 * (cls == CLASSES.index(cname)).sum(), f"{name} {cname}: {k} redraws"
        # the control runs: tmin_random at tmin = 0, scaled_dir before scaling (redrawn rays: their own redraw's)
        control = rays.copy()
        control[class_of(cls, "tmin_random"), 6] = 0.0
        sd = class_of(cls, "scaled_dir")
        for k in np.unique(redraw[sd]):
            m = sd & (redraw == k)
            control[m] = edge_rays_full(sc, seed, fp, redraw=int(k), unscaled=True)[0][m]
        trav = None
        if name in TRAV_SCENES:
            rays.tofile(rp)
            subprocess.run([REF, "bvh", sp, rp, tp, vp], check=True, capture_output=True)
            trav = np.fromfile(vp, dtype=np.uint32)
        for order in ("bvh", "embree"):
            rec, occ = got[order]
            crec, _ = run(order, control)
            hit = rec[:, 1].view(np.int32) >= 0
            assert set(np.unique(occ)) <= {0, 1}
            info = {"classes": class_counts(cls, hit, f"{name} {order}"), "redraws": redraws}
            m = class_of(cls, "tmin_random") & (crec[:, 1].view(np.int32) >= 0)
            changed = int((rec[m, :3] != crec[m, :3]).any(axis=1).sum())
            assert changed >= 0.10 * m.sum(), f"{name} {order}: tmin changes {changed} of {int(m.sum())} answers"
            info["tmin_random"] = {"hit_at_tmin_0": int(m.sum()), "other_t_or_primitive": changed}
            # scaled_dir.  Two kinds answer a scaled direction in a mix of units and not geometrically -- Sphere::compute_t has no
            # `a` term (geometry.cpp:73-83), OBB::intersect normalises the direction and keeps the ray's tmin / tmax
            # (bbox.cpp:141-171) --, so a scene with a sphere gives a quarter of the rays scaled by 3 or 1e3 a hit on it wherever
            # they point.  The 90 % are asked of the hits that name neither kind, scaled or unscaled; the share over all hits is
            # written next to it.  (Every ray stays in the fixture and in every test: the reference decides.)
            m = sd & hit
            chit = crec[:, 1].view(np.int32) >= 0
            loose = np.isin(kinds[np.where(hit, rec[:, 1], 0)], SCALE_LOOSE) & hit | np.isin(kinds[np.where(chit, crec[:, 1], 0)], SCALE_LOOSE) & chit
            same_all = int((rec[m, 1] == crec[m, 1]).sum())
            m = m & ~loose
            same = int((rec[m, 1] == crec[m, 1]).sum())
            assert m.sum() >= 10 and same >= 0.90 * m.sum(), f"{name} {order}: scaled_dir: {same} of {int(m.sum())} hits keep their geometry"
            info["scaled_dir"] = {"hits": int((sd & hit).sum()), "same_geometry_as_unscaled": same_all, "hits_off_sphere_and_obb": int(m.sum()),
                                  "same_geometry_off_sphere_and_obb": same, "other_off_sphere_and_obb": int(m.sum()) - same,
                                  "unscaled_hits_now_missed": int((sd & ~hit & chit).sum())}
            whole = {"pscene": np.frombuffer(ps.encode(), dtype=np.uint8), "first_pass": fp, "info": np.frombuffer(json.dumps(info).encode(), dtype=np.uint8)}
            if order == "bvh" and trav is not None:
                whole["trav"] = trav
            sizes = save(f"accel_{name}_{order}_edge", {"rays": (rays, 0), "cls": (cls, 0), "redraw": (redraw, 0), "records": (rec, 0), "occluded": (occ, 0)},
                         whole, len(rays))
            print(f"accel_{name}_{order}_edge", sizes, json.dumps(info), flush=True)


def main():
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE) or not os.path.exists(REF):
        sys.exit("the reference's sources and oracle/_ref (make -C oracle ref) are needed")
    if not os.path.exists(EMB_LIBS[0]):
        sys.exit("oracle/_ref/embree_build is missing: make -C oracle embree")
    with tempfile.TemporaryDirectory() as tmp:
        shape_files(tmp)
        accel_files(tmp, {"bvh": build_driver(tmp, False), "embree": build_driver(tmp, True)})


if __name__ == "__main__":
    main()
