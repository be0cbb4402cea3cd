#!/usr/bin/env python3
"""Generate tests/golden/accel_<scene>_<bvh|embree>.npz from the REAL reference's Accel::intersect / Accel::hit.

Runs only where the reference's sources are: tools/ref_accel_driver.cpp is compiled in place against them and linked with
oracle/_ref/libpine_ref.a (make -C oracle ref) -- twice: as it is for Accel(BVH()), and with -DPINE_REF_WITH_EMBREE against the
Embree of oracle/_ref/embree_build (make -C oracle embree) for Accel(EmbreeAccel()).  The binaries go to a scratch directory;
nothing of the reference is copied into this tree.  No test calls this tool: the tests read what it wrote.

    python tools/make_golden_accel.py [--no-embree] [scene ...]

Per file: the .pscene text, 1000 rays (tools/make_golden.py bvh_rays, the seeds of tests/accel_scenes.py), the 12-word records
(include/pine_gpu.h) and the occlusion bytes; where tests/golden/bvh_<scene>.npz describes the same scene, also the driver's
answers to that fixture's first rays.  Asserted here, so that no test can pass on a fixture that says nothing:
  * at least 10 % of the rays hit (the open scenes -- shapes_zoo -- let most rays between random points pass) and at least 5 % miss; in the mesh scenes at least 5 % of the rays hit a mesh;
  * under BVH() the driver's nearest-triangle rule names the traversal's own triangle for every mesh hit (it supplies the
    triangle word under EmbreeAccel());
  * the two orders' records are compared: a ray whose t bits agree but whose triangle differs is a tie that EmbreeAccel's own
    hierarchy decides -- none may be in a fixture: change the scene's seed.
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
from accel_scenes import CROSS_RAYS, NUM_RAYS, SAME_AS_BVH_FIXTURE, SEEDS, accel_rays, accel_scene  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
ARCHIVE = os.path.join(REF_OUT, "libpine_ref.a")
EMB = os.path.join(REF_OUT, "embree_build")
EMB_LIBS = [os.path.join(EMB, p) for p in ("kernels/libembree4.a", "kernels/libembree_avx2.a", "kernels/libembree_avx.a", "kernels/libembree_sse42.a",
                                           "common/lexers/liblexers.a", "common/simd/libsimd.a", "common/tasking/libtasking.a", "common/math/libmath.a",
                                           "common/sys/libsys.a")]
OUT = os.path.join(ROOT, "tests", "golden")
MESH_SCENES = ("sss_mesh", "mesh_attrs")


def build_driver(tmp, embree):
    """The compile lines of oracle/Makefile's pine_ref / pine_ref_embree, with this repository's driver."""
    exe = os.path.join(tmp, "ref_accel_driver" + ("_embree" if embree else ""))
    flags = ["g++", "-std=c++20", "-O2", "-DNDEBUG", "-w", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib", "-I" + REF_SRC + "/contrib/embree/include"]
    src = os.path.join(ROOT, "tools", "ref_accel_driver.cpp")
    if embree:
        subprocess.check_call(flags + ["-DPINE_REF_WITH_EMBREE", src, "-o", exe, ARCHIVE, "-Wl,--start-group", *EMB_LIBS, "-Wl,--end-group", "-pthread", "-ldl",
                                       "-Wl,--unresolved-symbols=ignore-all"])
    else:
        subprocess.check_call(flags + [src, "-o", exe, ARCHIVE, "-pthread", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def main(argv):
    with_embree = "--no-embree" not in argv
    names = [a for a in argv if not a.startswith("--")] or list(SEEDS)
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    if with_embree and not os.path.exists(EMB_LIBS[0]):
        sys.exit("oracle/_ref/embree_build is missing: make -C oracle embree (or --no-embree)")
    with tempfile.TemporaryDirectory() as tmp:
        exes = {"bvh": build_driver(tmp, False)}
        if with_embree:
            exes["embree"] = build_driver(tmp, True)
        for name in names:
            scene = accel_scene(name)
            ps = scene.describe()
            rays = accel_rays(scene, name)
            assert rays.shape == (NUM_RAYS, 8) and rays.dtype == np.float32
            sp, rp, op, bp = (os.path.join(tmp, x) for x in ("s.pscene", "r.bin", "o.records", "o.occluded"))
            open(sp, "w").write(ps)
            rays.tofile(rp)
            got = {}
            for order, exe in exes.items():
                info = json.loads(subprocess.run([exe, order, sp, rp, op, bp], capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1])
                rec = np.fromfile(op, dtype=np.uint32).reshape(NUM_RAYS, 12)
                occ = np.fromfile(bp, dtype=np.uint8)
                assert occ.shape == (NUM_RAYS,) and set(np.unique(occ)) <= {0, 1}
                hit = rec[:, 1].view(np.int32) >= 0
                assert 0.10 * NUM_RAYS <= hit.sum() <= 0.95 * NUM_RAYS, f"{name} {order}: {hit.sum()} of {NUM_RAYS} rays hit"
                assert (rec[~hit, 0] == rays[~hit, 7].view(np.uint32)).all() and (rec[~hit, 4:] == 0).all(), f"{name} {order}: a miss's record"
                assert (rec[hit, 0].view(np.float32) < rays[hit, 7]).all()
                assert (occ[hit] == 1).all(), f"{name} {order}: a closest hit that the any-hit query does not see"
                if name in MESH_SCENES:
                    assert info["mesh_hits"] >= 0.05 * NUM_RAYS, f"{name} {order}: only {info['mesh_hits']} rays hit a mesh"
                if order == "bvh":
                    assert info["nearest_differs"] == 0, f"{name}: the nearest-triangle rule names another triangle for {info['nearest_differs']} rays"
                got[order] = rec
                extra = {}
                if order == "bvh" and name in SAME_AS_BVH_FIXTURE:
                    # the same driver on the first rays of tests/golden/bvh_<scene>.npz, whose answers `pine_ref bvh` wrote: the
                    # CPU suite compares the two runs of the reference (tests/test_accel.py)
                    z = np.load(os.path.join(OUT, f"bvh_{SAME_AS_BVH_FIXTURE[name]}.npz"))
                    assert str(z["pscene"]) == ps, f"{name}: bvh_{SAME_AS_BVH_FIXTURE[name]}.npz describes another scene"
                    np.ascontiguousarray(z["rays"][:CROSS_RAYS]).tofile(rp)
                    subprocess.run([exe, order, sp, rp, op, bp], capture_output=True, text=True, check=True)
                    extra = {"cross_records": np.fromfile(op, dtype=np.uint32).reshape(CROSS_RAYS, 12), "cross_occluded": np.fromfile(bp, dtype=np.uint8)}
                    rays.tofile(rp)
                path = os.path.join(OUT, f"accel_{name}_{order}.npz")
                np.savez_compressed(path, pscene=np.frombuffer(ps.encode(), dtype=np.uint8), rays=rays, records=rec, occluded=occ, **extra)
                size = os.path.getsize(path)
                assert size < 100 * 1024, f"{path}: {size} bytes"
                print(name, order, info, size, "bytes", flush=True)
            if len(got) == 2:
                b, e = got["bvh"], got["embree"]
                both = (b[:, 1].view(np.int32) >= 0) & (e[:, 1].view(np.int32) >= 0)
                ties = both & (b[:, 0] == e[:, 0]) & ((b[:, 1] != e[:, 1]) | (b[:, 2] != e[:, 2]))
                assert not ties.any(), f"{name}: rays {np.nonzero(ties)[0].tolist()} report the same t on different primitives: change the seed"
                print(name, "orders differ in", int((b != e).any(axis=1).sum()), "records; in the hit primitive of", int((b[:, 1:3] != e[:, 1:3]).any(axis=1).sum()),
                      flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
