#!/usr/bin/env python3
"""Generate tests/golden/ao_*.npz + ao_films.json from the REAL reference's AOIntegrator(BVH(), sampler).

Runs only where the reference's sources are: tools/ref_ao_driver.cpp is compiled in place against them, together with the
reference's impl/integrator/ao.cpp read from where it lies, and linked with oracle/_ref/libpine_ref.a (make -C oracle ref)
-- the compile line of build()'s adapter_roundtrip.  The binary goes to a scratch directory; nothing of the reference is
copied into this tree.  No test calls this tool: the tests read what it wrote.

    python tools/make_golden_ao.py [name ...]

Per film: the film (H, W, 4), the 25 constants (radius, directions[8]), the integrator's sample count, the .pscene text.
Asserted here, so that no test can pass on an all-black or all-white film: at least 10 % of every film's pixels lie strictly
between 0 and 1; zoo_48_s32 and xshapes_40_s16 have at least 1 % exact misses (0, 0, 0, 1); every value is (k / 8) / spp for an
integer k (the rounded quotient where spp is no power of two).
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
from ao_scenes import AO_FILMS, ao_scene  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
OUT = os.path.join(ROOT, "tests", "golden")
NEED_MISSES = ("zoo_48_s32", "xshapes_40_s16")


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_ao_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_ao_driver.cpp"), os.path.join(REF_SRC, "pine", "impl", "integrator", "ao.cpp"),
                           "-o", exe, ARCHIVE, "-pthread", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def main(names):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    listing = {}
    path = os.path.join(OUT, "ao_films.json")
    if os.path.exists(path):
        listing = json.load(open(path))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in names or AO_FILMS:
            kind, spp = AO_FILMS[name]
            scene = ao_scene(name)
            w, h = scene.camera.film().size
            ps = scene.describe()
            sp, fp, cp = (os.path.join(tmp, x) for x in ("s.pscene", "s.film", "s.consts"))
            open(sp, "w").write(ps)
            subprocess.check_call([exe, sp, str(spp), kind, fp, cp])
            film = np.fromfile(fp, dtype=np.float32).reshape(h, w, 4)
            consts = np.fromfile(cp, dtype=np.float32)
            ao_spp = int(consts[25:26].view(np.int32)[0])
            v = film[..., 0]
            assert np.array_equal(film[..., 0], film[..., 1]) and np.array_equal(film[..., 0], film[..., 2]) and (film[..., 3] == 1).all()
            grey = float(((v > 0) & (v < 1)).mean())
            miss = float((v == 0).mean())
            # every value is k eighths over spp, k an integer: (k * 0.125f) / float(spp) as the reference rounds it (for a count
            # that is no power of two -- SobolSampler(24) -> 3 -- the quotient is rounded, so "value * 8 * spp is an integer" is
            # asked of k, not of the rounded quotient)
            k = np.round(v.astype(np.float64) * 8 * ao_spp)
            assert np.array_equal((k * 0.125).astype(np.float32) / np.float32(ao_spp), v), f"{name}: a film value is not k / 8 / spp"
            assert k.min() >= 0 and k.max() <= 8 * ao_spp
            assert grey >= 0.10, f"{name}: only {grey:.3f} of the pixels lie strictly between 0 and 1"
            if name in NEED_MISSES:
                assert miss >= 0.01, f"{name}: only {miss:.4f} of the pixels are exact zeros"
            np.savez_compressed(os.path.join(OUT, f"ao_{name}.npz"), film=film, constants=consts[:25].copy(), spp=np.int32(ao_spp),
                                pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
            listing[name] = {"sampler": kind, "sampler_spp": spp, "ao_spp": ao_spp, "size": [w, h], "between_0_and_1": round(grey, 4),
                             "exact_zero": round(miss, 4), "mean": float(v.mean(dtype=np.float64))}
            print(name, listing[name], os.path.getsize(os.path.join(OUT, f"ao_{name}.npz")), "bytes", flush=True)
    json.dump(listing, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
