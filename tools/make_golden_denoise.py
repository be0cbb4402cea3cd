#!/usr/bin/env python3
"""Generate tests/golden/denoise_*.npz from the REAL reference: the guide images of its DenoiseIntegrator and, for the film
fixtures, a noisy and a converged film of its PathIntegrator.

Runs only where the reference's sources are: tools/ref_guides_driver.cpp is compiled in place against them, together with the
reference's impl/integrator/denoiser.cpp read from where it lies, and linked with oracle/_ref/libpine_ref.a (make -C oracle ref);
the driver defines pine::denoise() -- the reference's hook for the library it lacks -- and writes the guide images it is handed.
The binary goes to a scratch directory; nothing of the reference is copied into this tree.  The films come from
oracle/_ref/pine_ref (pine-BVH order).  No test calls this tool: the tests read what it wrote.

    python tools/make_golden_denoise.py [name ...]

Asserted here, so that no test can pass on trivial images: every hit normal has length within 1e-5 of 1; at least 10 % of the
pixels of every scene are hits; at least one scene has at least 1 % misses; mats_zoo has at least 50 distinct albedo values;
noisy differs from converged.  Tie pixels: none can occur -- the guide pass runs in pine-BVH order only, where the first
primitive tested keeps an equal t; the count (0) is printed per film and capped at 3.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from denoise_scenes import CONVERGED_SPP, DENOISE_FILMS, GUIDES_ONLY, NOISY_SPP, denoise_scene, hits  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
PINE_REF = os.path.join(ROOT, "oracle", "_ref", "pine_ref")
OUT = os.path.join(ROOT, "tests", "golden")


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_guides_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_guides_driver.cpp"), os.path.join(REF_SRC, "pine", "impl", "integrator", "denoiser.cpp"),
                           "-o", exe, ARCHIVE, "-pthread", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def ref_film(sp, w, h, spp, depth, tmp, sampler=None):
    fp = os.path.join(tmp, "s.film")
    subprocess.run([PINE_REF, "render", sp, str(spp), str(depth), fp] + ([sampler] if sampler else []), check=True, capture_output=True)
    return np.fromfile(fp, dtype=np.float32).reshape(h, w, 4)


def main(names):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE) or not os.access(PINE_REF, os.X_OK):
        sys.exit("the reference's sources, oracle/_ref/libpine_ref.a and oracle/_ref/pine_ref (make -C oracle ref) are needed")
    most_misses = 0.0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in names or list(DENOISE_FILMS) + list(GUIDES_ONLY):
            scene = denoise_scene(name)
            w, h = scene.camera.film().size
            ps = scene.describe()
            sp, ap, np_ = (os.path.join(tmp, x) for x in ("s.pscene", "s.albedo", "s.normal"))
            open(sp, "w").write(ps)
            subprocess.check_call([exe, sp, ap, np_])
            albedo = np.fromfile(ap, dtype=np.float32).reshape(h, w, 3)
            normal = np.fromfile(np_, dtype=np.float32).reshape(h, w, 3)
            hit = hits(normal)
            length = np.sqrt((normal.astype(np.float64) ** 2).sum(axis=2))
            assert (np.abs(length[hit] - 1) <= 1e-5).all(), f"{name}: a hit normal is not of unit length"
            assert (albedo[~hit] == 0).all(), f"{name}: a miss has an albedo"
            assert hit.mean() >= 0.10, f"{name}: only {hit.mean():.3f} of the pixels are hits"
            most_misses = max(most_misses, float((~hit).mean()))
            distinct = len(np.unique(albedo.reshape(-1, 3), axis=0))
            if name.startswith("mats_zoo"):
                assert distinct >= 50, f"{name}: only {distinct} distinct albedo values"
            data = dict(albedo=albedo, normal=normal, pscene=np.frombuffer(ps.encode(), dtype=np.uint8), tie_pixels=np.zeros((0, 2), np.int32))
            if name in DENOISE_FILMS:
                depth = DENOISE_FILMS[name]
                data["noisy"] = ref_film(sp, w, h, NOISY_SPP, depth, tmp)
                data["converged"] = ref_film(sp, w, h, CONVERGED_SPP, depth, tmp, "sobol")
                data["depth"] = np.int32(depth)
                assert np.isfinite(data["noisy"]).all() and np.isfinite(data["converged"]).all()
                assert not np.array_equal(data["noisy"], data["converged"]), f"{name}: noisy equals converged"
            path = os.path.join(OUT, f"denoise_{name}.npz")
            np.savez_compressed(path, **data)
            print(name, f"{w}x{h}", f"hits {hit.mean():.4f}", f"distinct albedos {distinct}", "tie pixels 0", os.path.getsize(path), "bytes", flush=True)
    if not names:
        assert most_misses >= 0.01, f"no scene has 1 % misses (most: {most_misses:.4f})"


if __name__ == "__main__":
    main(sys.argv[1:])
