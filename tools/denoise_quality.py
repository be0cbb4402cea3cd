#!/usr/bin/env python3
"""CPU: what the denoising filter's defaults and the tolerance of tests/test_denoise.py rest on -> profiles/denoise_quality.txt.

    python tools/denoise_quality.py

1. The sweep behind PINE_GPU_DENOISE_SIGMA_COLOR / _SIGMA_ALBEDO / _EPS_ALBEDO: on the four fixture scenes
   (tests/golden/denoise_*.npz: the real reference's guide images, a 16 spp and a 4096 spp film) the host build of the filter
   with 5 iterations over a grid of sigmas; per cell the ratio mse(denoised, converged) / mse(noisy, converged) over the rgb of
   hit pixels, per scene and as the geometric mean.  The choice: the cell with the smallest geometric mean among those where
   EVERY scene improves.
2. The host build against the float64 restatement of tests/test_denoise.py on the four fixtures with the chosen defaults: the
   largest absolute difference, and what four mutations of the restatement do to it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import denoise_scenes as S  # noqa: E402
import test_denoise as T  # noqa: E402
import pine_amd as pa  # noqa: E402

SIGMA_COLOR = [0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.1, 0.15, 0.25, 0.5, 1.0, 2.0]
SIGMA_ALBEDO = [0.03, 0.1, 0.3]
EPS_ALBEDO = [0.001, 0.01]


def ratio(f, out, dim_only=False):
    """dim_only: over the hit pixels whose converged value stays below 2 in every channel (no lamp in the pixel)."""
    hit = S.hits(f["normal"])
    if dim_only:
        hit = hit & (f["converged"][..., :3].max(axis=2) < 2)
    conv = f["converged"][..., :3].astype(np.float64)[hit]
    before = ((f["noisy"][..., :3].astype(np.float64)[hit] - conv) ** 2).mean()
    return ((out[..., :3].astype(np.float64)[hit] - conv) ** 2).mean() / before


def main():
    fx = {name: S.load(name) for name in S.DENOISE_FILMS}
    lines = ["# tools/denoise_quality.py: the host build of pine_denoise.h on tests/golden/denoise_*.npz (CPU; no timing here)", ""]
    lines += ["## 1. sweep: mse(denoised, converged) / mse(noisy, converged), rgb of hit pixels, iterations = 5, normal_power_log2 = 7",
              "eps_albedo sigma_color sigma_albedo | " + " ".join(f"{n:>15}" for n in fx) + " | geometric mean | every scene improves"]
    best = None
    for eps in EPS_ALBEDO:
        for sc in SIGMA_COLOR:
            for sa in SIGMA_ALBEDO:
                r = [ratio(f, pa.denoise(f["noisy"], f["albedo"], f["normal"], device=-1, sigma_color=sc, sigma_albedo=sa, eps_albedo=eps))
                     for f in fx.values()]
                gm = float(np.exp(np.mean(np.log(r))))
                ok = max(r) < 1
                lines.append(f"{eps:10.3f} {sc:11.2f} {sa:12.2f} | " + " ".join(f"{x:15.6f}" for x in r) + f" | {gm:14.6f} | {'yes' if ok else 'no'}")
                if ok and (best is None or gm < best[0]):
                    best = (gm, eps, sc, sa)
    lines += ["", f"chosen (smallest geometric mean among the cells where every scene improves): eps_albedo = {best[1]}, sigma_color = {best[2]}, "
              f"sigma_albedo = {best[3]} (geometric mean {best[0]:.6f})"]
    d = T.defaults()
    lines += [f"the library's defaults (include/pine_gpu.h): {d}", "",
              "What decides the sweep.  A few pixels of every scene hold a sliver of a lamp that the pixel centre misses: their guides are the",
              "wall's, their converged value is 10 ... 100, and 16 samples either miss the sliver (value < 1) or overshoot it.  Their",
              "squared error is 10^3 times that of all other pixels together, no guide-driven filter can repair them, and any averaging of a",
              "pixel that missed its sliver moves it a little further from the converged value.  Only a small sigma_color leaves them alone,",
              "so the criterion above selects a CAUTIOUS default; a larger sigma_color smooths the rest of the picture much more (below) at",
              "the price of those pixels.  Ratio over the hit pixels whose converged value stays below 2 (no lamp in the pixel):",
              "sigma_color | " + " ".join(f"{n:>15}" for n in fx)]
    for sc in (d["sigma_color"], 0.1, 0.25, 0.5):
        r = [ratio(f, pa.denoise(f["noisy"], f["albedo"], f["normal"], device=-1, sigma_color=sc), True) for f in fx.values()]
        lines.append(f"{sc:11.3f} | " + " ".join(f"{x:15.4f}" for x in r))
    lines.append("")
    lines += ["## 2. host build (fp32) against the float64 restatement of tests/test_denoise.py, the library's defaults",
              "scene | ratio at the defaults | max |host - restatement| | ... with: one tap dropped | one offset mirrored | hit(q) gate skipped | step i instead of 2^i"]
    worst = 0.0
    least_mutation = np.inf
    for name, f in fx.items():
        out = pa.denoise(f["noisy"], f["albedo"], f["normal"], device=-1).astype(np.float64)
        diffs = [np.abs(out - T.restate(f["noisy"], f["albedo"], f["normal"], mutate=m, **d)).max()
                 for m in (None, "drop_tap", "mirror_offset", "no_hit_gate", "linear_step")]
        worst = max(worst, diffs[0])
        least_mutation = min(least_mutation, diffs[1], diffs[2], diffs[4])
        lines.append(f"{name} | {ratio(f, out):.4f} | {diffs[0]:.3e} | " + " | ".join(f"{x:.3e}" for x in diffs[1:]))
    lines += ["", f"largest difference over the four fixtures: {worst:.3e}; tests/test_denoise.py allows 4 x the measured value it records "
              f"({T.RESTATEMENT_MEASURED:.3e} -> {T.RESTATEMENT_TOL:.3e})",
              f"smallest difference a dropped tap, a mirrored offset or a linear step leaves: {least_mutation:.3e} = "
              f"{least_mutation / T.RESTATEMENT_TOL:.0f} x the tolerance",
              "The hit(q) gate: skipping it changes nothing on these films, and cannot in exact arithmetic -- a miss has N(q) = 0, so",
              "w_n = max(0, N(p).N(q)) is 0 and the tap has no weight either way.  The gate matters in fp32 only: a miss's demodulated colour",
              "F / eps_albedo may overflow to inf, and 0 x inf is NaN; with the gate a miss is never read",
              "(tests/test_denoise.py::test_misses_contribute_nothing_whatever_their_colour)."]
    path = os.path.join(ROOT, "profiles", "denoise_quality.txt")
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[-12:]))


if __name__ == "__main__":
    main()
