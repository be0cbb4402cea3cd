#!/usr/bin/env python3
"""usage (GPU box): tools/envsky_speed.py [out.txt]  -- what ImageSky costs: path-kernel time of the open_sun scene of the ImageSky
fixtures (tests/envsky_scenes.py) at 640 x 640, 64 spp, depth 6 under ImageSky(sun) against the same scene under Sky, precompiled
kernels, same binary; and the lights_zoo scene (Sky, no ImageSky) for comparison with the commit before ImageSky
($PINE_GPU_LIB selects that library: run this tool once with each).  Medians of five alternating runs after one uncounted run of
each (as profiles/tile_resolve.txt was taken)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before anything else touches the HIP runtime)

import pine_amd as pa  # noqa: E402
from pine_amd import scenes  # noqa: E402
import envsky_scenes as E  # noqa: E402


def path_ms(sc, spp, depth):
    w, h = sc.camera.film().size
    plan = pa.Plan(sc, spp, depth, specialize=False, timing=True)
    film = torch.zeros((h, w, 4), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plan.launch(film.data_ptr(), s)
    torch.cuda.synchronize()
    plan.launch(film.data_ptr(), s)
    torch.cuda.synchronize()
    st = plan.stats()
    ms, feat = st.trace_ms, st.kernel_features
    plan.close()
    return ms, feat


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    cases = {"lights_zoo 640x640 s64 d6 (Sky)": (scenes.lights_zoo((640, 640)), 64, 6)}
    if hasattr(pa, "ImageSky"):
        image = E._open_sun((640, 640))
        image.set(E.image_sky("sun"))
        sky = E._open_sun((640, 640))
        sky.set(pa.Sky([1.0, 1.0, 1.0]))
        cases["open_sun 640x640 s64 d6, ImageSky(sun)"] = (image, 64, 6)
        cases["open_sun 640x640 s64 d6, Sky"] = (sky, 64, 6)
    runs = {k: [] for k in cases}
    feats = {}
    for rnd in range(6):  # (round 0 is the uncounted one)
        for k, (sc, spp, depth) in cases.items():
            ms, feats[k] = path_ms(sc, spp, depth)
            if rnd:
                runs[k].append(ms)
    print(f"library: {os.environ.get('PINE_GPU_LIB', 'pine_amd/lib/libpine_gpu.so')}", file=out)
    for k, v in runs.items():
        print(f"{k:42s} path kernel median {statistics.median(v):8.3f} ms  runs {' '.join('%.3f' % x for x in v)}  features {feats[k]:#x}", file=out)
    a, b = "open_sun 640x640 s64 d6, ImageSky(sun)", "open_sun 640x640 s64 d6, Sky"
    if a in runs:
        print(f"ImageSky / Sky: {statistics.median(runs[a]) / statistics.median(runs[b]):.3f}", file=out)
    out.flush()


if __name__ == "__main__":
    main()
