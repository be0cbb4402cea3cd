#!/usr/bin/env python3
"""usage (GPU box): tools/noise_speed.py [--parent DIR] [out.txt]  -- what the noise nodes cost.

(a) `bench.py` (the headline configuration) and `bench.py --config c4` three times each from DIR, a built checkout of the commit
    before the noise nodes, and three times from this tree, alternating, in one session: the benchmark's value (Msamples/s) of
    each run, the span of the parent's runs, and the verdict -- this commit's median against that span.  Neither kernel has a
    node program in it; the variant name of each bench line is printed: it says which feature set ran.
(b) a scene with node programs but WITHOUT noise -- the room of the texture fixtures (tests/texture_scenes.py) at 640 x 480,
    64 spp, depth 4 -- from both trees, alternating: its kernel now carries the noise body.  Path-kernel medians of five
    launches per run.
(c) the noise room (tests/noise_scenes.py) at 640 x 480, 64 spp, depth 4 against the same room with every noise node replaced
    by a constant: Msamples/s of both, and the difference per camera sample.
(d) the price of one evaluation: pine_gpu_test_material_params on the device over 2^20 queries of Metal(c, Noisef(P, 5)) --
    one fbm of five octaves, 40 corner gradients, per query -- against Metal(c, fract(P)[0]); the difference of the fastest of
    eight calls each, per query.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, SPP, DEPTH = (640, 480), 64, 4


def bench(tree, config):
    env = dict(os.environ, PINE_BENCH_DETAIL=os.devnull)
    env.pop("PINE_GPU_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"] + (["--config", config] if config else []),
                         cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode or not lines:
        raise SystemExit(f"bench.py in {tree} ended with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    r = json.loads(lines[-1])
    return float(r["value"]), r["config"]["name"] + ": " + r["roofline"]["kernel"]


def path_ms(sc, launches=5):
    """Median path-kernel time of `launches` launches after one uncounted one, and the variant that ran."""
    import torch
    import pine_amd as pa
    w, h = sc.camera.film().size
    plan = pa.Plan(sc, SPP, DEPTH, specialize=False, timing=True)
    film = torch.zeros((h, w, 4), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ms = []
    for k in range(launches + 1):
        plan.launch(film.data_ptr(), s)
        torch.cuda.synchronize()
        if k:
            ms.append(plan.stats().trace_ms)
    feat = plan.stats().kernel_features
    plan.close()
    return statistics.median(ms), feat


def worker(tree):
    """(b), run from `tree` with its own library and Python package."""
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch  # noqa: F401  (before anything else touches the HIP runtime)
    import texture_scenes as T
    ms, feat = path_ms(T.room(SIZE))
    print(json.dumps({"ms": ms, "features": feat}))


def span_line(what, runs, out):
    lo, hi, mine = min(runs["parent"]), max(runs["parent"]), statistics.median(runs["this"])
    where = "inside" if lo <= mine <= hi else "ABOVE" if mine > hi else "BELOW"
    print(f"    the parent's three runs span {lo:.3f} .. {hi:.3f}; this commit's median {mine:.3f} is {where} that span ({what})", file=out)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--worker"]:
        return worker(os.path.abspath(args[1]))
    parent = None
    if args[:1] == ["--parent"]:
        parent, args = os.path.abspath(args[1]), args[2:]
    out = open(args[0], "w") if args else sys.stdout
    if parent:
        for config, label in ((None, "headline"), ("c4", "--config c4")):
            runs, names = {"parent": [], "this": []}, {}
            for _ in range(3):
                for who, tree in (("parent", parent), ("this", ROOT)):
                    v, names[who] = bench(tree, config)
                    runs[who].append(v)
            for who in runs:
                print(f"(a) bench.py {label}, {who:6s}: Msamples/s {' '.join('%.2f' % v for v in runs[who])}  median {statistics.median(runs[who]):.2f}  {names[who]}",
                      file=out)
            span_line("Msamples/s, higher is better", runs, out)
            out.flush()
        runs, feats = {"parent": [], "this": []}, {}
        for _ in range(3):
            for who, tree in (("parent", parent), ("this", ROOT)):
                env = dict(os.environ)
                env.pop("PINE_GPU_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree], cwd=tree, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode:
                    raise SystemExit(f"worker in {tree} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                runs[who].append(got["ms"])
                feats[who] = got["features"]
        for who in runs:
            print(f"(b) texture room {SIZE[0]}x{SIZE[1]} s{SPP} d{DEPTH} (node programs, no noise), {who:6s}: path kernel ms {' '.join('%.3f' % v for v in runs[who])}"
                  f"  median {statistics.median(runs[who]):.3f}  features {feats[who]:#x}", file=out)
        span_line("ms, lower is better", runs, out)
        out.flush()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch  # noqa: F401  (before anything else touches the HIP runtime)
    import numpy as np
    import noise_scenes as X
    import pine_amd as pa
    from pine_amd import _lib
    cases = {"noise": X.room(SIZE), "every noise node replaced by a constant": X.room(SIZE, flat=True)}
    ms, feats = {k: [] for k in cases}, {}
    # (with constants for its noise nodes the room has no node program left and would run a smaller variant: it is pinned to
    # the variant the noise room selects, so that the difference is the noise alone)
    _, noise_features = path_ms(cases["noise"], 1)
    n = _lib.lib.pine_gpu_test_kernel_variants(0, None, None, None, 0)
    features = np.zeros(n, np.uint32)
    _lib.lib.pine_gpu_test_kernel_variants(0, features.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, n)
    pin = "queue:%d" % [int(f) for f in features].index(noise_features)
    for _ in range(3):
        for k, sc in cases.items():
            if k != "noise":
                os.environ["PINE_GPU_TEST_VARIANT"] = pin
            try:
                t, feats[k] = path_ms(sc)
            finally:
                os.environ.pop("PINE_GPU_TEST_VARIANT", None)
            ms[k].append(t)
    samples = SIZE[0] * SIZE[1] * SPP
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"(c) noise room {SIZE[0]}x{SIZE[1]} s{SPP} d{DEPTH}, {k:40s} path kernel ms {' '.join('%.3f' % x for x in v)}  median {med[k]:.3f}"
              f"  = {samples / med[k] / 1e3:.1f} Msamples/s  features {feats[k]:#x}", file=out)
    a, b = med["noise"], med["every noise node replaced by a constant"]
    print(f"(c) noise / constant: {a / b:.3f}; the noise costs {(a - b) * 1e6 / samples:.2f} ns per camera sample (a path of up to {DEPTH} vertices)", file=out)
    out.flush()
    n = 1 << 20
    q = (np.random.default_rng(7).random((n, 8), dtype=np.float32) * 6 - 3).astype(np.float32)
    rec = np.zeros((1, n, 10), np.float32)
    took = {}
    for name, rough in (("Noisef(P, 5)", pa.Noisef(pa.Position(), 5)), ("fract(P)[0]", pa.node_fract(pa.Position())[0])):
        sc = pa.Scene()
        sc.add("m", pa.Metal([0.5, 0.5, 0.5], rough))
        t = []
        for k in range(9):
            t0 = time.perf_counter()
            _lib.check(_lib.lib.pine_gpu_test_material_params(sc._h, 0, q.ctypes.data_as(_lib.c_f_p), n, rec.ctypes.data_as(_lib.c_f_p)), "material_params")
            if k:
                t.append((time.perf_counter() - t0) * 1e3)
        took[name] = min(t)  # (the copies' jitter is larger than the kernel: the fastest of eight)
        print(f"(d) material_params hook, 2^20 queries, roughness {name:14s}: {' '.join('%.2f' % x for x in t)} ms (upload, kernel, download)", file=out)
    d = took["Noisef(P, 5)"] - took["fract(P)[0]"]
    print(f"(d) one fbm of 5 octaves (40 corner gradients): {d * 1e6 / n:.3f} ns per query of a full machine (fastest runs' difference: {d:.2f} ms per 2^20)", file=out)
    out.flush()


if __name__ == "__main__":
    main()
