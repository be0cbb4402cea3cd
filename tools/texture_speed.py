#!/usr/bin/env python3
"""usage (GPU box): tools/texture_speed.py [--parent DIR] [out.txt]  -- what image texture nodes cost.

(a) `bench.py --config c4` (classic + 10 000 cones; the bench line names its kernel, path_queue_kernel<8284>, whose mask has no
    F_NODES bit: like every BASELINE configuration it runs no node-program code) three times from DIR, a
    built checkout of the commit before the texture nodes, and three times from this tree, alternating, in one session: the
    benchmark's value (Msamples/s) of each run and the verdict -- this commit's median against the parent's minimum.  The
    variant name of each bench line is printed: it says which feature set ran.
(b) the room scene of the texture fixtures (tests/texture_scenes.py) at 640 x 480, 64 spp, depth 4: path-kernel time textured,
    with the 8-bit images as stored (one word per texel, linearised on lookup); with them uploaded as floats; and with every
    texture replaced by its mean colour.  Medians of five alternating runs after one uncounted run of each.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_c4(tree):
    env = dict(os.environ, PINE_BENCH_DETAIL=os.devnull)
    env.pop("PINE_GPU_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--config", "c4"],
                         cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode or not lines:
        raise SystemExit(f"bench.py in {tree} ended with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    r = json.loads(lines[-1])
    return float(r["value"]), r["config"]["name"] + ": " + r["roofline"]["kernel"]


def path_ms(sc, spp, depth):
    import torch
    import pine_amd as pa
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
    args = sys.argv[1:]
    parent = None
    if args[:1] == ["--parent"]:
        parent, args = os.path.abspath(args[1]), args[2:]
    out = open(args[0], "w") if args else sys.stdout
    if parent:
        runs = {"parent": [], "this": []}
        names = {}
        for _ in range(3):
            for who, tree in (("parent", parent), ("this", ROOT)):
                v, names[who] = bench_c4(tree)
                runs[who].append(v)
        for who in runs:
            print(f"(a) bench.py --config c4, {who:6s}: Msamples/s {' '.join('%.2f' % v for v in runs[who])}  median {statistics.median(runs[who]):.2f}  {names[who]}",
                  file=out)
        lo, hi, mine = min(runs["parent"]), max(runs["parent"]), statistics.median(runs["this"])
        print(f"(a) the parent's three runs span {lo:.2f} .. {hi:.2f}; this commit's median {mine:.2f} is "
              f"{'NOT below' if mine >= lo else 'BELOW'} the parent's minimum", file=out)
        out.flush()
    import torch  # noqa: F401  (before anything else touches the HIP runtime)
    import texture_scenes as X
    size = (640, 480)
    cases = {"textured, 8-bit images as stored": X.room(size), "textured, 8-bit images uploaded as floats": X.room(size, as_float=True),
             "every texture replaced by its mean colour": X.room(size, flat=True)}
    ms, feats = {k: [] for k in cases}, {}
    for rnd in range(6):  # (round 0 is the uncounted one)
        for k, sc in cases.items():
            t, feats[k] = path_ms(sc, 64, 4)
            if rnd:
                ms[k].append(t)
    for k, v in ms.items():
        print(f"(b) room 640x480 s64 d4, {k:44s} path kernel median {statistics.median(v):8.3f} ms  runs {' '.join('%.3f' % x for x in v)}  features {feats[k]:#x}",
              file=out)
    base = statistics.median(ms["every texture replaced by its mean colour"])
    for k in list(cases)[:2]:
        print(f"(b) {k} / mean colour: {statistics.median(ms[k]) / base:.3f}", file=out)
    out.flush()


if __name__ == "__main__":
    main()
