#!/usr/bin/env python3
"""Measure Shader's batched path-vertex queries and the wavefront loop on the GPU and write profiles/shade_speed.txt.

    python tools/shade_speed.py [--out profiles/shade_speed.txt] [--size 1920x1080] [--spp 16] [--depth 5]

Per scene (the Cornell box: the narrow vertex kernel; materials_zoo: the all-features one):
  * the time of every call of one sample of the loop -- begin, then per level intersect, vertex and hit, then fold -- over all
    W * H paths (no compaction: a finished path costs a null ray and a "none" record);
  * the whole render through WavefrontPathIntegrator beside PathIntegrator's on the same scene, spp and depth, both by the host
    clock around render() (creation, every launch, the download), and Plan.launch alone between two device events.

How a number is taken: as tools/accel_speed.py does -- every call is warmed up (3 launches), then windows of K back-to-back launches
between two device events, K chosen so that a window lasts at least 0.25 s; the median of 5 windows, with the spread (min .. max).
Each call runs on the inputs the loop gives it at its level of sample 0.  The whole renders: the median of REPEATS calls after one
warm-up call.  No test gates on
any of this: the file records what was measured, so that a later change has a number to beat.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pine_amd as pa  # noqa: E402
from pine_amd import scenes  # noqa: E402

WINDOW_S, WINDOWS, WARMUP, REPEATS = 0.25, 5, 3, 5


def stats(xs):
    return float(np.median(xs)), float(min(xs)), float(max(xs))


def timed(fn):
    """Median, min and max milliseconds per call of fn (which enqueues on the current stream) over WINDOWS windows."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(), fn(), b.record()
    torch.cuda.synchronize()
    k = max(1, int(WINDOW_S * 1e3 / max(a.elapsed_time(b), 1e-3)))
    per_call = []
    for _ in range(WINDOWS):
        a.record()
        for _ in range(k):
            fn()
        b.record()
        torch.cuda.synchronize()
        per_call.append(a.elapsed_time(b) / k)
    return stats(per_call)


def per_call_times(scene, spp, depth):
    """[(call name, (median, min, max) ms)] of the calls of one sample of the loop (sample 0), each on the inputs the loop gives
    it: the sample is rendered once and every level's rays, hits and states are kept.  A vertex call advances the states in
    place, so a timed call is `copy the level's states back, vertex`, and the copy, timed alone, is subtracted."""
    out = []
    with pa.Accel(scene) as accel, pa.Shader(scene, pa.BlueSampler(spp), depth) as sh:
        n = sh.film_size[0] * sh.film_size[1]
        dev = torch.device("cuda", 0)
        records = torch.empty((depth, n, 16), dtype=torch.float32, device=dev)
        occluded = torch.empty((depth, n), dtype=torch.uint8, device=dev)
        sums = torch.empty((n, 4), dtype=torch.float32, device=dev)
        nxt = torch.empty((n, 8), dtype=torch.float32, device=dev)
        states, rays = sh.begin(0)
        levels, live = [], []
        for level in range(depth):
            hits = accel.intersect(rays)
            before = states.clone()
            shadow = torch.empty((n, 8), dtype=torch.float32, device=dev)
            _, _, following = sh.vertex(rays, hits, states, records[level], shadow)
            accel.hit(shadow, out=occluded[level])
            levels.append((rays, hits, before, shadow))
            live.append(float((states[:, 7] == 0).float().mean()))
            rays = following
        work = states.clone()
        out.append(("begin", timed(lambda: sh.begin(0, work, nxt)), ""))
        copy = timed(lambda: work.copy_(levels[0][2]))
        for level, (r, h, st, sh_rays) in enumerate(levels):
            out.append((f"intersect level {level}", timed(lambda: accel.intersect(r, out=h.records)), ""))
            both = timed(lambda: (work.copy_(st), sh.vertex(r, h, work, records[level], sh_rays, nxt)))
            ms = tuple(x - copy[0] for x in both)
            out.append((f"vertex    level {level}", ms, f" {n / ms[0] / 1e3:9.1f} Mvertices/s (paths still live after it: {100 * live[level]:.1f} %)"))
            out.append((f"hit       level {level}", timed(lambda: accel.hit(sh_rays, out=occluded[level])), ""))
        out.append((f"fold, {depth} levels", timed(lambda: sh.fold(records, occluded, 0, sums)), ""))
        out.append(("(the 32-byte state copy subtracted from every vertex line)", copy, ""))
        return out, n, sh.variant, sh.kernel_features, sh.lds_bytes


def host_ms(fn):
    fn()
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def plan_launch_ms(scene, spp, depth):
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, spp, depth, specialize=False)
    film = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    plan.launch(film.data_ptr(), stream)
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.launch(film.data_ptr(), stream)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    plan.check()
    plan.close()
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_speed.txt"))
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shade_speed: no GPU (a rate is measured on the device or not at all)")
    w, h = (int(x) for x in args.size.split("x"))
    spp, depth = args.spp, args.depth
    lines = [f"Shader vertex queries and the wavefront loop, {w} x {h} ({w * h} paths), {spp} spp, depth {depth}, {torch.cuda.get_device_name(0)}",
             f"per call: median of {WINDOWS} windows of >= {WINDOW_S} s each after {WARMUP} warm-up launches; ms per call (min .. max)",
             "bytes per path and call: begin writes 64; vertex reads 112 (ray, hit, state) and writes 160 (record, two rays, state); fold reads",
             "65 per level and 16 (sum) and writes 16", ""]
    for name, make in (("cbox", lambda: scenes.cbox((w, h), "readme")), ("materials_zoo", lambda: scenes.materials_zoo((w, h)))):
        sc = make()
        times, n, variant, features, lds = per_call_times(sc, spp, depth)
        lines.append(f"== {name} == vertex kernel variant {variant} (features 0x{features:x}, {lds} bytes of LDS)")
        total = 0.0
        for call, (ms, lo, hi), extra in times:
            if not call.startswith("("):
                total += ms
            lines.append(f"  {call:18s} {ms:8.3f} ms ({lo:.3f} .. {hi:.3f}){extra}")
        lines.append(f"  one sample, the sum of the medians above: {total:.3f} ms = {n / total / 1e3:.1f} Msamples/s")
        wf = host_ms(lambda: pa.WavefrontPathIntegrator(pa.BlueSampler(spp), depth).render(sc))
        fused = host_ms(lambda: pa.PathIntegrator(pa.BlueSampler(spp), depth, specialize=False).render(sc))
        launch = plan_launch_ms(sc, spp, depth)
        lines.append(f"  WavefrontPathIntegrator.render (host clock: creation, {spp * (3 * depth + 2) + 1} launches, download) {wf[0]:9.2f} ms ({wf[1]:.2f} .. {wf[2]:.2f}) "
                     f"{n * spp / wf[0] / 1e3:8.1f} Msamples/s")
        lines.append(f"  PathIntegrator.render, precompiled kernel (host clock: creation, launch, download)   {fused[0]:9.2f} ms ({fused[1]:.2f} .. {fused[2]:.2f}) "
                     f"{n * spp / fused[0] / 1e3:8.1f} Msamples/s")
        lines.append(f"  Plan.launch alone, precompiled kernel (device events)                                {launch[0]:9.2f} ms ({launch[1]:.2f} .. {launch[2]:.2f}) "
                     f"{n * spp / launch[0] / 1e3:8.1f} Msamples/s")
        lines.append(f"  the loop's launches / Plan.launch = {total * spp / launch[0]:.2f}; render / render = {wf[0] / fused[0]:.2f}")
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
