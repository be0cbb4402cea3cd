#!/usr/bin/env python3
"""Measure Accel's batched ray queries on the GPU and write profiles/accel_speed.txt.

    python tools/accel_speed.py [--out profiles/accel_speed.txt] [--size 1920x1080]

Per scene (the Cornell box, the 10 000-cone scene, the Subsurface icosphere room) and traversal order (pine's BVH, EmbreeAccel's):
Mrays/s of intersect and of hit on device buffers, for the film's pixel-centre rays in film order and in one fixed random
permutation of them.  Beside them the yardstick that existed before: one call of the guide pass (pine_gpu_guides_render_device)
on the same film, which walks the same rays through the same traversal and hit_surface and writes 24 bytes per ray where
intersect reads 32 and writes 48.

How a number is taken: every shape is warmed up (3 launches), then windows of K back-to-back launches between two device events,
K chosen so that a window lasts at least 0.25 s; the median of 5 windows, with the spread (min .. max) printed.  The guide pass
synchronises and uploads the scene's records inside every call, so its figure is a call time, not a kernel time: the host clock
around K calls.  No test gates on any of this.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pine_amd as pa  # noqa: E402
from pine_amd import _lib, scenes  # noqa: E402

WINDOW_S, WINDOWS, WARMUP = 0.25, 5, 3


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
    return float(np.median(per_call)), min(per_call), max(per_call), k


def timed_host(fn):
    for _ in range(WARMUP):
        fn()
    t0 = time.perf_counter()
    fn()
    k = max(1, int(WINDOW_S / max(time.perf_counter() - t0, 1e-6)))
    per_call = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        per_call.append((time.perf_counter() - t0) * 1e3 / k)
    return float(np.median(per_call)), min(per_call), max(per_call), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel_speed.txt"))
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("accel_speed: no GPU (a rate is measured on the device or not at all)")
    w, h = (int(x) for x in args.size.split("x"))
    n = w * h
    cases = [("cbox", lambda: scenes.cbox((w, h), "readme")), ("cones10k", lambda: scenes.classic_cones((w, h), 100)),
             ("sss_icosphere", lambda: scenes.sss((w, h), 3))]
    perm = torch.from_numpy(np.random.default_rng(2024).permutation(n)).cuda()
    lines = [f"Accel ray queries, {w} x {h} pixel-centre rays ({n} rays), {torch.cuda.get_device_name(0)}",
             f"median of {WINDOWS} windows of >= {WINDOW_S} s each after {WARMUP} warm-up launches; ms per call (min .. max), Mrays/s of the median",
             "bytes per ray: intersect reads 32 and writes 48 (80), hit reads 32 and writes 1 (33), the guide pass writes 24", ""]
    for name, make in cases:
        sc = make()
        rp = _lib.RenderParams(1, 1, 0, 0, 1, 0, 0, 0)
        albedo = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        normal = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def guide():
            _lib.check(_lib.lib.pine_gpu_guides_render_device(sc._h, C.byref(rp), C.c_void_p(albedo.data_ptr()), C.c_void_p(normal.data_ptr()), stream), "guides")

        g_ms, g_lo, g_hi, g_k = timed_host(guide)
        lines.append(f"== {name} ==")
        lines.append(f"  guide pass, one call (upload + kernel + wait; pine-BVH order) {g_ms:8.3f} ms ({g_lo:.3f} .. {g_hi:.3f}, {g_k} calls per window) "
                     f"{n / g_ms / 1e3:9.1f} Mrays/s")
        for order in ("pine", "embree"):
            with pa.Accel(sc, order=order) as accel:
                ordered = accel.camera_rays(tensor=True)
                permuted = ordered[perm].contiguous()
                hits = torch.empty((n, 12), dtype=torch.float32, device="cuda")
                occ = torch.empty((n,), dtype=torch.uint8, device="cuda")
                # (hit on camera rays of infinite length asks "does the pixel see anything": the any-hit walk of the same rays)
                res = {}
                for what, fn_of in (("intersect", lambda r: lambda: _lib.check(_lib.lib.pine_gpu_accel_intersect_device(
                        accel._h, C.c_void_p(r.data_ptr()), n, C.c_void_p(hits.data_ptr()), stream))),
                                    ("hit", lambda r: lambda: _lib.check(_lib.lib.pine_gpu_accel_hit_device(
                                        accel._h, C.c_void_p(r.data_ptr()), n, C.c_void_p(occ.data_ptr()), stream)))):
                    for arrangement, r in (("film order", ordered), ("permuted", permuted)):
                        ms, lo, hi, k = timed(fn_of(r))
                        res[what, arrangement] = ms
                        per_ray = 80 if what == "intersect" else 33
                        lines.append(f"  {order:6s} {what:9s} {arrangement:10s} {ms:8.3f} ms ({lo:.3f} .. {hi:.3f}, {k} launches per window) "
                                     f"{n / ms / 1e3:9.1f} Mrays/s {n * per_ray / ms / 1e6:8.1f} GB/s of rays and answers")
                for what in ("intersect", "hit"):
                    lines.append(f"  {order:6s} {what:9s} permuted / film order = {res[what, 'permuted'] / res[what, 'film order']:.2f}")
                if order == "pine":
                    lines.append(f"  intersect (film order) - guide call = {res['intersect', 'film order'] - g_ms:+.3f} ms; 56 more bytes per ray are {n * 56 / 1e6:.1f} MB")
        lines.append("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
