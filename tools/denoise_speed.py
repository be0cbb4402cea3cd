#!/usr/bin/env python3
"""DenoiseIntegrator speed on the GPU: the guide pass and the filter (5 iterations, default parameters) on device memory.

    python tools/denoise_speed.py [--reps 9] [--calls 50] > profiles/denoise_speed.txt

Cases: the Cornell box (README camera) at 640 x 640 and at 1920 x 1080.  The film is the guides' albedo under seeded
multiplicative noise -- the filter's cost does not depend on what the colours are, only on which taps are hits.
What is timed: CALLS of the two device entry points (pine_gpu_guides_render_device, pine_gpu_denoise_device) on the current
stream, each between two events recorded on that stream.  A guides call includes uploading the scene's records (it keeps no plan)
and the kernel; a denoise call includes taking its work buffers from the pool, the prepare launch and the iteration launches.
Neither is a kernel time: that takes a kernel trace, which this tool does not run.  2 warm-up calls, then `reps` windows of
`calls` calls; a window's figure is its mean, the case's figure the MEDIAN over the windows (min and max beside it).  Beside the
events' figure stands the host clock's over the same window (every call ends in a stream synchronise).
For scale: the parent commit's C2 path-kernel time from profiles/r04_bench.json.  Not bench.py.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    import torch
    import pine_amd as pa
    from pine_amd import _lib, scenes
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    print(f"# guides + denoise (5 iterations), device entry points; median of {args.reps} windows of {args.calls} calls [min .. max], ms per call")
    for w, h in ((640, 640), (1920, 1080)):
        scene = scenes.cbox((w, h), "readme")
        albedo = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        normal = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        rp = _lib.RenderParams(1, 1, 0, 0, 1, 0, 0, 0)
        prm = pa.api.denoise_params(device=0)

        def guides():
            _lib.check(_lib.lib.pine_gpu_guides_render_device(scene._h, C.byref(rp), ptr(albedo), ptr(normal), sp), "guides")

        guides()
        gen = torch.Generator(device="cuda").manual_seed(7)
        film = torch.ones((h, w, 4), dtype=torch.float32, device="cuda")
        film[..., :3] = albedo * (0.5 + torch.rand((h, w, 3), generator=gen, device="cuda"))
        out = torch.empty_like(film)

        def denoise():
            _lib.check(_lib.lib.pine_gpu_denoise_device(C.byref(prm), w, h, ptr(film), ptr(albedo), ptr(normal), ptr(out), sp), "denoise")

        for what, call in (("guides", guides), ("denoise x5", denoise)):
            for _ in range(2):
                call()
            windows, walls = [], []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record(stream)
                for _ in range(args.calls):
                    call()
                e1.record(stream)
                e1.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3 / args.calls)
                windows.append(e0.elapsed_time(e1) / args.calls)
            ms = statistics.median(windows)
            print(f"cbox {w}x{h} {what:11s} events {ms:8.3f} [{min(windows):.3f} .. {max(windows):.3f}]  host clock {statistics.median(walls):8.3f} "
                  f"[{min(walls):.3f} .. {max(walls):.3f}]  {w * h / ms * 1e-6:.3f} Gpixel/s (events)")
        changed = float((out[..., :3] - film[..., :3]).abs().max())
        print(f"cbox {w}x{h} hits {float((normal != 0).any(dim=2).float().mean()):.4f}; largest change of a colour by the filter {changed:.4f}")
    try:
        bench = json.load(open(os.path.join(ROOT, "profiles", "r04_bench.json")))
        print(f"# for scale, the parent commit's path kernel (profiles/r04_bench.json): {bench['config']['workload']}: "
              f"{bench['ms_per_step']} ms per launch, kernel {bench['roofline']['kernel_ms']} ms")
    except Exception as e:  # noqa: BLE001
        print("# profiles/r04_bench.json not read:", e)


if __name__ == "__main__":
    main()
