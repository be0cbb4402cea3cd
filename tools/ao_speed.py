#!/usr/bin/env python3
"""AOIntegrator speed: the regrouped kernel against its plain twin ($PINE_GPU_AO_KERNEL=serial), per scene.

    python tools/ao_speed.py [--reps 7] [--launches 5] [--only cbox] > profiles/ao_speed.txt

Cases: cbox 640 x 640, the 10 000-cone scene 720 x 360, the Subsurface-icosphere scene 640 x 640, each with
BlueSampler(256) = 32 AO samples per pixel.  Per case and schedule: a resident plan, 3 warm-up launches, then `reps`
windows of `launches` launches each; a window's figure is the mean trace_ms (HIP events around the AO kernel) of its
launches, the case's figure the MEDIAN over the windows (min and max beside it).  The two schedules take turns window by
window, so that a drift of the machine meets both alike.  Both films are checked to be the same bits.  Not bench.py.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "cbox": lambda s: s.cbox((640, 640), "readme"),
    "cones10k": lambda s: s.classic_cones((720, 360), 100),
    "sss_icosphere": lambda s: s.sss((640, 640), 3),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    import pine_amd as pa
    from pine_amd import scenes
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# AOIntegrator(BVH(), BlueSampler(256)): 32 samples per pixel; median of {args.reps} windows of {args.launches} launches [min .. max]")
    for name, build in CASES.items():
        if args.only and name != args.only:
            continue
        scene = build(scenes)
        w, h = scene.camera.film().size
        plans, films = {}, {}
        for kernel in ("regroup", "serial"):
            os.environ["PINE_GPU_AO_KERNEL"] = kernel
            plans[kernel] = pa.Plan(scene, 256, 1, integrator="ao", timing=True)
            films[kernel] = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            for _ in range(3):
                plans[kernel].launch(films[kernel].data_ptr(), stream)
            plans[kernel].stats()
        os.environ.pop("PINE_GPU_AO_KERNEL")
        windows = {"regroup": [], "serial": []}
        for _ in range(args.reps):
            for kernel in ("regroup", "serial"):
                for _ in range(args.launches):
                    plans[kernel].launch(films[kernel].data_ptr(), stream)
                windows[kernel].append(plans[kernel].stats().trace_ms)
        same = bool(torch.equal(films["regroup"], films["serial"]))
        for kernel in ("regroup", "serial"):
            st = plans[kernel].stats()
            ms = statistics.median(windows[kernel])
            print(f"{name:14s} {w}x{h} {kernel:8s} trace_ms {ms:8.3f} [{min(windows[kernel]):.3f} .. {max(windows[kernel]):.3f}]  "
                  f"camera samples/s {st.camera_samples / ms * 1e3:.4g}  any-hit rays/s {st.shadow_rays / ms * 1e3:.4g}  "
                  f"hits/sample {st.vertices / st.camera_samples:.3f}  grid {st.grid_blocks} x {st.block_threads}  lds {st.lds_bytes}  "
                  f"samples/item {st.samples_per_item}")
        r, s = statistics.median(windows["regroup"]), statistics.median(windows["serial"])
        print(f"{name:14s} regroup / serial = {r / s:.3f}  films identical: {same}")
        if not same:
            sys.exit("the two schedules disagree")
        for p in plans.values():
            p.close()


if __name__ == "__main__":
    main()
