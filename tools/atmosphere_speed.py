#!/usr/bin/env python3
"""usage (GPU box): tools/atmosphere_speed.py [--parent DIR] [out.txt]  -- what Atmosphere costs.

(a) lights_zoo 640 x 640, 64 spp, depth 6 (Sky, no Atmosphere): path-kernel time of this build and, with --parent DIR (a built
    checkout of the commit before Atmosphere: its own library and Python package), of that one, alternating in this one call.
(b) the open scene of the fixtures (tests/envsky_scenes.py _open_sun) at 640 x 640, 64 spp, depth 6 under Atmosphere(1024 x 1024)
    against the same scene under Sky: the ratio.
(c) the 1024 x 1024 tables: scene.set(Atmosphere) with the tables computed by the device kernel (copy back included) against the
    host build on min(16, $OMP_NUM_THREADS, hardware) threads: wall time of the whole call after a 1 x 1 call of the same kind,
    so both figures include the same sequential tree build over 2^20 texels.

Path-kernel time comes from the plan's own events (precompiled kernels).  Every run is a process of its own, so that the two
libraries can alternate; each figure is the median of five alternating runs after one uncounted run of each."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("lights_zoo", "open_atmosphere", "open_sky", "table_device", "table_host")


def one(case):
    """One run in this process: prints `<milliseconds> <kernel features or 0>`."""
    sys.path.insert(0, os.getcwd())  # (the checkout this run belongs to: the parent's, or this one)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch  # noqa: F401  (before anything else touches the HIP runtime)
    import pine_amd as pa
    from pine_amd import scenes
    if case.startswith("table"):
        device = 0 if case == "table_device" else None
        s = pa.Scene()
        s.set(pa.Atmosphere((0.3, 1.0, 0.2), (4.0, 4.0, 4.0), (1, 1), device=device))  # (the runtime's and the kernel's first use)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.set(pa.Atmosphere((0.3, 1.0, 0.2), (4.0, 4.0, 4.0), (1024, 1024), device=device))
        print(f"{(time.perf_counter() - t0) * 1e3:.3f} 0")
        return
    if case == "lights_zoo":
        sc = scenes.lights_zoo((640, 640))
    else:
        import envsky_scenes as E
        sc = E._open_sun((640, 640))
        sc.set(pa.Atmosphere((0.3, 1.0, 0.2), (4.0, 4.0, 4.0), device=0) if case == "open_atmosphere" else pa.Sky([1.0, 1.0, 1.0]))
    w, h = sc.camera.film().size
    plan = pa.Plan(sc, 64, 6, specialize=False, timing=True)
    film = torch.zeros((h, w, 4), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plan.launch(film.data_ptr(), s)
    torch.cuda.synchronize()
    plan.launch(film.data_ptr(), s)
    torch.cuda.synchronize()
    st = plan.stats()
    print(f"{st.trace_ms:.4f} {st.kernel_features}")
    plan.close()


def run(case, root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", case], cwd=root, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"{case} in {root} failed ({r.returncode}): {r.stderr[-2000:]}")
    ms, feat = r.stdout.split()[-2:]
    return float(ms), int(feat)


def main(argv):
    parent = None
    if "--parent" in argv:
        parent = os.path.abspath(argv[argv.index("--parent") + 1])
        argv = [a for i, a in enumerate(argv) if a != "--parent" and (i == 0 or argv[i - 1] != "--parent")]
    out = open(argv[0], "w") if argv else sys.stdout
    jobs = [("this build", c, ROOT) for c in CASES]
    if parent:
        jobs.insert(1, ("parent", "lights_zoo", parent))
    runs, feats = {j[:2]: [] for j in jobs}, {}
    for rnd in range(6):  # (round 0 is the uncounted one)
        for who, case, root in jobs:
            ms, feats[(who, case)] = run(case, root)
            if rnd:
                runs[(who, case)].append(ms)
    label = {"lights_zoo": "(a) lights_zoo 640x640 s64 d6 (Sky), path kernel", "open_atmosphere": "(b) open scene 640x640 s64 d6, Atmosphere(1024^2), path kernel",
             "open_sky": "(b) open scene 640x640 s64 d6, Sky, path kernel", "table_device": "(c) set Atmosphere(1024^2), tables on the device, wall",
             "table_host": "(c) set Atmosphere(1024^2), tables on host threads, wall"}
    med = {}
    for (who, case), v in runs.items():
        med[(who, case)] = statistics.median(v)
        print(f"{who:10s} {label[case]:66s} median {med[(who, case)]:9.3f} ms  range {max(v) - min(v):7.3f}  runs {' '.join('%.3f' % x for x in v)}"
              f"  features {feats[(who, case)]:#x}", file=out)
    t = "this build"
    if parent:
        a, b = med[(t, "lights_zoo")], med[("parent", "lights_zoo")]
        print(f"(a) this build / parent: {a / b:.4f} ({a - b:+.3f} ms)", file=out)
    print(f"(b) Atmosphere / Sky: {med[(t, 'open_atmosphere')] / med[(t, 'open_sky')]:.3f}", file=out)
    print(f"(c) host / device: {med[(t, 'table_host')] / med[(t, 'table_device')]:.2f}  (host threads: min(16, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}, hardware))", file=out)
    out.flush()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one(sys.argv[2])
    else:
        main(sys.argv[1:])
