#!/usr/bin/env python3
"""Generate tests/golden/noise_*.npz and noise.json from the REAL reference's NodeNoisef / NodeNoise3f.

Runs only where the reference's sources are: tools/ref_noise_driver.cpp is compiled in place against them, together with the
reference's impl/integrator/denoiser.cpp read from where it lies, and linked with oracle/_ref/libpine_ref.a (make -C oracle
ref).  The binary goes to a scratch directory; nothing of the reference is copied into this tree.  No test calls this tool:
the tests read what it wrote.

    python tools/make_golden_noise.py [calls] [films]

calls: the scene noise_zoo (tests/noise_scenes.py) at 384 queries: the reference's 10-float record per material and query.
films: the two rooms' films and the first room's albedo / normal guide pair, with the .pscene text of each.

Asserted here, on the inputs and with the reference alone (an assertion that fails asks for other queries, not for a weaker
assertion): every query is finite and inside the pinned domain |coordinate| * 2^(octaves - 1) < 2^30 for the zoo's largest
factor on a coordinate and its largest octave count; at least 25 % of the queries have a negative coordinate, at least 8 per
axis lie exactly on an integer, at least 16 have a coordinate of magnitude 2^16 or more; every record is finite, but those of
the oct0_* materials, which are NaN in the noise-driven slot at every query; the varying-octaves materials meet each of the
counts 1, 2, 3, 4 at 16 queries or more; per material that reads the surface at least 90 % of the queries give distinct
records; and the queries tell perlin_interp's binary64 step from a binary32 one: of fbm at every query and 1 to 8 octaves, at
least 16 results differ from the same sum over an interpolation written with `1.0f` (the count goes into noise.json).  Films:
the camera ray through the centre of at least 25 % of the pixels meets a noise-driven surface first (counted by the driver
with the reference's BVH), at least 100 distinct pixel values, every pixel finite.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_scenes as X  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
OUT = os.path.join(ROOT, "tests", "golden")
FRONT = ("node ", "material ")


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_noise_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_noise_driver.cpp"), os.path.join(REF_SRC, "pine", "impl", "integrator", "denoiser.cpp"),
                           "-o", exe, ARCHIVE, "-pthread", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def split_scene(tmp, ps):
    """The .pscene text as the driver's two files."""
    lines = [ln for ln in ps.splitlines() if ln and not ln.startswith("#")]
    fp, rp = os.path.join(tmp, "front.txt"), os.path.join(tmp, "rest.pscene")
    open(fp, "w").write("\n".join(ln for ln in lines if ln.startswith(FRONT)) + "\n")
    open(rp, "w").write("\n".join(ln for ln in lines if not ln.startswith(FRONT)) + "\n")
    return fp, rp


def do_calls(exe, tmp, listing):
    q = X.queries()
    assert q.shape == (X.NUM_QUERIES, 8) and np.isfinite(q).all(), "a query is not finite"
    reach = np.abs(q[:, [0, 1, 2, 3, 4, 5, 6, 7]]).max() * X.P_SCALE * 2.0 ** (X.MAX_OCTAVES - 1)
    assert reach < 2.0 ** 30, f"a query leaves the pinned domain: {reach}"
    coords = q[:, [0, 1, 2, 6, 7]]
    negative = float((coords < 0).any(axis=1).mean())
    on_integer = [int(((q[:, a] == np.floor(q[:, a])) & (np.abs(q[:, a]) < 2.0 ** 16)).sum()) for a in range(3)]
    large = int((np.abs(q[:, 0:3]) >= 2.0 ** 16).any(axis=1).sum())
    assert negative >= 0.25, negative
    assert min(on_integer) >= 8, on_integer
    assert large >= 16, large
    counts = np.bincount(X.varying_octaves_of(q), minlength=5)
    assert counts[0] == 0 and len(counts) == 5 and counts[1:].min() >= 16, counts

    sc, names = X.noise_zoo(q)
    ps = sc.describe()
    order = [ln.split()[1] for ln in ps.splitlines() if ln.startswith("material ")]
    assert len(order) == len(names) and order[-2:] == list(X.OCT0)
    fp, _ = split_scene(tmp, ps)
    qp, rp = os.path.join(tmp, "q.bin"), os.path.join(tmp, "r.bin")
    q.tofile(qp)
    print(subprocess.check_output([exe, "calls", fp, qp, rp]).decode().strip(), flush=True)
    rec = np.fromfile(rp, dtype=np.float32).reshape(len(names), len(q), 10)
    assert np.isfinite(rec[:-2]).all(), "a record is not finite"
    assert np.isnan(rec[-2][:, 0:6]).all() and np.isfinite(rec[-2][:, 6:]).all(), "oct0_albedo: NaN expected in the albedo slots alone"
    assert np.isnan(rec[-1][:, 6]).all() and np.isfinite(np.delete(rec[-1], 6, axis=1)).all(), "oct0_roughness: NaN expected in the roughness slot alone"
    surface = len(names) - 2 - len(X.twins())
    distinct = [len(np.unique(rec[i].view(np.uint32), axis=0)) / len(q) for i in range(surface)]
    assert min(distinct) >= 0.9, (min(distinct), names[int(np.argmin(distinct))])
    for t, o in X.twins():  # (a twin is one value, its original's at the twin's query)
        assert len(np.unique(rec[t].view(np.uint32), axis=0)) == 1
        assert np.array_equal(rec[t][0].view(np.uint32), rec[o][X.TWIN_QUERY].view(np.uint32)), names[t]
    sense = json.loads(subprocess.check_output([exe, "sense", qp, str(X.MAX_OCTAVES)]).decode())
    assert sense["differ_with_float_interp"] >= 16, sense
    np.savez_compressed(os.path.join(OUT, "noise_zoo.npz"), queries=q, records=rec, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["calls"] = {"materials": len(names), "queries": len(q), "negative_fraction": round(negative, 4), "on_integer_per_axis": on_integer,
                        "large_magnitude": large, "varying_octaves_counts": {str(k): int(counts[k]) for k in range(1, 5)},
                        "least_distinct_fraction": round(min(distinct), 4), "fbm_evaluations": sense["evaluations"],
                        "differ_with_float_interp": sense["differ_with_float_interp"]}
    print("calls", listing["calls"], os.path.getsize(os.path.join(OUT, "noise_zoo.npz")), "bytes", flush=True)


def do_films(exe, tmp, listing):
    for name, (size, spp, depth) in X.FILMS.items():
        w, h = size
        ps = X.film_scene(name).describe()
        fp, rp = split_scene(tmp, ps)
        op, hp = os.path.join(tmp, "s.film"), os.path.join(tmp, "s.first")
        subprocess.check_call([exe, "film", fp, rp, str(spp), str(depth), op, hp])
        film = np.fromfile(op, dtype=np.float32).reshape(h, w, 4)
        first = np.fromfile(hp, dtype=np.uint8)
        order = [ln.split()[1] for ln in ps.splitlines() if ln.startswith("material ")]
        noisy = float(np.isin(first, [1 + order.index(m) for m in X.NOISY]).mean())
        distinct = len(np.unique(film.reshape(-1, 4).view(np.uint32), axis=0))
        assert np.isfinite(film).all()
        assert noisy >= 0.25, f"{name}: only {noisy:.3f} of the centre camera rays meet a noise-driven surface first"
        assert distinct >= 100, f"{name}: only {distinct} distinct pixel values"
        np.savez_compressed(os.path.join(OUT, f"noise_film_{name}.npz"), film=film, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
        listing["films"][name] = {"size": [w, h], "spp": spp, "depth": depth, "centre_rays_on_noise": round(noisy, 4), "distinct_pixels": distinct,
                                  "mean": float(film[..., :3].mean(dtype=np.float64))}
        print(name, listing["films"][name], os.path.getsize(os.path.join(OUT, f"noise_film_{name}.npz")), "bytes", flush=True)
    w, h = X.GUIDES_SIZE
    ps = X.room(X.GUIDES_SIZE).describe()
    fp, rp = split_scene(tmp, ps)
    ap, np_ = os.path.join(tmp, "g.albedo"), os.path.join(tmp, "g.normal")
    subprocess.check_call([exe, "guides", fp, rp, ap, np_])
    albedo = np.fromfile(ap, dtype=np.float32).reshape(h, w, 3)
    normal = np.fromfile(np_, dtype=np.float32).reshape(h, w, 3)
    distinct = len(np.unique(albedo.reshape(-1, 3).view(np.uint32), axis=0))
    assert np.isfinite(albedo).all() and np.isfinite(normal).all()
    assert distinct >= 100, f"guides: only {distinct} distinct albedo values"
    np.savez_compressed(os.path.join(OUT, "noise_guides_room.npz"), albedo=albedo, normal=normal, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["guides"] = {"size": [w, h], "distinct_albedo": distinct}
    print("guides", listing["guides"], flush=True)


def main(what):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    what = what or ["calls", "films"]
    path = os.path.join(OUT, "noise.json")
    listing = json.load(open(path)) if os.path.exists(path) else {}
    listing.setdefault("films", {})
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "calls" in what:
            do_calls(exe, tmp, listing)
        if "films" in what:
            do_films(exe, tmp, listing)
    json.dump(listing, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
