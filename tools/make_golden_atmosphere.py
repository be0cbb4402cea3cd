#!/usr/bin/env python3
"""Generate tests/golden/atmos_*.npz and atmos.json from the REAL reference's Atmosphere light and atmosphere_color.

Runs only where the reference's sources are: tools/ref_atmosphere_driver.cpp is compiled in place against them and linked with
oracle/_ref/libpine_ref.a (make -C oracle ref).  The binary goes to a scratch directory; nothing of the reference is copied
into this tree.  No test calls this tool: the tests read what it wrote.

    python tools/make_golden_atmosphere.py [color] [configs] [films]

atmos_color.npz: the queries of tests/atmosphere_scenes.py color_queries() and the reference's atmosphere_color of each.
Per configuration (CONFIGS): the 512 queries, the reference's 13-float record of each, the Distribution2D(density, 15) as a
pre-order stream and the density's md5 -- the whole density and tree for the small configurations, the first 64 nodes for
`mid` and `default`.  Per film: the film and the .pscene text.

Expected of the reference, and checked (a disagreement is listed in atmos.json and the tool exits with an error after writing
the fixtures, which are the reference's numbers either way): 47 - 50 % of a configuration's texels have density 0 (the lower
hemisphere); the sun disc covers 2 - 3 texels at 64 x 32 and 900 - 1200 at 1024 x 1024, and `low`'s holds more than 90 % of
the weight.  The 64 x 32 configurations are known to miss the first: 15 of their 32 rows, 46.9 %, lie under the horizon row,
whose directions still have a positive height.
Asserted here, of the reference's own numbers: every density finite and >= 0; at least 30 distinct sampled texels (8 for
`tall` and `low`); in `mid` and `default` at least 10 records whose ds.p lies in a leaf of more than one texel and non-zero weight; at least 5 queried directions with pdf(wo) == 0;
every film pixel finite, at least 20 % of the centre camera rays miss, at least 100 distinct pixel values.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import atmosphere_scenes as A  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
OUT = os.path.join(ROOT, "tests", "golden")
SEARCH = 1 << 20
DISAGREE = []  # expectations of the module text's second paragraph that the reference does not meet


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_atmosphere_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_atmosphere_driver.cpp"), "-o", exe, ARCHIVE, "-pthread",
                           "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def light_args(name, color):
    w, h, sun = A.CONFIGS[name]
    return [float(np.float32(v)).hex() for v in (*sun, *color)] + [str(w), str(h)]


def do_color(exe, tmp, listing):
    q = A.color_queries()
    qp, op = os.path.join(tmp, "cq.bin"), os.path.join(tmp, "co.bin")
    q.tofile(qp)
    subprocess.check_call([exe, "color", qp, op])
    out = np.fromfile(op, dtype=np.float32).reshape(-1, 3)
    assert len(out) == len(q) and np.isfinite(out).all()
    with_sun, without = out[q[:, 6] != 0], out[q[:, 6] == 0]
    in_disc = int((with_sun != without).any(axis=1).sum())
    # (per sun above the horizon the sun itself and one of each pair; towards (0, -1, 0) the colour is zero with or without a disc)
    assert in_disc >= 4 * 4, f"only {in_disc} directions inside a sun disc"
    np.savez_compressed(os.path.join(OUT, "atmos_color.npz"), queries=q, colors=out)
    listing["color"] = {"queries": int(len(q)), "inside_a_sun_disc": in_disc, "zero": int((out == 0).all(axis=1).sum())}
    print("color", listing["color"], flush=True)


def texel_directions(w, h):
    """wo of every texel (float64: for counting only)."""
    y, x = np.mgrid[0:h, 0:w]
    phi, ct = x / w * 2 * np.pi, 1 - 2 * (y / h)
    st = np.sqrt(np.maximum(0, 1 - ct * ct))
    return np.stack([st * np.cos(phi), ct, st * np.sin(phi)], axis=2)


def leaves_of(stream):
    return stream[stream[:, 6] == 1]


def do_config(exe, tmp, name, listing):
    w, h, sun = A.CONFIGS[name]
    args = light_args(name, A.SUN_COLOR)
    qp, rp, dp, tp, sp = (os.path.join(tmp, x) for x in ("q.bin", "r.bin", "d.bin", "t.bin", "s.bin"))
    subprocess.check_call([exe, "density"] + args + [dp])
    density = np.fromfile(dp, dtype=np.float32).reshape(h, w)
    assert np.isfinite(density).all() and (density >= 0).all(), f"{name}: a density is negative or not finite"
    zero = float((density == 0).mean())
    disc = (texel_directions(w, h) @ A.normalized(sun).astype(np.float64)) > float(np.float32(0.998))
    disc_texels, disc_weight = int(disc.sum()), float(density[disc].sum(dtype=np.float64) / density.sum(dtype=np.float64))
    # what is expected of the reference (the module text): where it disagrees the fixtures are still its own numbers, and the
    # tool fails at the end with the list
    if not 0.47 <= zero <= 0.50:
        DISAGREE.append(f"{name}: {zero:.4f} of the texels have density 0, not 47 - 50 %")
    if name in ("noon", "low") and not 2 <= disc_texels <= 3:
        DISAGREE.append(f"{name}: the sun disc covers {disc_texels} texels, not 2 - 3")
    if name == "default" and not 900 <= disc_texels <= 1200:
        DISAGREE.append(f"{name}: the sun disc covers {disc_texels} texels, not about 1 050")
    if name == "low" and not disc_weight > 0.9:
        DISAGREE.append(f"low: the sun disc holds {disc_weight:.3f} of the weight, not more than 0.9")
    subprocess.check_call([exe, "tree"] + args + [tp])
    stream = np.fromfile(tp, dtype=np.int32).reshape(-1, 7)

    q = A.base_queries(name)
    q.tofile(qp)
    subprocess.check_call([exe, "calls"] + args + [qp, rp])
    first = np.fromfile(rp, dtype=np.float32).reshape(-1, 13)
    q[384:448, 2:5] = first[:64, 3:6]  # directions that sample() itself returned
    found = np.zeros((0, 2), dtype=np.float32)
    if name in A.SMALL:  # u2 whose ds.p has a coordinate equal to the image size
        subprocess.check_call([exe, "search"] + args + [str(SEARCH), sp])
        found = np.fromfile(sp, dtype=np.float32).reshape(-1, 2)
        q[448:448 + len(found), 0:2] = found
    q.tofile(qp)
    subprocess.check_call([exe, "calls"] + args + [qp, rp])
    rec = np.fromfile(rp, dtype=np.float32).reshape(-1, 13)
    assert len(rec) == A.NUM_QUERIES and np.isfinite(rec).all()
    texels = len({(int(a), int(b)) for a, b in rec[:, :2]})
    zero_pdf = int((rec[:, 12] == 0).sum())
    on_edge = int(((rec[:, 0] == w) | (rec[:, 1] == h)).sum())
    assert texels >= (8 if name in ("tall", "low") else 30), f"{name}: only {texels} distinct sampled texels"
    assert zero_pdf >= 5, f"{name}: pdf 0 for only {zero_pdf} queried directions"
    entry = {"size": [w, h], "nodes": int(len(stream)), "sampled_texels": texels, "zero_pdf_queries": zero_pdf, "zero_density": round(zero, 4),
             "sun_disc_texels": disc_texels, "sun_disc_weight": round(disc_weight, 4), "tree_md5": hashlib.md5(stream.tobytes()).hexdigest(),
             "density_md5": hashlib.md5(density.tobytes()).hexdigest()}
    if name in A.SMALL:
        entry["search"] = {"u2_tried": SEARCH, "found": int(len(found)), "records_on_row_h_or_column_w": on_edge}
    else:
        big = leaves_of(stream)
        big = big[((big[:, 4] - big[:, 2]) * (big[:, 5] - big[:, 3]) > 1) & (big[:, 0] != 0)]
        inside = 0
        for px, py in rec[:, :2]:
            inside += bool(((big[:, 2] <= px) & (px < big[:, 4]) & (big[:, 3] <= py) & (py < big[:, 5])).any())
        assert inside >= 10, f"{name}: only {inside} records in a leaf of more than one texel"
        entry["records_in_wide_leaves"] = inside
    data = {"queries": q, "records": rec}
    if name in A.SMALL:
        data["tree"], data["density"] = stream, density
    else:
        data["tree"] = stream[:64].copy()
    np.savez_compressed(os.path.join(OUT, f"atmos_{name}.npz"), **data)
    listing["configs"][name] = entry
    print(name, entry, os.path.getsize(os.path.join(OUT, f"atmos_{name}.npz")), "bytes", flush=True)


def do_film(exe, tmp, name, listing):
    config, kind, spp, depth = A.FILMS[name]
    scene = A.film_scene(name)
    w, h = A.FILM_SIZE
    ps = scene.describe()
    lines = ps.splitlines()
    assert len([ln for ln in lines if ln.startswith("envlight atmosphere ")]) == 1
    sp, fp, mp = (os.path.join(tmp, x) for x in ("s.pscene", "s.film", "s.miss"))
    open(sp, "w").write("\n".join(ln for ln in lines if not ln.startswith("envlight atmosphere ")) + "\n")
    subprocess.check_call([exe, "film"] + light_args(config, A.FILM_SUN_COLOR) + [sp, str(spp), kind, str(depth), fp, mp])
    film = np.fromfile(fp, dtype=np.float32).reshape(h, w, 4)
    miss = float(np.fromfile(mp, dtype=np.uint8).mean())
    distinct = len(np.unique(film.reshape(-1, 4).view(np.uint32), axis=0))
    assert np.isfinite(film).all()
    assert miss >= 0.20, f"{name}: only {miss:.3f} of the centre camera rays miss"
    assert distinct >= 100, f"{name}: only {distinct} distinct pixel values"
    np.savez_compressed(os.path.join(OUT, f"atmos_film_{name}.npz"), film=film, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["films"][name] = {"config": config, "size": [w, h], "sampler": kind, "spp": spp, "depth": depth, "centre_ray_misses": round(miss, 4),
                              "distinct_pixels": distinct, "mean": float(film[..., :3].mean(dtype=np.float64))}
    print(name, listing["films"][name], os.path.getsize(os.path.join(OUT, f"atmos_film_{name}.npz")), "bytes", flush=True)


def main(what):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    what = what or ["color", "configs", "films"]
    path = os.path.join(OUT, "atmos.json")
    listing = json.load(open(path)) if os.path.exists(path) else {}
    for k in ("color", "configs", "films"):
        listing.setdefault(k, {})
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "color" in what:
            do_color(exe, tmp, listing)
        if "configs" in what:
            for name in A.CONFIGS:
                do_config(exe, tmp, name, listing)
        if "films" in what:
            for name in A.FILMS:
                do_film(exe, tmp, name, listing)
    if "configs" in what:
        listing["expectations_not_met"] = DISAGREE
    json.dump(listing, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")
    if DISAGREE:
        sys.exit("the reference does not meet what is expected of it (fixtures written all the same):\n  " + "\n  ".join(DISAGREE))


if __name__ == "__main__":
    main(sys.argv[1:])
