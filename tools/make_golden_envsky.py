#!/usr/bin/env python3
"""Generate tests/golden/envsky_*.npz, envsky_reader_*.hdr and envsky.json from the REAL reference's ImageSky.

Runs only where the reference's sources are: tools/ref_envsky_driver.cpp is compiled in place against them and linked with
oracle/_ref/libpine_ref.a (make -C oracle ref).  The binary goes to a scratch directory; nothing of the reference is copied
into this tree.  No test calls this tool: the tests read what it wrote.

    python tools/make_golden_envsky.py [images] [films] [reader]

Per image (tests/envsky_scenes.py IMAGES): the 512 queries, the reference's 13-float record of each, the Distribution2D as a
pre-order stream (whole for the small images; node count, md5 and the first 64 nodes for `deep`), and for the 8-bit image the
texels Image::operator[] returns.  Per film: the film and the .pscene text.  The reader: one 9 x 5 Radiance file written twice,
flat and run-length encoded, with the floats the reference's image_from returned for each.

Asserted here: no query makes the reference read outside its image; every image but `const` and `black` has at least 30
distinct sampled texels; `sun` returns pdf 0 for at least 5 queried directions; in the films of NEED_MISSES the camera ray
through the centre of at least 20 % of the pixels meets nothing (counted by the driver with the reference's own BVH); no film
but black_24 has fewer than 100 distinct pixel values.
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
import envsky_scenes as E  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
OUT = os.path.join(ROOT, "tests", "golden")


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_envsky_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_envsky_driver.cpp"), "-o", exe, ARCHIVE, "-pthread",
                           "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def image_args(tmp, name):
    w, h, dtype, tint, elevation, rotation = E.IMAGES[name]
    path = os.path.join(tmp, name + ".texels")
    E.image(name).tofile(path)
    return [path, str(w), str(h), dtype] + [float(np.float32(v)).hex() for v in (*tint, elevation, rotation)]


def do_image(exe, tmp, name, listing):
    w, h = E.IMAGES[name][:2]
    args = image_args(tmp, name)
    qp, rp, fp, tp = (os.path.join(tmp, x) for x in ("q.bin", "r.bin", "f.bin", "t.bin"))
    q = E.base_queries(name)
    q.tofile(qp)
    subprocess.check_call([exe, "calls"] + args + [qp, rp, fp])
    first = np.fromfile(rp, dtype=np.float32).reshape(-1, 13)
    # (an edge u2 that would make the reference read past the end of its array -- the last row with a coordinate equal to
    #  `upper` -- is halved: the reference has no answer for it)
    q[np.fromfile(fp, dtype=np.uint8) != 0, 0:2] *= np.float32(0.5)
    q[384:448, 2:5] = first[:64, 3:6]  # directions that sample() itself returned
    q.tofile(qp)
    subprocess.check_call([exe, "calls"] + args + [qp, rp, fp])
    rec = np.fromfile(rp, dtype=np.float32).reshape(-1, 13)
    flags = np.fromfile(fp, dtype=np.uint8)
    assert len(rec) == E.NUM_QUERIES and not flags.any(), f"{name}: {int(flags.sum())} queries make the reference read outside its image"
    texels = len({(int(a), int(b)) for a, b in rec[:, :2]})
    zero_pdf = int((rec[:, 12] == 0).sum())
    if name not in ("const", "black"):
        assert texels >= 30, f"{name}: only {texels} distinct sampled texels"
    if name == "sun":
        assert zero_pdf >= 5, f"sun: pdf 0 for only {zero_pdf} queried directions"
    subprocess.check_call([exe, "tree"] + args + [tp])
    stream = np.fromfile(tp, dtype=np.int32).reshape(-1, 7)
    data = {"queries": q, "records": rec}
    entry = {"size": [w, h], "nodes": int(len(stream)), "sampled_texels": texels, "zero_pdf_queries": zero_pdf,
             "tree_md5": hashlib.md5(stream.tobytes()).hexdigest()}
    data["tree"] = stream if name in E.SMALL else stream[:64].copy()
    if E.IMAGES[name][2] == "u8":
        subprocess.check_call([exe, "texels"] + args + [tp])
        data["texels"] = np.fromfile(tp, dtype=np.float32).reshape(h, w, 3)
    np.savez_compressed(os.path.join(OUT, f"envsky_{name}.npz"), **data)
    listing["images"][name] = entry
    print(name, entry, os.path.getsize(os.path.join(OUT, f"envsky_{name}.npz")), "bytes", flush=True)


def do_film(exe, tmp, name, listing):
    img, size, kind, spp, depth = E.FILMS[name]
    scene = E.film_scene(name)
    w, h = size
    ps = scene.describe()
    lines = ps.splitlines()
    env = [ln for ln in lines if ln.startswith("envlight image ")]
    assert len(env) == 1
    sp, fp, mp = (os.path.join(tmp, x) for x in ("s.pscene", "s.film", "s.miss"))
    open(sp, "w").write("\n".join(ln for ln in lines if not ln.startswith("envlight image ")) + "\n")
    subprocess.check_call([exe, "film"] + image_args(tmp, img) + [sp, str(spp), kind, str(depth), fp, mp])
    film = np.fromfile(fp, dtype=np.float32).reshape(h, w, 4)
    miss = float(np.fromfile(mp, dtype=np.uint8).mean())
    distinct = len(np.unique(film.reshape(-1, 4).view(np.uint32), axis=0))
    assert np.isfinite(film).all()
    if name in E.NEED_MISSES:
        assert miss >= 0.20, f"{name}: only {miss:.3f} of the centre camera rays miss"
    if not name.startswith("black_24"):
        assert distinct >= 100, f"{name}: only {distinct} distinct pixel values"
    np.savez_compressed(os.path.join(OUT, f"envsky_film_{name}.npz"), film=film, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["films"][name] = {"image": img, "size": [w, h], "sampler": kind, "spp": spp, "depth": depth, "centre_ray_misses": round(miss, 4),
                              "distinct_pixels": distinct, "mean": float(film[..., :3].mean(dtype=np.float64))}
    print(name, listing["films"][name], os.path.getsize(os.path.join(OUT, f"envsky_film_{name}.npz")), "bytes", flush=True)


def rle_component(row):
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, row[i]])
            i += run
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and row[j] == row[j + 1] == row[j + 2]):
            j += 1
        out += bytes([j - i]) + bytes(row[i:j])
        i = j
    return bytes(out)


def do_reader(exe, tmp, listing):
    w, h = 9, 5
    px = (E._hash(w * h * 4, 99) >> np.uint32(24)).astype(np.uint8).reshape(h, w, 4)
    px[..., 3] = 120 + (px[..., 3] % 16)       # exponents around 128: values around 2^-16 ... 2^0
    px[1, :, 3] = 130                          # a row with one exponent: a run across the whole scanline
    px[2, 3:7, :] = [10, 200, 30, 0]           # e = 0: zero, whatever the mantissas
    px[3, 2:8, 0] = 77
    px[0, 0] = [200, 3, 2, 129]                # (a flat file must not begin like a run-length encoded scanline)
    head = b"#?RADIANCE\n# envsky reader fixture\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)
    files = {"flat": head + px.tobytes(),
             "rle": head.replace(b"#?RADIANCE", b"#?RGBE") + b"".join(bytes([2, 2, w >> 8, w & 255]) + b"".join(rle_component(px[j, :, k].tolist()) for k in range(4)) for j in range(h))}
    data = {}
    for kind, blob in files.items():
        path = os.path.join(OUT, f"envsky_reader_{kind}.hdr")
        open(path, "wb").write(blob)
        op = os.path.join(tmp, "hdr.bin")
        subprocess.check_call([exe, "hdr", path, op])
        raw = np.fromfile(op, dtype=np.float32)
        assert tuple(raw[:2].view(np.int32)) == (w, h)
        data[kind] = raw[2:].reshape(h, w, 3)
        listing["reader"][kind] = {"bytes": len(blob), "size": [w, h]}
    assert np.array_equal(data["flat"].view(np.uint32), data["rle"].view(np.uint32))
    np.savez_compressed(os.path.join(OUT, "envsky_reader.npz"), **data)
    print("reader", listing["reader"], flush=True)


def main(what):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    what = what or ["images", "films", "reader"]
    path = os.path.join(OUT, "envsky.json")
    listing = json.load(open(path)) if os.path.exists(path) else {}
    for k in ("images", "films", "reader"):
        listing.setdefault(k, {})
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "images" in what:
            for name in E.IMAGES:
                do_image(exe, tmp, name, listing)
        if "films" in what:
            for name in E.FILMS:
                do_film(exe, tmp, name, listing)
        if "reader" in what:
            do_reader(exe, tmp, listing)
    json.dump(listing, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
