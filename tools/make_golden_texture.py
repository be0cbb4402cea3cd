#!/usr/bin/env python3
"""Generate tests/golden/texture_*.npz and texture.json from the REAL reference's NodeImage / NodeImagef.

Runs only where the reference's sources are: tools/ref_texture_driver.cpp is compiled in place against them, together with the
reference's impl/integrator/denoiser.cpp read from where it lies, and linked with oracle/_ref/libpine_ref.a (make -C oracle
ref).  The binary goes to a scratch directory; nothing of the reference is copied into this tree.  No test calls this tool:
the tests read what it wrote.

    python tools/make_golden_texture.py [calls] [films] [png] [glb]

calls: the scene texture_zoo (tests/texture_scenes.py) -- every program over the six images, then its constant twins -- at
512 queries: the reference's 10-float record per material and query.  films: the room scene's film and its albedo / normal
guide pair, with the .pscene text.  png: six small PNG files written here with hand-chosen filter types (all five occur in each),
one per supported colour type plus a palette with tRNS, with the bytes the reference's image_from returns for each (3 channels)
and the bytes tinygltf's loader returns (4 channels); and four files a reader must refuse: 16-bit, interlaced, a bad CRC, a
truncated IDAT stream.  glb: tests/golden/textured_quad.glb (tools/make_texture_glb.py) through the reference's OWN importer,
rendered on a 40 x 30 film; the fixture keeps the film and the .pscene text of this package's import of the same file.

Asserted here, on the inputs and with the reference alone: no query has a coordinate that is not finite; the driver flags no
read outside an image; per image at least min(texels, 30) distinct texels are read; per image with a side above 1 at least 8
lookups take the clamp on that side (vec2i(size * fract) == size before the min); in the film the camera ray through the centre
of at least 25 % of the pixels meets a textured surface first (counted by the driver with the reference's BVH); the film has at
least 100 distinct pixel values.
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
import texture_scenes as X  # noqa: E402

REF_SRC = os.environ.get("PINE_REF_SRC", "/root/reference/src")
ARCHIVE = os.path.join(ROOT, "oracle", "_ref", "libpine_ref.a")
OUT = os.path.join(ROOT, "tests", "golden")
FRONT = ("image ", "node ", "material ")


def build_driver(tmp):
    exe = os.path.join(tmp, "ref_texture_driver")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-w", "-DNDEBUG", "-I" + REF_SRC, "-I" + REF_SRC + "/contrib",
                           os.path.join(ROOT, "tools", "ref_texture_driver.cpp"), os.path.join(REF_SRC, "pine", "impl", "integrator", "denoiser.cpp"),
                           "-o", exe, ARCHIVE, "-pthread", "-Wl,--unresolved-symbols=ignore-all"])
    return exe


def split_scene(tmp, ps, texels):
    """The .pscene text as the driver's two files, and the texels of image i as image_<i>.bin."""
    lines = [ln for ln in ps.splitlines() if ln and not ln.startswith("#")]
    fp, rp = os.path.join(tmp, "front.txt"), os.path.join(tmp, "rest.pscene")
    open(fp, "w").write("\n".join(ln for ln in lines if ln.startswith(FRONT)) + "\n")
    open(rp, "w").write("\n".join(ln for ln in lines if not ln.startswith(FRONT)) + "\n")
    n = sum(ln.startswith("image ") for ln in lines)
    assert n == len(texels), (n, len(texels))
    for i, t in enumerate(texels):
        t.tofile(os.path.join(tmp, f"image_{i}.bin"))
    return fp, rp


def do_calls(exe, tmp, listing):
    q = X.queries()
    assert np.isfinite(q).all(), "a query is not finite"
    sc, mats = X.texture_zoo(q)
    names = list(X.IMAGES)
    fp, _ = split_scene(tmp, sc.describe(), [X.image(n) for n in names])  # (the zoo adds its images in IMAGES order)
    qp, rp, lp = (os.path.join(tmp, x) for x in ("q.bin", "r.bin", "l.bin"))
    q.tofile(qp)
    print(subprocess.check_output([exe, "calls", tmp, fp, qp, rp, lp]).decode().strip(), flush=True)
    rec = np.fromfile(rp, dtype=np.float32).reshape(len(mats), len(q), 10)
    look = np.fromfile(lp, dtype=np.int32).reshape(-1, len(q), 4)
    assert not look[..., 3].any(), f"{int(look[..., 3].sum())} lookups read outside an image or have a coordinate that is not finite"
    # (the counts below are of the programs that read the surface: a twin's lookup is one lookup, whatever the query)
    look = look[:X.texture_zoo(q, twins=False)[0].describe().count(" image")]
    entry = {}
    for i, name in enumerate(names):
        w, h, _ = X.IMAGES[name]
        mine = look[look[:, 0, 0] == i].reshape(-1, 4)
        texels = len({(min(int(x), w - 1), min(int(y), h - 1)) for _, x, y, _ in mine})
        clamp_x, clamp_y = int((mine[:, 1] == w).sum()), int((mine[:, 2] == h).sum())
        assert texels >= min(w * h, 30), f"{name}: only {texels} distinct texels read"
        assert w == 1 or clamp_x >= 8, f"{name}: only {clamp_x} lookups take the clamp in x"
        assert h == 1 or clamp_y >= 8, f"{name}: only {clamp_y} lookups take the clamp in y"
        assert (mine[:, 1] <= w).all() and (mine[:, 2] <= h).all() and (mine[:, 1:3] >= 0).all()
        entry[name] = {"size": [w, h], "distinct_texels": texels, "clamped_x": clamp_x, "clamped_y": clamp_y, "lookups": int(len(mine))}
    ps = sc.describe()
    np.savez_compressed(os.path.join(OUT, "texture_zoo.npz"), queries=q, records=rec, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["calls"] = {"materials": len(mats), "queries": len(q), "images": entry}
    print("calls", listing["calls"], os.path.getsize(os.path.join(OUT, "texture_zoo.npz")), "bytes", flush=True)


def do_films(exe, tmp, listing):
    room_images = [X.image(n) for n in ("ramp8_16x16", "rgba8_7x4", "f32_3x5")]
    for key, fname in X.SCRIPT_PNGS.items():  # the PNG files examples/textured.pine loads (the RGBA one keeps its alpha in the file)
        open(os.path.join(OUT, fname), "wb").write(png_file(X.image(key), 2 if X.IMAGES[key][2] == "u8x3" else 6, 1))
    for name, (size, spp, depth) in X.FILMS.items():
        w, h = size
        scene = X.film_scene(name)
        ps = scene.describe()
        fp, rp = split_scene(tmp, ps, X.film_images(name))
        op, hp = os.path.join(tmp, "s.film"), os.path.join(tmp, "s.first")
        subprocess.check_call([exe, "film", tmp, fp, rp, str(spp), str(depth), op, hp])
        film = np.fromfile(op, dtype=np.float32).reshape(h, w, 4)
        first = np.fromfile(hp, dtype=np.uint8)
        order = [ln.split()[1] for ln in ps.splitlines() if ln.startswith("material ")]
        textured = float(np.isin(first, [1 + order.index(m) for m in X.TEXTURED + ("chrome",) if m in order]).mean())
        distinct = len(np.unique(film.reshape(-1, 4).view(np.uint32), axis=0))
        assert np.isfinite(film).all()
        assert textured >= 0.25, f"{name}: only {textured:.3f} of the centre camera rays meet a textured surface first"
        assert distinct >= 100, f"{name}: only {distinct} distinct pixel values"
        np.savez_compressed(os.path.join(OUT, f"texture_film_{name}.npz"), film=film, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
        listing["films"][name] = {"size": [w, h], "spp": spp, "depth": depth, "centre_rays_on_textures": round(textured, 4), "distinct_pixels": distinct,
                                  "mean": float(film[..., :3].mean(dtype=np.float64))}
        print(name, listing["films"][name], os.path.getsize(os.path.join(OUT, f"texture_film_{name}.npz")), "bytes", flush=True)
    w, h = X.GUIDES_SIZE
    ps = X.room(X.GUIDES_SIZE).describe()
    fp, rp = split_scene(tmp, ps, room_images)
    ap, np_ = os.path.join(tmp, "g.albedo"), os.path.join(tmp, "g.normal")
    subprocess.check_call([exe, "guides", tmp, fp, rp, ap, np_])
    albedo = np.fromfile(ap, dtype=np.float32).reshape(h, w, 3)
    normal = np.fromfile(np_, dtype=np.float32).reshape(h, w, 3)
    distinct = len(np.unique(albedo.reshape(-1, 3).view(np.uint32), axis=0))
    assert distinct >= 100, f"guides: only {distinct} distinct albedo values"
    np.savez_compressed(os.path.join(OUT, "texture_guides_room.npz"), albedo=albedo, normal=normal, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["guides"] = {"size": [w, h], "distinct_albedo": distinct}
    print("guides", listing["guides"], flush=True)


def png_chunk(kind, body):
    import struct
    import zlib
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(px, ctype, first_filter, palette=None, trns=None, depth=8, interlace=0, cut=0):
    """px (h, w, c) uint8 -> the file, row y filtered with type (first_filter + y) % 5; cut: bytes taken off the IDAT stream."""
    import struct
    import zlib
    h, w, c = px.shape
    bpp = c * depth // 8
    rows = px.reshape(h, w * c).astype(np.int32)
    if depth == 16:
        rows = np.repeat(rows, 2, axis=1)
    raw, prev = bytearray(), np.zeros(rows.shape[1], np.int32)
    for y in range(h):
        f, cur = (first_filter + y) % 5, rows[y]
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        cc = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        pa, pb, pc = abs(prev - cc), abs(a - cc), abs(a + prev - 2 * cc)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, cc))
        pred = [0, a, prev, (a + prev) >> 1, paeth][f]
        raw += bytes([f]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    stream = zlib.compress(bytes(raw), 9)
    stream = stream[:len(stream) - cut]
    out = b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if palette is not None:
        out += png_chunk(b"PLTE", palette.tobytes())
    if trns is not None:
        out += png_chunk(b"tRNS", bytes(trns))
    half = len(stream) // 2  # two IDAT chunks: a reader joins them
    return out + png_chunk(b"IDAT", stream[:half]) + png_chunk(b"IDAT", stream[half:]) + png_chunk(b"tEXt", b"Comment\0texture fixture") + png_chunk(b"IEND", b"")


def png_fixtures():
    """name -> file bytes: the six good files, then the four refused ones."""
    w, h = 9, 7
    v = (X._hash(w * h * 4, 77) >> np.uint32(24)).astype(np.uint8).reshape(h, w, 4)
    v[2, :, :] = v[2, 0, :]  # a constant row: long zero runs under Sub
    palette = (X._hash(13 * 3, 78) >> np.uint32(24)).astype(np.uint8).reshape(13, 3)
    index = (v[..., :1] % 13).astype(np.uint8)
    good = {
        "grey": png_file(v[..., :1], 0, 0),
        "rgb": png_file(v[..., :3], 2, 1),
        "palette": png_file(index, 3, 2, palette=palette),
        "palette_trns": png_file(index, 3, 3, palette=palette, trns=[0, 255, 17, 128, 200, 1, 254]),
        "grey_alpha": png_file(v[..., :2], 4, 4),
        "rgba": png_file(v, 6, 2),
    }
    crc = bytearray(good["rgb"])
    crc[bytes(crc).rindex(b"IDAT") + 6] ^= 0x10  # a byte of the second IDAT chunk's data: its CRC no longer matches
    bad = {
        "refused_16bit": png_file(v[..., :3], 2, 0, depth=16),
        "refused_interlaced": png_file(v[..., :3], 2, 0, interlace=1),
        "refused_crc": bytes(crc),
        "refused_truncated": png_file(v[..., :3], 2, 1, cut=9),
    }
    return good, bad


def do_png(exe, tmp, listing):
    good, bad = png_fixtures()
    data = {}
    listing["png"] = {}
    for name, blob in {**good, **bad}.items():
        open(os.path.join(OUT, f"texture_png_{name}.png"), "wb").write(blob)
        listing["png"][name] = {"bytes": len(blob)}
    for name, blob in good.items():
        op = os.path.join(tmp, "png.bin")
        subprocess.check_call([exe, "png", os.path.join(OUT, f"texture_png_{name}.png"), op])
        raw = np.fromfile(op, dtype=np.uint8)
        w, h = (int(x) for x in raw[:8].view(np.int32))
        assert (w, h) == (9, 7) and len(raw) == 8 + w * h * 7
        data[name + "_3"] = raw[8:8 + w * h * 3].reshape(h, w, 3)
        data[name + "_4"] = raw[8 + w * h * 3:].reshape(h, w, 4)
        assert np.array_equal(data[name + "_3"], data[name + "_4"][..., :3])
    assert len({data[k].tobytes() for k in data if k.endswith("_3")}) == 3  # (grey, rgb, palette: each twice, with and without alpha)
    assert not (data["palette_trns_4"][..., 3] == 255).all() and (data["palette_4"][..., 3] == 255).all()
    np.savez_compressed(os.path.join(OUT, "texture_png.npz"), **data)
    print("png", listing["png"], flush=True)


def do_glb(exe, tmp, listing):
    from pine_amd import gltf
    glb = os.path.join(OUT, "textured_quad.glb")
    name, (size, spp, depth) = next(iter(X.GLB_FILMS.items()))
    w, h = size
    op, hp = os.path.join(tmp, "g.film"), os.path.join(tmp, "g.first")
    subprocess.check_call([exe, "glb", glb, str(w), str(h), str(spp), str(depth), op, hp])
    film = np.fromfile(op, dtype=np.float32).reshape(h, w, 4)
    first = np.fromfile(hp, dtype=np.uint8)
    ps = X.glb_scene(gltf, glb, size).describe()
    shapes = [ln.split()[2] for ln in ps.splitlines() if ln.startswith("shape ")]
    lamps = {ln.split()[1] for ln in ps.splitlines() if ln.startswith("material ") and ln.split()[2] == "emissive"}
    textured = float(np.isin(first, [1 + i for i, m in enumerate(shapes) if m not in lamps]).mean())
    distinct = len(np.unique(film.reshape(-1, 4).view(np.uint32), axis=0))
    assert np.isfinite(film).all()
    assert textured >= 0.25, f"{name}: only {textured:.3f} of the centre camera rays meet a textured surface first"
    assert distinct >= 100, f"{name}: only {distinct} distinct pixel values"
    np.savez_compressed(os.path.join(OUT, f"texture_film_{name}.npz"), film=film, pscene=np.frombuffer(ps.encode(), dtype=np.uint8))
    listing["films"][name] = {"size": [w, h], "spp": spp, "depth": depth, "centre_rays_on_textures": round(textured, 4), "distinct_pixels": distinct,
                              "mean": float(film[..., :3].mean(dtype=np.float64))}
    print(name, listing["films"][name], flush=True)


def main(what):
    if not os.path.isdir(REF_SRC) or not os.path.exists(ARCHIVE):
        sys.exit("the reference's sources and oracle/_ref/libpine_ref.a (make -C oracle ref) are needed")
    what = what or ["calls", "films", "png", "glb"]
    path = os.path.join(OUT, "texture.json")
    listing = json.load(open(path)) if os.path.exists(path) else {}
    listing.setdefault("films", {})
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        if "calls" in what:
            do_calls(exe, tmp, listing)
        if "films" in what:
            do_films(exe, tmp, listing)
        if "png" in what:
            do_png(exe, tmp, listing)
        if "glb" in what:
            do_glb(exe, tmp, listing)
    json.dump(listing, open(path, "w"), indent=1, sort_keys=True)
    open(path, "a").write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
