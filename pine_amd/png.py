"""Minimal PNG writer (stands in for stb_image_write, which the reference's save() calls,
src/pine/core/fileio.cpp:55-76).  RGBA8, no filtering.

PNG reader: the bytes the reference's image loaders return for such a file -- (h, w, channels) uint8, rows top first.  PNG is
lossless, so a correct decoder returns exactly what stb_image returns: `channels` = 3 is what the reference's image_from asks
stb for, 4 what tinygltf asks for.  Bit depth 8, colour types 0 (grey), 2 (rgb), 3 (palette, alpha from tRNS), 4 (grey + alpha)
and 6 (rgba), non-interlaced; a tRNS colour key of a grey or rgb image gives alpha 0, as in stb.  Expansion as stb does it: grey
becomes r = g = b, a missing alpha is 255, a dropped alpha is simply dropped.  Refused by name: 16-bit samples, depths below 8,
interlaced images, and every damaged file -- chunk lengths and CRCs, each row's filter byte and the decompressed size are checked.
Inflate is Python's zlib."""
import struct
import zlib

import numpy as np

from ._lib import PineError


def write_png(path, rgba):
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w, c = rgba.shape
    assert c == 4
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def read_png_bytes(data, channels=3, name="<bytes>"):
    def refuse(why):
        raise PineError(f"`{name}` is no PNG image this reader takes ({why})")

    if channels not in (3, 4):
        raise PineError("read_png: channels is 3 or 4")
    data = bytes(data)
    if data[:8] != SIGNATURE:
        refuse("no PNG signature")
    pos, header, palette, trns, idat, ended = 8, None, None, None, [], False
    while not ended:
        if pos + 12 > len(data):
            refuse("truncated: a chunk header or CRC is missing")
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if length > len(data) - pos - 12:
            refuse(f"truncated: chunk {kind!r} is longer than the file")
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(data[pos + 4:pos + 8 + length]) != struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0]:
            refuse(f"bad CRC in chunk {kind!r}")
        pos += 12 + length
        if header is None and kind != b"IHDR":
            refuse("the first chunk is not IHDR")
        if kind == b"IHDR":
            if header is not None or length != 13:
                refuse("bad IHDR")
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            if length == 0 or length % 3 or length > 768:
                refuse("bad PLTE length")
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"tRNS":
            if idat:
                refuse("tRNS after IDAT")
            trns = body
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif not kind[0] & 32:
            refuse(f"unknown critical chunk {kind!r}")
    w, h, depth, ctype, compression, filt, interlace = header
    if w < 1 or h < 1 or w * h > 1 << 26:
        refuse("a size below 1 or more than 2^26 texels")
    if ctype not in _CHANNELS:
        refuse(f"colour type {ctype}")
    if depth == 16:
        refuse("16-bit samples are not supported")
    if depth != 8:
        refuse(f"bit depth {depth}: depths below 8 are not supported")
    if interlace:
        refuse("interlaced images are not supported")
    if compression or filt:
        refuse("unknown compression or filter method")
    if not idat:
        refuse("no IDAT chunk")
    bpp = _CHANNELS[ctype]
    stride = w * bpp
    try:
        d = zlib.decompressobj()
        raw = d.decompress(b"".join(idat), h * (1 + stride) + 1)
        if not d.eof:
            refuse("truncated or oversized IDAT stream")
    except zlib.error as e:
        refuse(f"IDAT does not inflate: {e}")
    if len(raw) != h * (1 + stride):
        refuse(f"IDAT holds {len(raw)} bytes, the image needs {h * (1 + stride)}")
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + stride)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        f = int(rows[y, 0])
        line = rows[y, 1:].astype(np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f in (1, 3, 4):
            cur = line.tolist()
            up = prev.tolist()
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + up[i]) >> 1
                else:
                    b, c = up[i], up[i - bpp] if i >= bpp else 0
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (cur[i] + p) & 255
            cur = np.array(cur, np.int32)
        else:
            refuse(f"row {y} has filter type {f}")
        out[y] = cur
        prev = cur
    px = out.reshape(h, w, bpp)
    alpha = np.full((h, w, 1), 255, np.uint8)
    if ctype == 3:
        if palette is None:
            refuse("a palette image without PLTE")
        if int(px.max()) >= len(palette):
            refuse("a palette index past the end of PLTE")
        rgb = palette[px[..., 0]]
        if trns is not None:
            if len(trns) > len(palette):
                refuse("tRNS is longer than PLTE")
            table = np.full(256, 255, np.uint8)
            table[:len(trns)] = np.frombuffer(trns, np.uint8)
            alpha = table[px[..., 0]][..., None]
    elif ctype in (0, 4):
        rgb = np.repeat(px[..., :1], 3, axis=2)
        if ctype == 4:
            alpha = px[..., 1:2]
        elif trns is not None:
            if len(trns) != 2:
                refuse("bad tRNS length")
            alpha = np.where(px[..., :1] == (struct.unpack(">H", trns)[0] & 255), 0, 255).astype(np.uint8)
    else:
        rgb = px[..., :3]
        if ctype == 6:
            alpha = px[..., 3:4]
        elif trns is not None:
            if len(trns) != 6:
                refuse("bad tRNS length")
            key = np.array([v & 255 for v in struct.unpack(">HHH", trns)], np.uint8)
            alpha = np.where((rgb == key).all(axis=2, keepdims=True), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(rgb if channels == 3 else np.concatenate([rgb, alpha], axis=2), dtype=np.uint8)


def read_png(path, channels=3):
    with open(path, "rb") as f:
        return read_png_bytes(f.read(), channels, str(path))
