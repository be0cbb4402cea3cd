"""Radiance HDR (.hdr / RGBE) reader: what the reference's image loader (stb's stbi_loadf, 3 channels) returns for such a
file -- (h, w, 3) float32, rows top first.  `#?RADIANCE` / `#?RGBE` headers, FORMAT=32-bit_rle_rgbe, `-Y h +X w` only, flat and
new-style run-length encoded scanlines.  Anything else is refused by name: there is no PNG / JPEG decoder in this package."""
import numpy as np

from ._lib import PineError


def _convert(rgbe):
    """(n, 4) uint8 -> (n, 3) float32: mantissa * ldexp(1, e - 136), zero where e = 0."""
    e = rgbe[:, 3].astype(np.int32)
    f = np.ldexp(np.float32(1.0), e - 136).astype(np.float32)
    out = rgbe[:, :3].astype(np.float32) * f[:, None]
    out[e == 0] = 0.0
    return out


def read_hdr_bytes(data, name="<bytes>"):
    def refuse(why):
        raise PineError(f"`{name}` is no Radiance HDR image this reader takes ({why}); other image formats enter as arrays")

    pos = 0

    def line():
        nonlocal pos
        end = data.find(b"\n", pos)
        if end < 0:
            refuse("truncated header")
        s = data[pos:end]
        pos = end + 1
        return s

    if line() not in (b"#?RADIANCE", b"#?RGBE"):
        refuse("no #?RADIANCE / #?RGBE signature")
    fmt_ok = False
    while True:
        s = line()
        if not s:
            break
        if s == b"FORMAT=32-bit_rle_rgbe":
            fmt_ok = True
    if not fmt_ok:
        refuse("FORMAT is not 32-bit_rle_rgbe")
    tok = line().split()
    if len(tok) != 4 or tok[0] != b"-Y" or tok[2] != b"+X":
        refuse("orientation is not -Y h +X w")
    h, w = int(tok[1]), int(tok[3])
    if h < 1 or w < 1:
        refuse("empty image")
    buf = np.frombuffer(data, dtype=np.uint8)

    def flat():
        if pos + 4 * w * h > len(data):
            refuse("truncated pixels")
        return _convert(buf[pos:pos + 4 * w * h].reshape(-1, 4)).reshape(h, w, 3)

    if w < 8 or w >= 32768:
        return flat()
    rows = np.zeros((h, w, 4), dtype=np.uint8)
    for j in range(h):
        if pos + 4 > len(data):
            refuse("truncated pixels")
        c1, c2, hi, lo = data[pos:pos + 4]
        if c1 != 2 or c2 != 2 or (hi & 0x80):
            if j == 0:
                return flat()  # not run-length encoded: the four bytes were the first pixel
            refuse("a scanline that is not run-length encoded after one that is")
        pos += 4
        if (hi << 8 | lo) != w:
            refuse("scanline width")
        for k in range(4):
            i = 0
            while i < w:
                if pos >= len(data):
                    refuse("truncated pixels")
                count = data[pos]
                pos += 1
                if count > 128:
                    count -= 128
                    if count == 0 or count > w - i or pos >= len(data):
                        refuse("corrupt run")
                    rows[j, i:i + count, k] = data[pos]
                    pos += 1
                else:
                    if count == 0 or count > w - i or pos + count > len(data):
                        refuse("corrupt run")
                    rows[j, i:i + count, k] = buf[pos:pos + count]
                    pos += count
                i += count
    return _convert(rows.reshape(-1, 4)).reshape(h, w, 3)


def read_hdr(path):
    with open(path, "rb") as f:
        return read_hdr_bytes(f.read(), str(path))
