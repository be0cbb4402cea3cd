"""The PNG readers (pine_amd/png.py, pine_amd/host/png_read.hpp) against what the reference's own loaders returned for six small
files (tools/make_golden_texture.py: stb through image_from in 3 channels, tinygltf's loader in 4), the four refusals, and the
C++ reader -- a stand-alone program built with the address and undefined-behaviour sanitizers -- over seeded mutations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_envsky import _Lazy, pa  # (imported at first use: a GPU run imports torch first)

png = _Lazy("pine_amd.png")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOOD = ("grey", "rgb", "palette", "palette_trns", "grey_alpha", "rgba")
REFUSED = {"refused_16bit": "16-bit", "refused_interlaced": "interlaced", "refused_crc": "bad CRC", "refused_truncated": "truncated"}
MUTATIONS = 2000


def path_of(name):
    return os.path.join(GOLDEN, f"texture_png_{name}.png")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "texture_png.npz"))


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name", GOOD)
def test_python_reader_returns_the_references_bytes(name, channels, golden):
    got = png.read_png(path_of(name), channels)
    assert got.dtype == np.uint8 and np.array_equal(got, golden[f"{name}_{channels}"])


def test_every_filter_type_occurs_in_every_file():
    import struct
    import zlib
    for name in GOOD:
        data, pos, idat, header = open(path_of(name), "rb").read(), 8, b"", None
        while pos < len(data):
            n, kind = struct.unpack(">I4s", data[pos:pos + 8])
            if kind == b"IHDR":
                header = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
            if kind == b"IDAT":
                idat += data[pos + 8:pos + 8 + n]
            pos += 12 + n
        raw = zlib.decompress(idat)
        w, h, _, ctype = header[:4]
        stride = 1 + w * {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
        assert {raw[y * stride] for y in range(h)} == {0, 1, 2, 3, 4}, name


@pytest.mark.parametrize("name", list(REFUSED))
def test_python_reader_refuses(name):
    with pytest.raises(pa.PineError, match=REFUSED[name]):
        png.read_png(path_of(name))


def test_python_reader_refuses_other_formats():
    with pytest.raises(pa.PineError, match="no PNG signature"):
        png.read_png_bytes(b"\xff\xd8\xff\xe0" + bytes(64))
    with pytest.raises(pa.PineError, match="depths below 8"):
        data = bytearray(open(path_of("grey"), "rb").read())
        import struct
        import zlib
        data[24] = 4  # IHDR's bit depth, with the chunk's CRC made right again
        data[29:33] = struct.pack(">I", zlib.crc32(bytes(data[12:29])))
        png.read_png_bytes(bytes(data))


def mutations(tmp_path):
    """MUTATIONS files: single-byte changes and truncations of the ten fixture files, seeded."""
    files = [open(path_of(n), "rb").read() for n in GOOD + tuple(REFUSED)]
    x = 0x9e3779b97f4a7c15
    out = []
    for i in range(MUTATIONS):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        r = x >> 16
        blob = bytearray(files[i % len(files)])
        at = (r >> 8) % len(blob)
        if i % 4 == 3:
            blob = blob[:at]
        else:
            blob[at] ^= 1 + (r & 0xff) % 255
        p = tmp_path / f"m{i}.png"
        p.write_bytes(bytes(blob))
        out.append((str(p), bytes(blob)))
    return out


def python_answer(blob, channels):
    try:
        a = png.read_png_bytes(blob, channels)
        return f"ok {a.shape[1]} {a.shape[0]} {a.tobytes().hex()}"
    except pa.PineError:
        return "refused"


def test_cpp_reader_under_sanitizers(tmp_path):
    """Nothing is loaded into Python: png_read.hpp is compiled into an executable of its own with the sanitizers and run as a child."""
    cxx = shutil.which("g++")
    exe = tmp_path / "png_read_main"
    if cxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (the sanitizers' runtimes linked into the executable itself: it needs nothing preloaded, whatever else the loader brings)
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    if subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler cannot link with -fsanitize")
    subprocess.check_call([cxx, *flags, "-Wall", os.path.join(ROOT, "tools", "png_read_main.cpp"), "-o", str(exe)])
    cases = [(path_of(n), open(path_of(n), "rb").read()) for n in GOOD + tuple(REFUSED)] + mutations(tmp_path)
    listing = tmp_path / "list.txt"
    listing.write_text("\n".join(p for p, _ in cases) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for channels in (3, 4):
        run = subprocess.run([str(exe), str(channels), str(listing)], capture_output=True, text=True, env=env, timeout=120)
        assert run.returncode == 0 and "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
        lines = run.stdout.splitlines()
        assert len(lines) == len(cases)
        for i, ((path, blob), line) in enumerate(zip(cases, lines)):
            want = python_answer(blob, channels)
            if i < len(GOOD):
                assert want.startswith("ok ") and line == want, path
            elif i < len(GOOD) + len(REFUSED):
                assert line.startswith("refused ") and list(REFUSED.values())[i - len(GOOD)] in line, (path, line)
            else:  # a mutation: every one of them damages a checked field, so both readers refuse
                assert line.startswith("refused ") and want == "refused", (path, line[:200], want[:40])
