"""glTF materials with image textures: tests/golden/textured_quad.glb (tools/make_texture_glb.py) through pine_amd/gltf.py and
through pine_amd/host/gltf_import.hpp builds the scene whose film the real reference's own importer rendered
(tools/make_golden_texture.py glb; the film is compared on the device, tests/test_texture_gpu.py); other image formats are
refused by name."""
import base64
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import texture_scenes as X
from test_envsky import _Lazy, pa

gltf = _Lazy("pine_amd.gltf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GLB = os.path.join(GOLDEN, "textured_quad.glb")
NAME = "tex_glb_40x30_s4_d3"


def fixture_pscene():
    return bytes(np.load(os.path.join(GOLDEN, f"texture_film_{NAME}.npz"))["pscene"]).decode()


def test_python_import_builds_the_fixtures_scene():
    ps = X.glb_scene(gltf, GLB, X.GLB_FILMS[NAME][0]).describe()
    assert ps == fixture_pscene()
    lines = ps.splitlines()
    assert sum(ln.startswith("image ") for ln in lines) == 3 and all(ln.split()[4] == "u8x4" for ln in lines if ln.startswith("image "))
    assert sum(" image " in ln for ln in lines if ln.startswith("node ")) == 6  # one NodeImage per use, three images stored once
    # a roughnessFactor beside a metallicRoughnessTexture wins over the texture's roughness; the metallic stays the texture's
    rough = [ln.split() for ln in lines if ln.startswith("material ")][3]
    kinds = {int(ln.split()[1]): ln.split()[2] for ln in lines if ln.startswith("node ")}
    assert kinds[int(rough[4])] == "constf" and kinds[int(rough[5])] == "comp"


def test_cpp_import_builds_the_same_scene(tmp_path):
    """pine::load of the C++ facade (pine_amd/host/gltf_import.hpp, png_read.hpp): the same scene, line for line."""
    src = tmp_path / "t.cpp"
    src.write_text('#include "%s/pine_amd/host/pine.hpp"\n#include <cstdio>\n#include <vector>\n'
                   'int main(int, char** argv) {\n  pine::Scene s;\n'
                   '  try { pine::load(s, argv[1]); } catch (const std::exception& e) { std::fprintf(stderr, "%%s", e.what()); return 4; }\n'
                   '  std::vector<char> buf(1 << 20);\n  int n = pine_gpu_scene_describe(s.handle(), buf.data(), int(buf.size()));\n'
                   '  if (n < 0) return 2;\n  std::fwrite(buf.data(), 1, size_t(n), stdout);\n  return 0;\n}\n' % ROOT)
    exe = tmp_path / "t"
    lib = os.path.join(ROOT, "pine_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O0", str(src), "-o", str(exe), "-L" + lib, "-lpine_gpu", "-Wl,-rpath," + lib], check=True)
    r = subprocess.run([str(exe), GLB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.rstrip("\x00") == gltf.load(GLB).describe()
    jpeg = tmp_path / "jpeg.glb"
    jpeg.write_bytes(_with_first_image(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(40), "image/jpeg"))
    r = subprocess.run([str(exe), str(jpeg)], capture_output=True, text=True)
    assert r.returncode == 4 and "is a JPEG: not supported" in r.stderr, r.stderr


def _with_first_image(data, mime):
    """textured_quad.glb with its first image replaced by `data` in a data URI."""
    blob = open(GLB, "rb").read()
    n = struct.unpack("<I", blob[12:16])[0]
    doc = json.loads(blob[20:20 + n])
    doc["images"][0] = {"uri": f"data:{mime};base64," + base64.b64encode(data).decode(), "name": "swapped"}
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    rest = blob[20 + n:]
    return struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + len(rest)) + struct.pack("<II", len(js), 0x4E4F534A) + js + rest


def test_other_image_formats_are_refused_by_name(tmp_path):
    p = tmp_path / "jpeg.glb"
    p.write_bytes(_with_first_image(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(40), "image/jpeg"))
    with pytest.raises(pa.PineError, match="`swapped` is a JPEG: not supported"):
        gltf.load(str(p))
    p.write_bytes(_with_first_image(b"GIF89a" + bytes(40), "image/gif"))
    with pytest.raises(pa.PineError, match="`swapped` is not a PNG: not supported"):
        gltf.load(str(p))
    p.write_bytes(_with_first_image(open(os.path.join(GOLDEN, "texture_png_refused_interlaced.png"), "rb").read(), "image/png"))
    with pytest.raises(pa.PineError, match="interlaced"):
        gltf.load(str(p))


def test_an_image_file_beside_the_document(tmp_path):
    """A .gltf whose image is a file next to it: the same scene as the binary form."""
    blob = open(GLB, "rb").read()
    n = struct.unpack("<I", blob[12:16])[0]
    doc = json.loads(blob[20:20 + n])
    binary = blob[20 + n + 8:]
    view = doc["bufferViews"][doc["images"][0]["bufferView"]]
    (tmp_path / "first.png").write_bytes(binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]])
    doc["images"][0] = {"uri": "first.png"}
    doc["buffers"][0]["uri"] = "data.bin"
    (tmp_path / "data.bin").write_bytes(binary)
    (tmp_path / "scene.gltf").write_text(json.dumps(doc))
    assert gltf.load(str(tmp_path / "scene.gltf")).describe() == gltf.load(GLB).describe()
