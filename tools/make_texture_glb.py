"""Writes tests/golden/textured_quad.glb: a small binary glTF whose materials carry image textures, as the reference's importer
reads them (src/pine/core/fileio.cpp:150-160, 278-293): three textured quads -- a baseColorTexture from an RGB PNG in a buffer
view, one from a palette PNG in a data URI, a metallicRoughnessTexture from an RGBA PNG (beside a roughnessFactor, which the
importer applies after the texture: it walks the material's parameters in name order) -- one untextured emissive quad, a floor
that shares the first image, and a camera node.  Texture coordinates leave [0, 1]; samplers are present and ignored.  The PNG
files are written by tools/make_golden_texture.py's png_file with every filter type.  The file is DATA (a fixture);
tools/make_golden_texture.py glb renders it with the reference."""
import base64
import json
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import texture_scenes as X  # noqa: E402
from make_golden_texture import png_file  # noqa: E402


def images():
    """(rgb png, palette png, rgba png) bytes."""
    rgb = X.image("ramp8_16x16")
    v = (X._hash(12 * 10, 91) >> np.uint32(24)).astype(np.uint8).reshape(10, 12, 1)
    palette = (X._hash(6 * 3, 92) >> np.uint32(24)).astype(np.uint8).reshape(6, 3)
    rgba = (X._hash(8 * 8 * 4, 93) >> np.uint32(24)).astype(np.uint8).reshape(8, 8, 4)
    return png_file(rgb, 2, 0), png_file(v % 6, 3, 1, palette=palette), png_file(rgba, 6, 3)


def main(out):
    blob = bytearray()
    views, accessors = [], []

    def view(data):
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)})
        blob.extend(data)
        return len(views) - 1

    def add(arr, kind, ctype):
        accessors.append({"bufferView": view(arr.tobytes()), "componentType": ctype, "count": len(arr) if kind != "SCALAR" else arr.size, "type": kind})
        if kind == "VEC3":
            accessors[-1]["min"], accessors[-1]["max"] = arr.min(axis=0).tolist(), arr.max(axis=0).tolist()
        return len(accessors) - 1

    meshes = []

    def quad(p0, ex, ey, material, uv0=(0.0, 0.0), uv1=(1.0, 1.0)):
        p0, ex, ey = map(np.float32, (p0, ex, ey))
        v = np.float32([p0, p0 + ex, p0 + ex + ey, p0 + ey])
        t = np.float32([[uv0[0], uv0[1]], [uv1[0], uv0[1]], [uv1[0], uv1[1]], [uv0[0], uv1[1]]])
        attrs = {"POSITION": add(v, "VEC3", 5126), "TEXCOORD_0": add(t, "VEC2", 5126)}
        meshes.append({"primitives": [{"attributes": attrs, "indices": add(np.uint16([0, 1, 2, 0, 2, 3]), "SCALAR", 5123), "material": material, "mode": 4}]})
        return len(meshes) - 1

    rgb, pal, rgba = images()
    gl_images = [{"bufferView": view(rgb), "mimeType": "image/png"},
                 {"uri": "data:image/png;base64," + base64.b64encode(pal).decode()},
                 {"bufferView": view(rgba), "mimeType": "image/png"}]
    textures = [{"source": 0, "sampler": 0}, {"source": 1}, {"source": 2, "sampler": 0}]
    materials = [
        {"name": "rgb", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.3, 0.4, 1.0], "baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 0.8}},
        {"name": "palette", "pbrMetallicRoughness": {"baseColorTexture": {"index": 1, "texCoord": 0}, "metallicFactor": 0.0, "roughnessFactor": 0.6}},
        {"name": "rough", "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.6, 1.0], "metallicRoughnessTexture": {"index": 2}, "roughnessFactor": 0.35}},
        {"name": "lamp", "emissiveFactor": [1.0, 0.95, 0.8], "pbrMetallicRoughness": {"metallicFactor": 0.0},
         "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 14.0}}},
        {"name": "shiny", "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.8, 0.6, 1.0], "metallicRoughnessTexture": {"index": 2}}},
    ]
    nodes = [
        {"name": "floor", "mesh": quad([-2, 0, -2], [0, 0, 4], [4, 0, 0], 0, (-1.0, -0.5), (2.0, 1.5))},
        {"name": "left", "mesh": quad([-1.9, 0.2, 1.0], [1.2, 0, 0.3], [0, 1.5, 0], 0)},
        {"name": "middle", "mesh": quad([-0.6, 0.2, 1.3], [1.2, 0, 0], [0, 1.5, 0], 1, (-0.25, 0.0), (1.25, 2.0))},
        {"name": "right", "mesh": quad([0.7, 0.2, 1.3], [1.2, 0, -0.3], [0, 1.5, 0], 2)},
        {"name": "back", "mesh": quad([-2, 0, 2], [4, 0, 0], [0, 3, 0], 4, (0.0, 0.0), (3.0, 2.0))},
        {"name": "lamp", "mesh": quad([-0.6, 2.8, -0.6], [1.2, 0, 0], [0, 0, 1.2], 3), "translation": [0.0, 0.1, 0.2]},
        {"name": "camera", "camera": 0, "translation": [0.0, 1.2, -3.6], "rotation": [0.0, 1.0, 0.0, 0.0]},
    ]
    doc = {"asset": {"version": "2.0", "generator": "pine-mi355x tools/make_texture_glb.py"}, "scene": 0, "scenes": [{"nodes": list(range(len(nodes)))}],
           "nodes": nodes, "meshes": meshes, "materials": materials, "textures": textures, "images": gl_images,
           "samplers": [{"magFilter": 9729, "minFilter": 9987, "wrapS": 33071, "wrapT": 33648}],
           "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob)}],
           "cameras": [{"type": "perspective", "perspective": {"yfov": 0.8, "aspectRatio": 4.0 / 3.0, "znear": 0.1}}],
           "extensionsUsed": ["KHR_materials_emissive_strength"]}
    while len(blob) % 4:
        blob.append(0)
    doc["buffers"][0]["byteLength"] = len(blob)
    js = json.dumps(doc, separators=(",", ":")).encode()
    js += b" " * (-len(js) % 4)
    with open(out, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(blob)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(blob), 0x004E4942) + bytes(blob))
    print(out, 12 + 16 + len(js) + len(blob), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "textured_quad.glb"))
