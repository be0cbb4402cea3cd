"""The scenes of the Accel ray-query fixtures (tests/golden/accel_<scene>_<bvh|embree>.npz, written by tools/make_golden_accel.py
from the real reference's Accel::intersect / Accel::hit) and the helpers tests/test_accel.py and tests/test_accel_gpu.py share."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
NUM_RAYS = 1000
ORDERS = ("bvh", "embree")
# scene: the seed of its rays (tools/make_golden.py bvh_rays; the bvh_*.npz fixtures use 77 ... 82)
SEEDS = {"cbox": 4101, "zoo": 4102, "xshapes": 4103, "sss_mesh": 4104, "mesh_attrs": 4105}
# the scenes that tests/golden/bvh_<name>.npz describes too (`pine_ref bvh`: another run of the reference, other rays)
SAME_AS_BVH_FIXTURE = {"cbox": "cbox", "zoo": "zoo", "sss_mesh": "sss_mesh"}
CROSS_RAYS = 250  # of that fixture's rays, answered by the accel driver too (accel_<scene>_bvh.npz: cross_records, cross_occluded)


def mesh_attrs_scene(size=(48, 48)):
    """The Rect room of the Subsurface scene around one icosphere that carries per-vertex normals and texcoords: the
    interaction's n is interpolated and its uv are texcoords (geometry.h:195-212)."""
    import pine_amd as pa
    from pine_amd import scenes
    s = pa.Scene()
    s.add("floor", pa.Diffuse([0.9, 0.9, 0.9]))
    s.add("red", pa.Diffuse([0.9, 0.1, 0.05]))
    s.add("ball", pa.Glossy([0.9, 0.5, 0.3], 0.15))
    s.add(pa.Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], True), "floor")
    s.add(pa.Rect([0, 2, 1], [2, 0, 0], [0, 0, 2]), "floor")
    s.add(pa.Rect([-1, 1, 1], [0, 0, 2], [0, 2, 0], True), "red")
    s.add(pa.Rect([1, 1, 1], [0, 0, 2], [0, 2, 0]), "red")
    s.add(pa.Rect([0, 1, 2], [2, 0, 0], [0, 2, 0], True), "floor")
    center = np.array([0.1, 0.7, 1.1])
    verts, faces = scenes.icosphere(2, 0.55, tuple(center))
    d = verts.astype(np.float64) - center
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    normals = d.astype(np.float32)
    uvs = np.stack([np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 1], -1, 1)) / np.pi], axis=1).astype(np.float32)
    s.add(pa.Mesh(verts, faces, texcoords=uvs, normals=normals), "ball")
    s.add(pa.Rect([0.0, 1.9, 1], [0.1, 0, 0], [0, 0, 0.1]), pa.Emissive([60.0, 40.0, 12.0]))
    frm, to, fov = scenes.CAMERAS["readme"]
    s.set(pa.ThinLenCamera(pa.Film(list(size), pa.Uncharted2()), frm, to, fov))
    return s


def accel_scene(name):
    from pine_amd import scenes
    return {"cbox": lambda: scenes.cbox((64, 64), "readme"),          # order-dependent scaled boxes
            "zoo": lambda: scenes.shapes_zoo((48, 48)),
            "xshapes": lambda: scenes.xshapes_zoo((48, 48)),          # Plane, Line, Cylinder, Triangle
            "sss_mesh": lambda: scenes.sss((64, 64), 2, emissive_mesh=True),  # meshes without normals: uv are barycentrics
            "mesh_attrs": mesh_attrs_scene}[name]()


def accel_rays(scene, name, n=NUM_RAYS):
    """The fixture's rays, seed for seed: bvh_rays of tools/make_golden.py."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_golden import bvh_rays
    finally:
        sys.path.pop(0)
    return bvh_rays(scene, n, SEEDS[name])


def load_fixture(name, order):
    z = np.load(os.path.join(GOLDEN, f"accel_{name}_{order}.npz"))
    return {"pscene": z["pscene"].tobytes().decode(), "rays": np.ascontiguousarray(z["rays"]), "records": np.ascontiguousarray(z["records"]),
            "occluded": np.ascontiguousarray(z["occluded"])}


def records_as_words(hits):
    """An intersect() result (structured array, or anything of 48 bytes per ray) as (N, 12) uint32."""
    a = np.ascontiguousarray(hits)
    return a.view(np.uint32).reshape(len(a), 12)
