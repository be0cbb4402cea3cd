"""The edge rays of tests/golden/*_edge.npz (written by tools/make_golden_edge.py from the real reference): the rays an Accel user
writes and the path kernels never send -- tmin > 0, directions that are not unit vectors, axis-parallel directions with signed
zeros, origins exactly on a surface, spans that end exactly at a hit.  Plain numpy, deterministic by seed; shared by the
generator, tests/test_edge_rays.py and tests/test_edge_rays_gpu.py.

edge_rays(scene, seed, first_pass) -> (rays[n, 8] float32, cls[n] uint8), PER_CLASS rays of every class of CLASSES in that
order (a scene without a closed analytic shape has no `inside` rays).  The base rays are bvh_rays(scene, NUM_BASE, seed) of
tools/make_golden.py.  `first_pass` holds the reference's 12-word records (include/pine_gpu.h) of those base rays at tmin = 0;
the two-pass rays are functions of them and cannot be made without: edge_rays(scene, seed) leaves them out,
edge_rays_full(...)[2] says which they are.  `redraw` draws every class anew from the same base rays and first pass: the
generator replaces a ray that ties under the two traversal orders by its redraw.

Never in here, by contract (include/pine_gpu.h calls them unspecified): a non-finite word, the all-zero direction."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("tmin_random", "tmin_at_hit", "tmax_at_hit", "span_degenerate", "scaled_dir", "axis", "axis_on_plane", "in_plane", "near_parallel",
           "on_surface", "inside", "plain")
TWO_PASS = ("tmin_at_hit", "tmax_at_hit", "on_surface")  # (wholly; span_degenerate and, outside cbox, axis_on_plane in part)
PER_CLASS = 160
NUM_BASE = 640
FLT_MAX = np.finfo(np.float32).max
EXTENT = 4.0                                   # of every scene here: a 2 x 2 x 2 room, the camera 4 in front of it
LO, HI = np.float32([-1.2, -0.2, -0.2]), np.float32([1.2, 2.2, 2.2])
SCALES = np.float32([0.25, 3.0, 1e-3, 1e3])
NEAR_PARALLEL = np.float32([9e-7, 1e-6, 1.1e-6, 1e-30, 1e-42])  # around box_slabs' |d| < 1e-6, and denormal
# what _adversarial_rays of tests/test_specialize.py uses for cbox: per coordinate the two walls and a box face / the middle
CBOX_PLANES = np.float32([[-1.0, 1.0, 0.0], [0.0, 2.0, 1.0], [0.0, 2.0, 0.5]])
EDGE_SEEDS = {"cbox": 5102, "zoo": 5106, "xshapes": 5103, "sss_mesh": 5104, "mesh_attrs": 5105, "shapes_zoo": 5128, "shapes_xzoo": 5121}


def at_hit_values(t):
    """The five boundary values of a first-pass t (float32 in, float32 out): itself, its neighbours, 0.5 x and 1.5 x."""
    t = np.float32(t)
    return np.float32([t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(0)), np.float32(0.5) * t, np.float32(1.5) * t])


def base_rays(scene, seed):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_golden import bvh_rays
    finally:
        sys.path.pop(0)
    return bvh_rays(scene, NUM_BASE, seed)


def closed_shapes(pscene):
    """(kind, float parameters) of the description's spheres, boxes, OBBs, cylinders and cones."""
    out = []
    for line in pscene.splitlines():
        w = line.split()
        if len(w) > 3 and w[0] == "shape" and w[1] in ("sphere", "box", "obb", "cylinder", "cone"):
            out.append((w[1], np.array([float.fromhex(x) for x in w[3:]], np.float64)))
    return out


def _shape_lines(pscene):
    return [line for line in pscene.splitlines() if line.startswith("shape ")]


def _cbox_description():
    from pine_amd import scenes
    return scenes.cbox((16, 16), "readme").describe()


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _perp(a):
    """Two unit vectors that span the plane across a."""
    a = a / np.linalg.norm(a)
    u = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return u, np.cross(a, u)


def _round_robin(rng, fp, hits, k):
    """k of the first pass's hits, taken in turn from every geometry that was hit: each gets boundary rays of its own."""
    geom = fp[hits, 1]
    lists = [list(rng.permutation(hits[geom == g])) for g in np.unique(geom)]
    out = []
    while len(out) < k:
        for q in lists:
            if len(out) < k:
                out.append(q[(len(out) // len(lists)) % len(q)])
    return np.array(out)


def _inside_point(rng, kind, q):
    if kind == "sphere":
        return q[0:3] + _unit(rng, 1)[0] * q[3] * rng.uniform(0, 0.95)
    if kind == "box":
        return q[0:3] + (q[3:6] - q[0:3]) * rng.uniform(0.02, 0.98, 3)
    if kind == "obb":
        m = q[6:22].reshape(4, 4)
        return (m @ np.append(q[0:3] + (q[3:6] - q[0:3]) * rng.uniform(0.02, 0.98, 3), 1.0))[:3]
    if kind == "cylinder":
        u, v = _perp(q[3:6] - q[0:3])
        phi, rad = rng.uniform(0, 2 * np.pi), q[6] * np.sqrt(rng.uniform(0, 0.9))
        return q[0:3] + (q[3:6] - q[0:3]) * rng.uniform(0.02, 0.98) + (u * np.cos(phi) + v * np.sin(phi)) * rad
    n = q[3:6] / np.linalg.norm(q[3:6])  # cone: base centre, axis, radius, height; the apex is at base + n * h
    u, v = _perp(n)
    s, phi = rng.uniform(0.02, 0.9), rng.uniform(0, 2 * np.pi)
    return q[0:3] + n * q[7] * s + (u * np.cos(phi) + v * np.sin(phi)) * q[6] * (1 - s) * np.sqrt(rng.uniform(0, 0.9))


def _grid_origins(rng, n):
    """Cell centres of a 12 x 12 x 12 grid over the scene's extent."""
    return (LO + (rng.integers(0, 12, (n, 3)).astype(np.float32) + np.float32(0.5)) * ((HI - LO) / np.float32(12))).astype(np.float32)


def _axis_dirs(rng, n):
    """+-e_i; the other two components +0.0 or -0.0, half each."""
    d = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    axis = rng.integers(0, 3, n)
    d[np.arange(n), axis] = np.where(rng.random(n) < 0.5, np.float32(1.0), np.float32(-1.0))
    return d, axis


def _aim(rng, o, d, axis):
    """Half of the axis rays start outside the extent and look through it, as an orthographic camera's do."""
    n = len(o)
    out = rng.random(n) < 0.5
    sign = d[np.arange(n), axis]
    start = np.where(sign > 0, LO[axis] - np.float32(0.5), HI[axis] + np.float32(0.5)).astype(np.float32)
    o[np.arange(n), axis] = np.where(out, start, o[np.arange(n), axis])
    return o


def edge_rays_full(scene, seed, first_pass=None, redraw=0, unscaled=False):
    """-> rays, cls, two_pass (bool: the ray is a function of first_pass).  unscaled: the scaled_dir rays before scaling (the
    generator compares the two answers)."""
    pscene = scene.describe()
    B = base_rays(scene, seed)
    fp = None if first_pass is None else np.ascontiguousarray(first_pass, dtype=np.uint32).reshape(NUM_BASE, 12)
    hits = None if fp is None else np.nonzero(fp[:, 1].view(np.int32) >= 0)[0]
    cbox = _shape_lines(pscene) == _shape_lines(_cbox_description())  # (the Cornell box: CBOX_PLANES are its planes)
    n = PER_CLASS
    rays_out, cls_out, two_out = [], [], []

    def emit(ci, r, two):
        r = np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 8)
        rays_out.append(r)
        cls_out.append(np.full(len(r), ci, np.uint8))
        two_out.append(np.broadcast_to(np.asarray(two, dtype=bool), (len(r),)).copy())

    def ray(o, d, tmin, tmax):
        k = len(o)
        return np.concatenate([np.float32(o), np.float32(d), np.broadcast_to(np.float32(tmin), (k,))[:, None], np.broadcast_to(np.float32(tmax), (k,))[:, None]], axis=1)

    for ci, name in enumerate(CLASSES):
        rng = np.random.default_rng([seed, ci, redraw])
        if name == "tmin_random":
            # (three quarters camera rays: in the open scenes a tmin of this size leaves too few hits among the short rays
            #  between two points for the class to say anything)
            r = B[np.r_[rng.choice(NUM_BASE // 2, n - n // 4, replace=False), NUM_BASE // 2 + rng.choice(NUM_BASE - NUM_BASE // 2, n // 4, replace=False)]].copy()
            r[:, 6] = rng.uniform(0, 1.5 * EXTENT, n).astype(np.float32)
            emit(ci, r, False)
        elif name in ("tmin_at_hit", "tmax_at_hit"):
            if fp is None:
                continue
            pick = _round_robin(rng, fp, hits, n // 5)
            r = np.repeat(B[pick], 5, axis=0)
            r[:, 6 if name == "tmin_at_hit" else 7] = np.concatenate([at_hit_values(t) for t in fp[pick, 0].view(np.float32)])
            emit(ci, r, True)
        elif name == "span_degenerate":
            k = n // 8
            if fp is not None:  # tmin == tmax == a hit's t
                pick = _round_robin(np.random.default_rng([seed, ci, redraw, 1]), fp, hits, k)  # (a stream of its own: the rest is the same without a first pass)
                r = B[pick].copy()
                r[:, 6] = r[:, 7] = fp[pick, 0].view(np.float32)
                emit(ci, r, True)
            r = B[rng.choice(NUM_BASE, n - k, replace=False)].copy()
            u = rng.uniform(size=(n - k, 2)).astype(np.float32)
            a, b, c = k, 2 * k, 3 * k                   # ... elsewhere | tmin > tmax | tmax == 0 | the rest: a finite negative tmin
            r[:a, 6] = r[:a, 7] = np.float32(0.1) + np.float32(5.0) * u[:a, 0]
            r[a:b, 6] = np.float32(1.0) + np.float32(4.0) * u[a:b, 0]
            r[a:b, 7] = r[a:b, 6] * (np.float32(0.1) + np.float32(0.8) * u[a:b, 1])
            r[b:c, 7] = 0.0
            r[c:, 6] = -(np.float32(0.01) + np.float32(10.0) * u[c:, 0])
            emit(ci, r, False)
        elif name == "scaled_dir":
            r = B[rng.choice(NUM_BASE, n, replace=False)].copy()
            s = SCALES[np.arange(n) % 4]
            r[n // 2:, 6] = rng.uniform(0, 2.0, n - n // 2).astype(np.float32)
            if not unscaled:
                r[:, 3:6] *= s[:, None]
                r[:, 6] /= s
                finite = r[:, 7] < FLT_MAX
                r[finite, 7] /= s[finite]
            emit(ci, r, False)
        elif name == "axis":
            d, axis = _axis_dirs(rng, n)
            emit(ci, ray(_aim(rng, _grid_origins(rng, n), d, axis), d, 0.0, FLT_MAX), False)
        elif name == "axis_on_plane":
            if not cbox and fp is None:
                continue
            d, axis = _axis_dirs(rng, n)
            o = _aim(rng, _grid_origins(rng, n), d, axis)
            on = rng.random((n, 3)) < 0.5
            on[np.arange(n), rng.integers(0, 3, n)] = True
            on[on.all(axis=1), 0] = False                # one or two coordinates
            if cbox:
                plane = CBOX_PLANES[np.arange(3)[None, :], rng.integers(0, 3, (n, 3))]
            else:
                plane = fp[rng.choice(hits, n), 4:7].view(np.float32)
            emit(ci, ray(np.where(on, plane, o), d, 0.0, FLT_MAX), not cbox)
        elif name == "in_plane":
            d = _unit(rng, n)
            j = rng.integers(0, 3, n)
            d[np.arange(n), j] = 0.0
            d = (d / np.linalg.norm(d, axis=1, keepdims=True) * (1 - 1e-6)).astype(np.float32)
            d[np.arange(n), j] = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0))
            emit(ci, ray(rng.uniform(LO, HI, (n, 3)), d, 0.0, FLT_MAX), False)
        elif name == "near_parallel":
            d = (_unit(rng, n) * (1 - 1e-6)).astype(np.float32)
            mag = NEAR_PARALLEL[np.arange(n) % len(NEAR_PARALLEL)]
            d[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.random(n) < 0.5, mag, -mag)
            emit(ci, ray(rng.uniform(LO, HI, (n, 3)), d, 0.0, FLT_MAX), False)
        elif name == "on_surface":
            if fp is None:
                continue
            pick = _round_robin(rng, fp, hits, n)
            tmin = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(1e-4))
            emit(ci, ray(fp[pick, 4:7].view(np.float32), _unit(rng, n), tmin, FLT_MAX), True)
        elif name == "inside":
            shapes = closed_shapes(pscene)
            if not shapes:
                continue
            o = np.array([_inside_point(rng, *shapes[i % len(shapes)]) for i in range(n)])
            emit(ci, ray(o, _unit(rng, n), 0.0, FLT_MAX), False)
        else:
            emit(ci, B[rng.choice(NUM_BASE, n, replace=False)], False)
    rays, cls, two = np.concatenate(rays_out), np.concatenate(cls_out), np.concatenate(two_out)
    assert np.isfinite(rays).all() and (rays[:, 3:6] != 0).any(axis=1).all() and len(rays) <= 2000
    return np.ascontiguousarray(rays), cls, two


def edge_rays(scene, seed, first_pass=None):
    rays, cls, _ = edge_rays_full(scene, seed, first_pass)
    return rays, cls


def class_of(cls, name):
    return cls == CLASSES.index(name)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACCEL_SCENES = ("cbox", "zoo", "xshapes", "sss_mesh", "mesh_attrs")
TRAV_SCENES = ("cbox", "zoo")
SHAPE_FILES = {"shapes_zoo": "shapes_zoo_edge", "shapes_xzoo": "shapes_xzoo_edge"}


def shape_scene(which):
    from pine_amd import scenes
    return scenes.shapes_zoo((48, 48)) if which == "shapes_zoo" else scenes.xshapes_zoo((48, 48))


def fixture_parts(stem):
    """The files of one fixture: <stem>.npz, or <stem>_a.npz, <stem>_b.npz ... where one file would pass 100 KB (split by ray)."""
    one = os.path.join(GOLDEN, stem + ".npz")
    if os.path.exists(one):
        return [one]
    parts = [os.path.join(GOLDEN, f"{stem}_{c}.npz") for c in "abcdef"]
    parts = [p for p in parts if os.path.exists(p)]
    assert parts, stem
    return parts


PER_RAY = {"rays": 0, "cls": 0, "redraw": 0, "records": 0, "occluded": 0, "shape_records": 1}  # (key: the axis that runs over the rays)


def load_edge(stem):
    """One fixture as a dict; the per-ray arrays of a split fixture joined again."""
    zs = [np.load(p) for p in fixture_parts(stem)]
    out = {}
    for k in zs[0].files:
        if k in PER_RAY:
            out[k] = np.ascontiguousarray(np.concatenate([z[k] for z in zs], axis=PER_RAY[k]))
        elif k in ("pscene", "info"):
            out[k] = zs[0][k].tobytes().decode()
        else:
            out[k] = np.ascontiguousarray(zs[0][k])
    return out


def regenerate(scene, seed, fx):
    """The fixture's rays from its stored first pass and redraw counts."""
    rays, cls, two = edge_rays_full(scene, seed, fx["first_pass"])
    for k in range(1, int(fx["redraw"].max()) + 1):
        again = edge_rays_full(scene, seed, fx["first_pass"], redraw=k)[0]
        rays[fx["redraw"] == k] = again[fx["redraw"] == k]
    return rays, cls, two
