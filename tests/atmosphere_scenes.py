"""The light configurations, queries and scenes of the Atmosphere fixtures (tests/golden/atmos_*.npz, listed in atmos.json):
shared by tools/make_golden_atmosphere.py, which runs them through the real reference, and tests/test_atmosphere.py /
test_atmosphere_gpu.py.  The stored queries are what the tests read; the functions here say where they came from."""
import numpy as np

import envsky_scenes as E

# name: (w, h, sun direction as the caller gives it)
CONFIGS = {
    "noon": (64, 32, (0.3, 1.0, 0.2)),
    "zenith": (33, 17, (0.0, 1.0, 0.0)),
    "tall": (8, 40, (1.0, 0.05, 0.0)),
    "low": (64, 32, (1.0, -0.02, 0.0)),
    "mid": (256, 128, (0.3, 1.0, 0.2)),
    "default": (1024, 1024, (0.3, 1.0, 0.2)),
}
SMALL = ("noon", "zenith", "tall", "low")
SUN_COLOR = (4.0, 3.0, 2.5)  # of the per-call records (the films: FILM_SUN_COLOR)
NUM_QUERIES = 512
SUNS = ((0.3, 1.0, 0.2), (0.0, 1.0, 0.0), (1.0, 0.05, 0.0), (1.0, -0.02, 0.0), (0.0, -1.0, 0.0))  # of atmos_color.npz


def light(name, device=None, color=SUN_COLOR):
    import pine_amd as pa
    w, h, sun = CONFIGS[name]
    return pa.Atmosphere(sun, color, (w, h), device=device)


def normalized(v):
    """normalize(vec3) in binary32, the operations of vecmath.h: x * x + y * y + z * z, sqrt, three divisions."""
    v = np.asarray(v, dtype=np.float32)
    length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v / length).astype(np.float32)


def dot32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cone_pairs(sun):
    """Three pairs of binary32 directions next to each other on either side of the sun-disc test dot(direction, sun) > 0.998f,
    found by bisection of the angle in three planes through the (normalised) sun direction."""
    s = normalized(sun).astype(np.float64)
    out = []
    for axis in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)):
        t = np.cross(s, axis)
        if np.linalg.norm(t) < 0.3:
            t = np.cross(s, (0.6, 0.0, 0.8))
        t /= np.linalg.norm(t)

        def at(theta):
            return (np.cos(theta) * s + np.sin(theta) * t).astype(np.float32)

        def inside(theta):
            return dot32(at(theta), s.astype(np.float32)) > np.float32(0.998)

        lo, hi = 0.0, 0.2  # cos(0.2) = 0.980
        assert inside(lo) and not inside(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if inside(mid):
                lo = mid
            else:
                hi = mid
        out += [at(lo), at(hi)]
    return out


def color_queries():
    """The (n, 7) queries of atmos_color.npz: direction, sun direction (normalised), flag.  Every direction with both flags."""
    rows = []
    for k, sun in enumerate(SUNS):
        s = normalized(sun)
        r = (E._hash(200 * 3, 500 + k) >> np.uint32(8)).astype(np.float32) / np.float32(1 << 24)
        d = r.reshape(200, 3) * 2 - 1
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
        dirs = [x.astype(np.float32) for x in d]
        dirs += [np.array(v, dtype=np.float32) for v in ((0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, 1), (-0.6, 0, 0.8))]
        for y in (1e-3, -1e-3):
            for xz in ((1, 0), (0, -1), (0.6, 0.8)):
                dirs.append(normalized((xz[0], y, xz[1])))
        dirs.append(s)
        dirs.append((-s).astype(np.float32))
        dirs += cone_pairs(sun)
        for dv in dirs:
            for flag in (0.0, 1.0):
                rows.append(np.concatenate([dv, s, [flag]]).astype(np.float32))
    return np.stack(rows).astype(np.float32)


def base_queries(name):
    """The (NUM_QUERIES, 5) queries of a configuration before the generator overwrites the directions of [384, 448) with
    directions the reference's sample() returned and the u2 of [448, 456) with what its search found: u2, then wo."""
    w, h = CONFIGS[name][:2]
    n = NUM_QUERIES
    r = (E._hash(n * 5, 3000 + w * 31 + h) >> np.uint32(8)).astype(np.float32) / np.float32(1 << 24)
    q = r.reshape(n, 5).copy()
    top = np.float32(1) - np.float32(2.0 ** -24)
    edge = [np.float32(0), top] + [np.float32(k) / np.float32(w) for k in range(1, min(w, 12))]
    for i in range(0, 96):  # u2: edge values in one or both components
        if i % 3 != 1:
            q[i, 0] = edge[i % len(edge)]
        if i % 3 != 0:
            q[i, 1] = edge[(i // 3) % len(edge)] if i % 2 else np.float32((i // 2) % h) / np.float32(h)
    for i in range(256, 320):  # u2 within 2^-9 of 0 and of 1: what the sun's texels leave for every other texel
        k = i - 256
        near = (np.float32(k % 16) + q[i, 0]) * np.float32(2.0 ** -13)
        near = near if (k // 16) % 2 == 0 else min(top, np.float32(1) - near)
        q[i, k % 2] = near
    d = q[:, 2:5] * 2 - 1
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-6)
    q[:, 2:5] = d.astype(np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    for i in range(128, 192):  # the poles and the atan2 seam, and directions next to them
        q[i, 2:5] = axes[i % 6]
        if i >= 134:
            q[i, 2 + (i // 6) % 3] += np.float32((i - 160) * 1e-4)
    for i in range(192, 256):  # directions whose ic lands (as nearly as float allows) on texel centres, corners and on size - 1
        k = i - 192
        sx = (np.float32(k % w) + np.float32(0.5 * (k % 2))) / np.float32(w)
        sy = (np.float32((k // 2) % h) + np.float32(0.5 * ((k // 2) % 2))) / np.float32(h)
        if k >= 48:
            sx, sy = np.float32(w - 1) / np.float32(w), np.float32(h - 1) / np.float32(h) if k % 2 else np.float32(1)
        phi = np.float32(sx) * np.float32(2 * np.pi)
        ct = np.float32(1) - 2 * np.float32(sy)
        st = np.sqrt(max(np.float32(0), 1 - ct * ct))
        q[i, 2:5] = [st * np.cos(phi), ct, st * np.sin(phi)]  # (y and z swapped, as Atmosphere swaps them)
    s = normalized(CONFIGS[name][2])
    q[320:328, 2:5] = s  # the sun itself, and the sun-disc boundary
    q[328:334, 2:5] = np.stack(cone_pairs(CONFIGS[name][2]))
    return q.astype(np.float32)


# ---- films: the open scene of the ImageSky fixtures, 48 x 32, sun colour (4, 4, 4) ------------------------------------------------
FILM_SIZE = (48, 32)
FILM_SUN_COLOR = (4.0, 4.0, 4.0)
# name: (configuration, sampler kind, spp, depth)
FILMS = {
    "noon_blue_s16_d5": ("noon", "blue", 16, 5),
    "low_blue_s16_d5": ("low", "blue", 16, 5),
    "noon_sobol_s8_d5": ("noon", "sobol", 8, 5),
    "default_blue_s16_d5": ("default", "blue", 16, 5),
}


def film_scene(name, device=None):
    """The scene of a film, its Atmosphere set (its tables built on `device`, or None: on the host)."""
    s = E._open_sun(FILM_SIZE)
    s.set(light(FILMS[name][0], device, FILM_SUN_COLOR))
    return s


def film_sampler(name):
    import pine_amd as pa
    kind, spp = FILMS[name][1:3]
    return {"blue": pa.BlueSampler, "sobol": pa.SobolSampler}[kind](spp)
