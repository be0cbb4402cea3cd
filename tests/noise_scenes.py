"""The queries and scenes of the noise-node fixtures (tests/golden/noise_*.npz, listed in noise.json): shared by
tools/make_golden_noise.py, which runs them through the real reference, and tests/test_noise.py / test_noise_gpu.py."""
import numpy as np

F32 = np.float32
NUM_QUERIES = 384
TWIN_QUERY = 200  # an ordinary query: the constant twins' p, n and uv are its values
OCTAVES = (1, 2, 3, 5, 8)
MAX_OCTAVES = 8   # the largest count any material of the zoo runs
P_SCALE = 7.3     # the largest factor on a coordinate before it reaches a noise node


def _hash(n, seed):
    """n 32-bit words of an integer hash of the index."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def _unit(n, seed):
    return (_hash(n, seed) >> np.uint32(8)).astype(F32) / F32(1 << 24)


def queries():
    """(NUM_QUERIES, 8): p, n, uv.  Ordinary values in [-3, 3) (half of them negative); then, one axis at a time, coordinates
    exactly on an integer (the smoothed fraction is 0: one corner carries the whole weight) and coordinates of magnitude 2^16
    to 2^18 (the cell index is large, and after a few doublings the fraction has no bits left)."""
    n = NUM_QUERIES
    q = (_unit(n * 8, 41).reshape(n, 8) * F32(6) - F32(3)).astype(F32)
    nn = q[:, 3:6] / np.maximum(np.linalg.norm(q[:, 3:6], axis=1, keepdims=True), F32(1e-6))
    q[:, 3:6] = nn.astype(F32)
    i = 0
    ints = [0, 1, -1, 2, -2, 3, -3, 5, -7, 100, -0.0, 16]
    for axis in range(3):
        for v in ints:
            q[i, axis] = F32(v)
            i += 1
    for axis in (6, 7):  # uv on an integer
        for v in ints[:6]:
            q[i, axis] = F32(v)
            i += 1
    big = _unit(24, 43) * F32(3 * 65536) + F32(65536)  # [2^16, 2^18)
    for k in range(24):
        q[i, k % 3] = big[k] if k % 2 == 0 else -big[k]
        i += 1
    assert i <= TWIN_QUERY < n, i
    return np.ascontiguousarray(q, dtype=F32)


def varying_octaves(pa, P):
    """1 + 3.99 * fract(p.x): the counts 1 to 4, another for each lane."""
    return pa.node_fract(pa.Node.of(P, True)[0]) * 3.99 + 1.0


def varying_octaves_of(q):
    """The count varying_octaves gives at each query, in the node programs' float arithmetic."""
    x = q[:, 0].astype(F32)
    v = (x - np.floor(x)).astype(F32) * F32(3.99) + F32(1.0)
    return v.astype(F32).astype(np.int32)


# ---- the per-call zoo --------------------------------------------------------------------------------------------------------
def programs(pa, P, N, U):
    """(name, has a twin, material) over Position-like P, Normal-like N and UV-like U (nodes, or constants for the twins)."""
    Nf, N3 = pa.Noisef, pa.Noise3f
    P, N, U = pa.Node.of(P, True), pa.Node.of(N, True), pa.Node.of(U, True)
    grey = [0.8, 0.7, 0.6]
    out = []
    for o in OCTAVES:
        out.append((f"noise3f position {o}", o in (1, 5), pa.Diffuse(N3(P, o))))
        out.append((f"noisef position {o} roughness", o in (2, 8), pa.Metal(grey, Nf(P, float(o)))))
    var = varying_octaves(pa, P)
    out += [
        ("noisef octaves 2.9", True, pa.Glossy(grey, Nf(P, 2.9), 1.5)),
        ("noise3f varying octaves", True, pa.Diffuse(N3(P, var))),
        ("noisef varying octaves", True, pa.Metal(grey, Nf(P, var))),
        ("noise3f uv", True, pa.Diffuse(N3(U, 3))),
        ("noisef scaled roughness", True, pa.Glossy(grey, Nf(P * P_SCALE, 5), 1.5)),
        ("noisef normal", True, pa.Metal(grey, Nf(N, 8))),
        ("noisef squared", True, pa.Diffuse(pa.Vec3(Nf(P, 3) ** 2.0))),
        ("comps", True, pa.Uber(grey, N3(P, 2)[2], N3(U, 2)[1], Nf(N, 1) * 0.5, 1.45)),
    ]
    return out


OCT0 = ("oct0_albedo", "oct0_roughness")


def noise_zoo(q):
    """-> (scene, [name]): every program over Position() / Normal() / UV(), the constant twins at TWIN_QUERY, then the two
    oct0_* materials, whose octaves are 0 and -0.5: no round, the reference's 0 / 0."""
    import pine_amd as pa
    sc, names = pa.Scene(), []
    progs = programs(pa, pa.Position(), pa.Normal(), pa.UV())
    for name, _, m in progs:
        sc.add(f"m{len(names)}", m)
        names.append(name)
    t = [float(v) for v in q[TWIN_QUERY]]
    for name, twin, m in programs(pa, t[0:3], t[3:6], [t[6], t[7], 0.0]):
        if twin:
            sc.add(f"m{len(names)}", m)
            names.append("twin of " + name)
    sc.add(OCT0[0], pa.Diffuse(pa.Noise3f(pa.Position(), 0)))
    sc.add(OCT0[1], pa.Metal([0.8, 0.7, 0.6], pa.Noisef(pa.Position(), -0.5)))
    names += list(OCT0)
    return sc, names


def twins():
    """[(index of the twin, index of its original)] in noise_zoo's material order."""
    import pine_amd as pa
    flags = [t for _, t, _ in programs(pa, pa.Position(), pa.Normal(), pa.UV())]
    originals = [i for i, t in enumerate(flags) if t]
    return [(len(flags) + k, i) for k, i in enumerate(originals)]


# ---- films -------------------------------------------------------------------------------------------------------------------
# name: (size, spp, depth)
FILMS = {"noise_room_48x32_s8_d4": ((48, 32), 8, 4), "noise_script_room_48x32_s8_d4": ((48, 32), 8, 4)}
GUIDES_SIZE = (32, 24)
NOISY = ("floor", "back", "ball", "pearl")  # the rooms' materials that a noise node drives


def _walls(pa, s, size, default):
    s.add(pa.Rect([0, 0, 0], [4, 0, 0], [0, 0, 4], True), "floor")
    s.add(pa.Rect([0, 3, 0], [4, 0, 0], [0, 0, 4], False), "white")
    s.add(pa.Rect([0, 1.5, 2], [4, 0, 0], [0, 3, 0], True), "back")
    s.add(pa.Rect([0, 1.5, -2], [4, 0, 0], [0, 3, 0], False), "white")
    s.add(pa.Rect([-2, 1.5, 0], [0, 0, 4], [0, 3, 0], False), "white")
    s.add(pa.Rect([2, 1.5, 0], [0, 0, 4], [0, 3, 0], True), "white")
    s.add(pa.Rect([0, 2.99, 0], [1.2, 0, 0], [0, 0, 1.2], False), "lamp")
    s.add(pa.Sphere([-0.8, 0.6, 0.4], 0.6), "ball")
    s.add(pa.Sphere([0.875, 0.5, 0.25], 0.5), "pearl")
    s.set(pa.ThinLenCamera(pa.Film(list(size or default), pa.Uncharted2()), [0, 1.5, -1.875], [0, 1.2, 2], 0.875))


def room(size=None, flat=False):
    """A closed room with an area light: a marbled back wall, a floor whose octave count varies across it, a noise-roughened
    ball and a pearl with noise in albedo and metallic.  flat: every noise node replaced by a constant (tools/noise_speed.py)."""
    import pine_amd as pa
    Nf, N3 = pa.Noisef, pa.Noise3f
    if flat:
        Nf = lambda p, o: pa.Node.of(0.25)  # noqa: E731
        N3 = lambda p, o: pa.Node.of([0.25, 0.25, 0.25])  # noqa: E731
    P, U = pa.Position(), pa.UV()
    s = pa.Scene()
    s.add("floor", pa.Diffuse(N3(U * 6.0, varying_octaves(pa, U * 2.0)) * 2.0))
    s.add("back", pa.Diffuse(pa.lerp(Nf(P * 3.0, 5), [0.9, 0.85, 0.8], [0.2, 0.25, 0.4])))
    s.add("ball", pa.Metal([0.9, 0.8, 0.6], Nf(P * 8.0, 3)))
    s.add("pearl", pa.Uber(N3(pa.Normal() * 2.0, 2) * 2.0, 0.25, Nf(P * 5.0, 2), 0.0, 1.45))
    s.add("white", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add("lamp", pa.Emissive([12.0, 11.0, 9.0]))
    _walls(pa, s, size, FILMS["noise_room_48x32_s8_d4"][0])
    return s


def script_room(size=None):
    """The room as examples/noise.pine builds it, line for line: a marbled wall and a noise-roughened sphere."""
    import pine_amd as pa
    P, U = pa.Position(), pa.UV()
    s = pa.Scene()
    s.add("floor", pa.Diffuse(pa.Noise3f(U * 6.0, 3) * 2.0))
    s.add("back", pa.Diffuse(pa.lerp(pa.Noisef(P * 3.0, 5), [0.875, 0.75, 0.625], [0.25, 0.25, 0.5])))
    s.add("ball", pa.Metal([0.875, 0.75, 0.5], pa.Noisef(P * 8.0, 3)))
    s.add("pearl", pa.Diffuse(pa.Noise3f(P * 4.0, 2)))
    s.add("white", pa.Diffuse([0.75, 0.75, 0.75]))
    s.add("lamp", pa.Emissive([12.0, 11.0, 9.0]))
    _walls(pa, s, size, FILMS["noise_script_room_48x32_s8_d4"][0])
    return s


def film_scene(name):
    return script_room(FILMS[name][0]) if name.startswith("noise_script_room") else room(FILMS[name][0])
