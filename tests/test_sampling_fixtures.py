"""The middle of a path vertex, one call at a time: the six BSDF lobes (bxdf_f / bxdf_pdf / bxdf_is_delta / bxdf_sample with
the Trowbridge-Reitz sampling, Refract and FrDielectric under them), shape_sample / shape_pdf of every geometry and
light_sample_other of every other light -- compared three ways, bit for bit: the real reference (tests/golden/bxdf_lobes.npz,
lightsamples_*.npz, written by `pine_ref bxdf` / `pine_ref lightsamples` through tools/make_golden.py --sampling), the CPU
oracle (oracle_bxdf / oracle_light_samples) and the product's PINE_HD functions, built for the host (device = -1) and for the
device (pine_gpu_test_bxdf / pine_gpu_test_light_samples, include/pine_gpu.h has the layouts).

No tolerance: float bits, except that where the reference's value is a NaN the value under test must be a NaN (payload and
sign free).  The inputs come from the seeded generators below; the fixtures store them and the tests rebuild and compare them.

What is left out because the REFERENCE cannot be asked: f / pdf of the Conductor, Refractive and RefractiveDielectric lobes
below alpha = roughness^2 < 1e-4f, where the reference's CHECK aborts (bxdf.cpp:67,82,120,136,200,224) -- those cases call
sample only (calls = 2); and Cylinder::sample, which is PINE_UNREACHABLE (geometry.h:148): its records carry -1."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

LOBES = ["Diffuse", "Conductor", "Refractive", "RefractiveDielectric", "DiffusiveDielectric", "BSSRDF"]
F32 = np.float32
ONE_MINUS = F32(1) - F32(2.0 ** -24)

Z_EDGES = [1.0, float(ONE_MINUS), 0.99999, 0.999995, 0.5, 0.1, 0.0316, 0.0317, 1e-3, 1e-6]
Z_ALL = [s * z for z in Z_EDGES for s in (1.0, -1.0)] + [0.0, -0.0]                     # 22 values
ROUGHNESS = [0.0, 0.0099999, 0.01, 0.010001, 0.05, 0.2, 0.6, 0.60000002, 1.0]
IOR = [1.0, 1.0000001, 1.45, 1.5, 1.9999999, 2.0, 2.5, 0.9, 1 / 1.5]
ALBEDO = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.8, 0.5, 0.2)]
AZIMUTHS = 4  # 0: +x axis, 1: +y axis (both give CosPhi / SinPhi their sin(theta) = 0 and exact-zero components), 2, 3: oblique


# (pixel x, pixel y, sample index) of SobolSampler(64) on a 1024 x 1024 image, see bxdf_cases part F
RIM_STATES = [(4, 143, 10), (39, 26, 53), (66, 69, 29), (196, 15, 52), (310, 32, 22), (450, 112, 6), (639, 50, 44), (674, 44, 57),
              (759, 32, 12), (817, 62, 63), (1009, 47, 14)]
TIR_STATES = [(102, 258, 27), (352, 409, 7), (365, 277, 20), (586, 312, 51), (689, 296, 42), (796, 48, 48), (817, 202, 9),
              (820, 215, 4), (908, 332, 61), (925, 85, 29), (936, 334, 47), (957, 259, 27)]


def direction(z, az):
    """A float32 unit vector with the given z; azimuths 0 and 1 lie on the axes exactly."""
    z = float(z)
    s = float(np.sqrt(max(0.0, 1.0 - z * z)))
    if az == 0:
        v = (s, 0.0, z)
    elif az == 1:
        v = (0.0, s, z)
    else:
        phi = 0.7 if az == 2 else 3.9
        v = (s * np.cos(phi), s * np.sin(phi), z)
    return np.array(v, dtype=np.float64).astype(F32)


def refract32(wi, ior):
    """Refract(wi, (0,0,1), ior) of scattering.h:58-77 in float32 steps: the exact refraction partner of wi, or None."""
    wi = wi.astype(F32)
    cos, eta, n = wi[2], F32(ior), np.array([0, 0, 1], F32)
    if cos < 0:
        eta, cos, n = F32(1) / eta, -cos, -n
    sin2i = max(F32(0), F32(1) - cos * cos)
    sin2t = F32(sin2i / (eta * eta))
    if sin2t >= 1:
        return None
    cos_t = np.sqrt(F32(1) - sin2t, dtype=F32)
    return (-wi / eta + (cos / eta - cos_t) * n).astype(F32)


def bxdf_cases():
    """-> cases[n, 16] float32 in the layout of `pine_ref bxdf`, the same list for every lobe, plus the scanned sampler states of part F."""
    rng = np.random.default_rng(20261018)
    rows = []

    def add(lobe, albedo, roughness, ior, wi, wo, calls=3, px=None):
        p = rng.integers(0, 1024, 2) if px is None else px[:2]
        index = int(rng.integers(0, 64)) if px is None else px[2]
        rows.append([lobe, *albedo, roughness, ior, *wi, *wo, p[0], p[1], index, calls])

    nz = len(Z_ALL)
    for lobe in range(6):
        # A. every z x every azimuth as wi, against three other edge directions
        for i, z in enumerate(Z_ALL):
            for a in range(AZIMUTHS):
                for k in range(3):
                    add(lobe, ALBEDO[(i + k) % 3], ROUGHNESS[(i + a + k) % 9], IOR[(i + 2 * a + k) % 9], direction(z, a),
                        direction(Z_ALL[(i * 7 + a * 5 + k * 3 + 1) % nz], (a + k) % AZIMUTHS))
        # B. every roughness x every z;  C. every ior x every z (rough and smooth)
        for r, rough in enumerate(ROUGHNESS):
            for i, z in enumerate(Z_ALL):
                add(lobe, ALBEDO[(r + i) % 3], rough, IOR[(r + i) % 9], direction(z, (r + i) % AZIMUTHS),
                    direction(Z_ALL[(i * 5 + r) % nz], (i + 2) % AZIMUTHS))
        for e, ior in enumerate(IOR):
            for i, z in enumerate(Z_ALL):
                add(lobe, ALBEDO[(e + i) % 3], (0.2, 0.0, 0.05)[(e + i) % 3], ior, direction(z, (e + i + 1) % AZIMUTHS),
                    direction(Z_ALL[(i * 3 + e + 11) % nz], (i + e) % AZIMUTHS))
        # D. special pairs per ior: wo = -wi, Reflect(wi), wi, the exact refraction of wi (from above and from below)
        for e, ior in enumerate(IOR):
            for j, z in enumerate([0.5, -0.5, 0.1, -0.1, 0.99999, -0.99999, 1e-3, -1e-3, 1.0, -1.0]):
                wi = direction(z, (e + j) % AZIMUTHS)
                rough = (0.05, 0.2, 0.6, 1.0, 0.010001)[(e + j) % 5]
                pairs = [-wi, wi * np.array([-1, -1, 1], F32), wi]
                wt = refract32(wi, ior)
                if wt is not None:
                    pairs.append(wt)
                for wo in pairs:
                    add(lobe, ALBEDO[1 + (e + j) % 2], rough, ior, wi, wo)
            # ... and wi just inside / outside total internal reflection: sin2ThetaT = (1 - z^2) / eta^2 around 1
            crit = 1.0 - 1.0 / (ior * ior) if ior > 1 else 1.0 - ior * ior
            if crit > 0:
                zc = F32(np.sqrt(crit))
                side = -1.0 if ior > 1 else 1.0  # the dense side of the interface
                for zz in (np.nextafter(zc, F32(0)), zc, np.nextafter(zc, F32(2)), F32(zc * F32(1.001)), F32(zc * F32(0.999))):
                    for rough in (0.0, 0.2):
                        wi = direction(side * float(zz), 2)
                        add(lobe, ALBEDO[2], rough, ior, wi, direction(-side * 0.5, 3))
        # E. sample(): 16 (pixel, index) pairs per (roughness, ior, wi), so that `get1d() < fr` falls both ways
        combos = [(rough, IOR[(r * 2 + 3) % 9], direction((0.5, -0.5, 0.1)[r % 3], 2 + r % 2)) for r, rough in enumerate(ROUGHNESS)]
        combos += [(rough, ior, direction(z, 2)) for ior in IOR for rough, z in ((0.0, 0.5), (0.2, -0.3))]
        for c, (rough, ior, wi) in enumerate(combos):
            for s in range(16):
                add(lobe, ALBEDO[2], rough, ior, wi, direction(0.3, 3), px=((37 * c + 5 * s) % 1024, (101 * c + 3 * s) % 1024, (7 * s + c) % 64))
        # F. sampler states found by scanning all 1024 x 1024 x 64 of them, where tr_SampleWm's nh.z falls below 1e-6 (a grazing wi,
        #    a disk sample on the lower rim: `pmax(1e-6f, nh.z)` decides wm) ...
        if lobe in (1, 2, 3, 4):
            for px in RIM_STATES:
                add(lobe, ALBEDO[2], 0.2, 1.5, np.array([1.0, 0.0, 1e-6], F32), direction(0.3, 3), px=px)
        #    ... and where Refract(wi, wm, ior) of the rough RefractiveDielectric lobe meets sin2ThetaT == 1 exactly (the smooth
        #    branch never does: FrDielectric returns 1 at the same equality and the reflection is taken)
        if lobe == 3:
            for px in TIR_STATES:
                add(lobe, ALBEDO[2], 0.2, 1.5, np.array([0.6499231, 0.0, -0.76], F32), direction(0.3, 3), px=px)
        # G. random: uniform directions and parameters
        for _ in range(460):
            v = rng.normal(size=(2, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            add(lobe, rng.uniform(0, 1, 3), float(rng.uniform(0, 1)) ** 2, float(rng.uniform(0.6, 2.6)), v[0].astype(F32), v[1].astype(F32))
    cases = np.array(rows, dtype=np.float64).astype(F32)
    # the reference aborts in f / pdf of these lobes below alpha = 1e-4f (CHECK, bxdf.cpp): sample() only
    alpha = cases[:, 4] * cases[:, 4]
    no_f = np.isin(cases[:, 0], (1, 2, 3)) & (alpha < F32(1e-4))
    cases[no_f, 15] = 2
    return cases


SCENES = {
    "shapes_zoo": lambda sc: sc.shapes_zoo((48, 48)),
    "xshapes_zoo": lambda sc: sc.xshapes_zoo((48, 48)),
    "lights_zoo": lambda sc: sc.lights_zoo((48, 48)),
    "mesh_lamp": lambda sc: sc.sss((16, 16), 1, emissive_mesh=True),  # the scene list's emissive Mesh (Mesh::sample)
}


def parse_shapes(pscene):
    """-> [(kind, [floats...])] of the description's shape lines, (light count incl. the environment light)"""
    shapes, lights = [], 0
    for line in pscene.splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "shape":
            vals = []
            for t in tok[3:]:
                try:
                    vals.append(float.fromhex(t) if "x" in t.lower() else float(t))
                except ValueError:
                    vals.append(float("nan"))
            shapes.append((tok[1], vals))
        elif tok[0] in ("light", "envlight"):
            lights += 1
    return shapes, lights


def light_queries(pscene):
    """-> queries[256, 6] float32 (o, u2, u1) for `pine_ref lightsamples` on this scene."""
    rng = np.random.default_rng(777)
    shapes, _ = parse_shapes(pscene)
    grid = [(a, b) for a in (0.0, 0.5, float(ONE_MINUS)) for b in (0.0, 0.5, float(ONE_MINUS))]
    q = []

    def add(o, u2=None):
        u2 = rng.uniform(0, 1, 2) if u2 is None else u2
        q.append([*o, *u2, rng.uniform(0, 0.9999)])

    def unit():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v)

    centre = np.array([0.0, 1.0, 1.0])
    for k in range(9):  # the u2 grid from an ordinary origin, far away (1e6), and so far that distance^2 overflows (rejected)
        add(centre + rng.uniform(-0.8, 0.8, 3), grid[k])
        add(1e6 * unit(), grid[k])
        add(1e20 * unit(), grid[(k + 4) % 9])
    for kind, v in shapes:
        a = np.array(v[:9] if len(v) >= 9 else v + [0.0] * 9, dtype=np.float64)
        if kind == "rect":  # p ex ey: exactly in its plane (axis-aligned: the third coordinate is p's), close in front, behind
            p, ex, ey = a[0:3], a[3:6], a[6:9]
            n = np.cross(ex, ey)
            n /= np.linalg.norm(n)
            add(p + 0.25 * ex + 0.125 * ey), add(p + 2.0 * ex - 0.5 * ey), add(p + 1e-3 * n), add(p - 0.5 * n)
        elif kind == "sphere":  # inside (sqrt of a negative), the centre itself (r / 0), close to the surface
            c, r = a[0:3], a[3]
            add(c + 0.5 * r * unit()), add(c), add(c + (r + 1e-3) * unit()), add(c + 0.999 * r * unit(), grid[8])
        elif kind == "disk":  # p n r: the centre and a point of its plane, close, behind
            p, n = a[0:3], a[3:6] / np.linalg.norm(a[3:6])
            t = np.cross(n, [1.0, 0.0, 0.0])
            add(p), add(p + 0.2 * t), add(p + 1e-3 * n), add(p - 0.5 * n)
        elif kind == "triangle":  # a b c: a vertex, the centroid, a point of the plane outside it, close
            va, vb, vc = a[0:3], a[3:6], a[6:9]
            n = np.cross(va - vb, va - vc)
            n /= np.linalg.norm(n)
            add(va), add((va + vb + vc) / 3), add(va + 2.0 * (vb - va) + 1.5 * (vc - va)), add((va + vb + vc) / 3 + 1e-3 * n)
        elif kind == "line":  # a b thickness: on the axis (inside and beyond the end), close
            va, vb = a[0:3], a[3:6]
            add(0.5 * (va + vb)), add(va), add(va - 0.5 * (vb - va)), add(0.5 * (va + vb) + (a[6] + 1e-3) * unit())
        elif kind == "plane":  # p n: in the plane, behind
            p, n = a[0:3], a[3:6]
            t = np.cross(n, [0.3, 0.2, 0.9])
            add(p + t), add(p - 0.5 * n)
        elif kind in ("mesh", "mesh_full"):  # nv nt vertices...: a vertex, the first triangle's centroid
            vs = np.array(v[2:11], dtype=np.float64).reshape(3, 3)
            add(vs[0]), add(vs.mean(axis=0))
    # Triangle::sample's fold at u.x + u.y > 1: sums of 1 - ulp, 1 and 1 + ulp
    for uy in (0.75 - 2.0 ** -24, 0.75, 0.75 + 2.0 ** -23):
        for _ in range(3):
            add(centre + rng.uniform(-0.8, 0.8, 3), (0.25, uy))
    assert len(q) <= 200, len(q)
    while len(q) < 256:  # random origins around the scene
        add(centre + rng.uniform(-1.5, 1.5, 3))
    out = np.array(q, dtype=np.float64).astype(F32)
    # u1 must keep the reference's own int(nt * u1) below nt (an index past the end is undefined behaviour there)
    for kind, v in shapes:
        if kind in ("mesh", "mesh_full"):
            assert (np.floor(F32(v[1]) * out[:, 5]) < v[1]).all()
    return out


# ---- the cap that keeps a fixture from hiding a failure: NaN share and outcome classes, asserted by the generator on the
# reference's records and by the tests on the stored ones ----------------------------------------------------------------
NAN_SHARE = 0.05
CLASS_MIN = 8
# which lobes can reach a class: a Diffuse / BSSRDF sample always exists and is never a delta; Diffuse stays on wi's side and
# the BSSRDF goes to the other; only RefractiveDielectric refracts, and DiffusiveDielectric's diffuse lobe is not flipped to
# wi's side (wi below the surface gives wo above it)
BXDF_CLASSES = {"absent": (1, 2, 3, 4), "delta": (1, 2, 3, 4), "reflected": (0, 1, 2, 3, 4), "transmitted": (3, 4, 5),
                "f_zero": (0, 1, 2, 3, 4, 5), "f_nonzero": (0, 1, 2, 3, 4, 5)}
# a Plane's pdf is the constant 1 / 2pi: never rejected; Cone::sample returns nothing and a box's sample leaves pdf = 0
SHAPE_ACCEPTS = ("rect", "sphere", "disk", "plane", "line", "triangle", "mesh")
SHAPE_REJECTS = ("rect", "box", "obb", "sphere", "disk", "cone", "line", "triangle", "mesh")


def bxdf_ledger(cases, rec):
    """-> {lobe: {class: count, 'nan': share of records with a NaN, 'cases': n}} of reference records."""
    out = {}
    for lobe in range(6):
        m = cases[:, 0] == lobe
        c, r = cases[m], rec[m]
        sampled, has_f = (c[:, 15].astype(int) & 2) != 0, (c[:, 15].astype(int) & 1) != 0
        present = r[:, 5] == 1
        side = r[:, 8] * c[:, 8]
        f_zero = (r[:, 0:3] == 0).all(axis=1)
        out[lobe] = {"cases": int(m.sum()), "nan": float(np.isnan(r).any(axis=1).mean()),
                     "absent": int((sampled & ~present).sum()), "delta": int((present & (r[:, 13] == 1)).sum()),
                     "reflected": int((present & (side > 0)).sum()), "transmitted": int((present & (side < 0)).sum()),
                     "f_zero": int((has_f & f_zero).sum()), "f_nonzero": int((has_f & ~f_zero & ~np.isnan(r[:, 0:3]).any(axis=1)).sum())}
    return out


def check_bxdf_ledger(led):
    for lobe, row in led.items():
        assert row["nan"] <= NAN_SHARE, f"{LOBES[lobe]}: {row['nan']:.3f} of the reference's records hold a NaN"
        for cls, lobes in BXDF_CLASSES.items():
            if lobe in lobes:
                assert row[cls] >= CLASS_MIN, f"{LOBES[lobe]}: only {row[cls]} cases reach '{cls}'"


def shape_ledger(pscene, shape_rec):
    kinds = [k for k, _ in parse_shapes(pscene)[0]]
    out = {}
    for k, r in zip(kinds, shape_rec):
        k = "mesh" if k.startswith("mesh") else k
        row = out.setdefault(k, {"records": 0, "accepted": 0, "rejected": 0, "nan": 0})
        row["records"] += len(r)
        row["accepted"] += int((r[:, 0] == 1).sum())
        row["rejected"] += int((r[:, 0] == 0).sum())
        row["nan"] += int(np.isnan(r).any(axis=1).sum())
    return out


def check_shape_ledger(led):
    for k, row in led.items():
        assert row["nan"] <= NAN_SHARE * row["records"], f"{k}: {row['nan']} of {row['records']} reference records hold a NaN"
        if k in SHAPE_ACCEPTS:
            assert row["accepted"] >= CLASS_MIN, f"{k}: only {row['accepted']} samples accepted"
        if k in SHAPE_REJECTS:
            assert row["rejected"] >= CLASS_MIN, f"{k}: only {row['rejected']} samples rejected"


# ---- comparison ------------------------------------------------------------------------------------------------------
BXDF_FIELDS = [("f", 0, 3), ("pdf", 3, 4), ("is_delta", 4, 5), ("sample present", 5, 6), ("sample wo", 6, 9), ("sample f", 9, 12),
               ("sample pdf", 12, 13), ("sample is_delta", 13, 14)]
SHAPE_FIELDS = [("shape_sample present", 0, 1), ("shape_sample p", 1, 4), ("shape_sample n", 4, 7), ("shape_sample w", 7, 10),
                ("shape_sample distance", 10, 11), ("shape_sample pdf", 11, 12), ("shape_pdf", 12, 13)]
LIGHT_FIELDS = [("light_sample_other present", 0, 1), ("light_sample_other w", 1, 4), ("light_sample_other distance", 4, 5),
                ("light_sample_other pdf", 5, 6), ("light_sample_other le", 6, 9)]


def _hex(row):
    return "[" + ", ".join(float(v).hex() for v in row) + "]"


def mismatches(got, want):
    """Boolean array: bits differ, except that a NaN is wanted and a NaN is there."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(want) & np.isnan(got))


def assert_records(who, got, want, inputs, fields, label):
    """got / want [n, width]; inputs [n, k]; label(i) names the lobe or shape of record i."""
    bad = mismatches(got, want)
    if not bad.any():
        return
    lines = []
    for i in np.flatnonzero(bad.any(axis=1))[:8]:
        name = next(f for f, a, b in fields if bad[i, a:b].any())
        a, b = next((a, b) for f, a, b in fields if f == name)
        lines.append(f"{who}: {name}, {label(i)}, case {i}: inputs {_hex(inputs[i])}\n      got  " +
                     " ".join(f"{w:08x}" for w in got[i, a:b].view(np.uint32)) + f" {_hex(got[i, a:b])}\n      want " +
                     " ".join(f"{w:08x}" for w in want[i, a:b].view(np.uint32)) + f" {_hex(want[i, a:b])}")
    raise AssertionError(f"{int(bad.any(axis=1).sum())} of {len(got)} records differ\n" + "\n".join(lines))


@pytest.fixture(scope="module")
def bxdf_fixture():
    z = np.load(os.path.join(GOLDEN, "bxdf_lobes.npz"))
    return np.ascontiguousarray(z["cases"]), np.ascontiguousarray(z["records"])


@pytest.fixture(scope="module")
def light_fixtures():
    out = {}
    for name in SCENES:
        z = np.load(os.path.join(GOLDEN, f"lightsamples_{name}.npz"))
        out[name] = (str(z["pscene"]), np.ascontiguousarray(z["queries"]), z["shape_records"], z["light_records"])
    return out


def product_bxdf(device, cases):
    from pine_amd import _lib
    out = np.full((2, len(cases), 14), -7.0, F32)
    _lib.check(_lib.lib.pine_gpu_test_bxdf(device, cases.ctypes.data_as(_lib.c_f_p), len(cases), out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_bxdf")
    return out


def product_light_samples(device, scene, queries, ng, nl):
    from pine_amd import _lib
    n = len(queries)
    out = np.full(n * (13 * ng + 9 * nl), -7.0, F32)
    _lib.check(_lib.lib.pine_gpu_test_light_samples(scene._h, device, queries.ctypes.data_as(_lib.c_f_p), n, out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_light_samples")
    return out[:n * 13 * ng].reshape(ng, n, 13), out[n * 13 * ng:].reshape(nl, n, 9)


def _lobe_label(cases):
    return lambda i: f"lobe {LOBES[int(cases[i, 0])]}"


def check_product_bxdf(device, fixture):
    cases, rec = fixture
    got = product_bxdf(device, cases)
    who = "host build" if device < 0 else "device"
    assert_records(f"{who}, every feature (F_ALL)", got[0], rec, cases, BXDF_FIELDS, _lobe_label(cases))
    assert_records(f"{who}, narrowest feature mask", got[1], rec, cases, BXDF_FIELDS, _lobe_label(cases))


def check_product_light_samples(device, name, fixture):
    from pine_amd import scenes
    pscene, queries, srec, lrec = fixture
    scene = SCENES[name](scenes)
    assert scene.describe() == pscene
    kinds = [k for k, _ in parse_shapes(pscene)[0]]
    got_s, got_l = product_light_samples(device, scene, queries, len(srec), len(lrec))
    who = f"{'host build' if device < 0 else 'device'}, {name}"
    n = len(queries)
    assert_records(who, got_s.reshape(-1, 13), srec.reshape(-1, 13), np.tile(queries, (len(srec), 1)), SHAPE_FIELDS,
                   lambda i: f"geometry {i // n} ({kinds[i // n]}), query {i % n}")
    assert_records(who, got_l.reshape(-1, 9), lrec.reshape(-1, 9), np.tile(queries, (len(lrec), 1)), LIGHT_FIELDS,
                   lambda i: f"light {i // n}, query {i % n}")


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_generators_reproduce_the_stored_cases(bxdf_fixture, light_fixtures):
    from pine_amd import scenes
    cases = bxdf_cases()
    assert cases.shape == bxdf_fixture[0].shape and not mismatches(cases, bxdf_fixture[0]).any()
    for name, (pscene, queries, srec, lrec) in light_fixtures.items():
        assert SCENES[name](scenes).describe() == pscene, name
        q = light_queries(pscene)
        assert q.shape == queries.shape and not mismatches(q, queries).any(), name
        shapes, nl = parse_shapes(pscene)
        assert srec.shape == (len(shapes), len(q), 13) and lrec.shape == (nl, len(q), 9), name


def test_nan_cap_and_outcome_classes(bxdf_fixture, light_fixtures):
    cases, rec = bxdf_fixture
    led = bxdf_ledger(cases, rec)
    print(led)
    check_bxdf_ledger(led)
    assert all(row["cases"] >= 1950 for row in led.values())
    total = {}
    for name, (pscene, queries, srec, lrec) in light_fixtures.items():
        for k, row in shape_ledger(pscene, srec).items():
            t = total.setdefault(k, dict.fromkeys(row, 0))
            for key, v in row.items():
                t[key] += v
        assert not np.isnan(lrec).any(), name
    print(total)
    check_shape_ledger(total)
    assert set(total) >= {"rect", "box", "obb", "sphere", "disk", "cone", "plane", "line", "cylinder", "triangle", "mesh"}


def test_oracle_bxdf_equals_reference(oracle, bxdf_fixture):
    cases, rec = bxdf_fixture
    assert_records("oracle", oracle.bxdf(cases), rec, cases, BXDF_FIELDS, _lobe_label(cases))


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_light_samples_equal_reference(oracle, light_fixtures, name):
    pscene, queries, srec, lrec = light_fixtures[name]
    kinds = [k for k, _ in parse_shapes(pscene)[0]]
    got_s, got_l = oracle.light_samples(pscene, queries, len(srec), len(lrec))
    n = len(queries)
    assert_records(f"oracle, {name}", got_s.reshape(-1, 13), srec.reshape(-1, 13), np.tile(queries, (len(srec), 1)), SHAPE_FIELDS,
                   lambda i: f"geometry {i // n} ({kinds[i // n]}), query {i % n}")
    assert_records(f"oracle, {name}", got_l.reshape(-1, 9), lrec.reshape(-1, 9), np.tile(queries, (len(lrec), 1)), LIGHT_FIELDS,
                   lambda i: f"light {i // n}, query {i % n}")


def test_host_build_bxdf_equals_reference(bxdf_fixture):
    check_product_bxdf(-1, bxdf_fixture)


@pytest.mark.parametrize("name", list(SCENES))
def test_host_build_light_samples_equal_reference(light_fixtures, name):
    check_product_light_samples(-1, name, light_fixtures[name])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_bxdf_equals_reference(bxdf_fixture):
    check_product_bxdf(0, bxdf_fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_device_light_samples_equal_reference(light_fixtures, name):
    check_product_light_samples(0, name, light_fixtures[name])
