"""From a material record and a surface point to a lobe, one call at a time: the shading-node programs (node_program_eval on the
device, node_fold / emit_program / compile_node_programs on the host), material_params and choose_lobe -- compared three ways,
bit for bit: the real reference (tests/golden/node_evals.npz and lobe_choice.npz over the scene nodes_zoo.pscene, written by
`pine_ref nodes` / `pine_ref lobes` through tools/make_golden.py --nodes), the CPU oracle (oracle_node_evals / oracle_lobe_choice:
recursive evaluation, nothing folded) and the product (pine_gpu_test_material_params: host build for device = -1 and device build;
pine_gpu_test_choose_lobe: device only, choose_lobe is __device__ code -- the CPU half of the lobe test is oracle against
reference).  include/pine_gpu.h has the layouts.

No tolerance: float bits, except that where the reference's value is a NaN the value under test must be a NaN.  The scene, the
queries and the cases come from the seeded generators below; the fixtures store them and the tests rebuild and compare them.

The reference was asked everything: its lobes' members are public (bxdf.h), so they are read directly; only the SobolSampler's
private `dimension` goes through the member-pointer idiom.  Emissive materials have no lobe there (sample_bxdf is unreachable):
no lobe case names one.  A member a material or a lobe does not have is 0 in the records of all sides."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from test_sampling_fixtures import F32, assert_records, mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_STACK = 8  # kNodeStack, pine_types.h
LOBES = ["Diffuse", "Conductor", "Refractive", "RefractiveDielectric", "DiffusiveDielectric", "BSSRDF"]
# members a material has (material.h): albedo xyz, roughness, metallic, transmission, ior -- the record slots that are compared
SLOTS = {"emissive": (1, 1, 1, 0, 0, 0, 0), "diffuse": (1, 1, 1, 0, 0, 0, 0), "metal": (1, 1, 1, 1, 0, 0, 0),
         "glossy": (1, 1, 1, 1, 0, 0, 1), "glass": (1, 1, 1, 1, 0, 0, 1), "uber": (1, 1, 1, 1, 1, 1, 1), "subsurface": (1, 1, 1, 1, 0, 0, 1)}
NODE_FIELDS = [("albedo", 0, 3), ("roughness", 3, 4), ("metallic", 4, 5), ("transmission", 5, 6), ("ior", 6, 7)]
LOBE_FIELDS = [("lobe", 0, 1), ("albedo", 1, 4), ("roughness", 4, 5), ("ior", 5, 6), ("sampler dimension", 6, 7), ("next RNG float", 7, 8)]


def _na(x, to):
    return float(np.nextafter(F32(x), F32(to)))


ROUGHNESS = [0.0, 0.3, 0.6, _na(0.6, 0), _na(0.6, 1), 1.0]                # around the min_roughness clamp (0.6 once diffused)
PROBS = [0.0, 1.0, _na(0, 1), _na(1, 0), 0.3, 0.7]                        # with_probability draws only strictly inside (0, 1)
PAIRS = [((37 * s + 11) % 1024, (101 * s + 5) % 1024, (7 * s + 3) % 64) for s in range(16)]  # (pixel x, pixel y, sample index)
COSINES = [1.0, 0.9, 0.5, 0.2, 0.05, 1e-3, 1e-6, 0.0]                     # dot(wi, n), both signs


# ---- the scene --------------------------------------------------------------------------------------------------------
def chain(leaves):
    """leaves[0] - (leaves[1] - (... - leaves[-1])): right-leaning, needs len(leaves) stack slots"""
    x = leaves[-1]
    for leaf in reversed(leaves[:-1]):
        x = leaf - x
    return x


def programs(api):
    """-> [(name, f(P, N, U) -> Node3f)]: every program is the albedo of its own Diffuse material.  P, N, U are Position() / Normal() /
    UV() -- or, in a constant twin, constants equal to a query."""
    V3, cb, lerp, of = api.Vec3, api.Checkerboard, api.lerp, api.Node.of
    ops = {"+": lambda a, b: a + b, "-": lambda a, b: a - b, "*": lambda a, b: a * b, "/": lambda a, b: a / b, "^": lambda a, b: a ** b}
    out = []
    for sym, op in ops.items():
        out.append((f"f{sym}f", lambda P, N, U, op=op: V3(op(P[0], N[1]))))
        out.append((f"v{sym}v", lambda P, N, U, op=op: op(P, N)))
        if sym in "-/^":  # both operand orders, distinct operands: a swapped pop shows
            out.append((f"f{sym}f swapped", lambda P, N, U, op=op: V3(op(N[1], P[0]))))
            out.append((f"v{sym}v swapped", lambda P, N, U, op=op: op(N, P)))
    # the splat forms of node.cpp:82-86
    out += [("v*f", lambda P, N, U: P * U[0]), ("f*v", lambda P, N, U: U[0] * P), ("v^f", lambda P, N, U: P ** U[0]),
            ("v/f", lambda P, N, U: P / U[0]), ("f/v", lambda P, N, U: U[0] / P)]
    un = {"-": lambda x: -x, "abs": api.node_abs, "sqr": api.node_sqr, "sqrt": api.node_sqrt, "fract": api.node_fract}
    for name, f in un.items():
        out.append((f"{name} f", lambda P, N, U, f=f: V3(f(P[0]))))
        out.append((f"{name} v", lambda P, N, U, f=f: f(P)))
    for k in range(3):
        out.append((f"comp {k}", lambda P, N, U, k=k: V3(P[k])))
    out.append(("Vec3(x, y, z)", lambda P, N, U: V3(N[0], U[1], P[2])))
    out.append(("Checkerboard(UV)", lambda P, N, U: V3(cb(U))))
    for r in (0.5, 0.95, 0.0, 1.0):
        out.append((f"Checkerboard(P, {r})", lambda P, N, U, r=r: V3(cb(P, r))))
    out += [("lerp(f, f, f)", lambda P, N, U: V3(lerp(U[0], P[1], N[2]))), ("lerp(f, v, v)", lambda P, N, U: lerp(U[0], P, N)),
            ("lerp(v, v, v)", lambda P, N, U: lerp(U, P, N))]
    # mixed trees: a constant subtree (folded on the host with glibc powf / sqrtf) inside a surface-reading one (device ppow / psqrt)
    c1 = lambda: api.node_fract(api.node_sqrt(of(7.3) ** of(1.7)) / of(0.37))  # noqa: E731
    c2 = lambda: of(-2.5) ** of(3.0) / api.node_sqrt(of(0.3))                  # noqa: E731  (a negative base)
    c3 = lambda: V3(of(-0.75) ** of(0.5), api.node_fract(of(-1e-8)), of(2.0) ** of(-0.5))  # noqa: E731  (NaN, 1.0, a fraction)
    out += [("P - c1", lambda P, N, U: P - c1()), ("c1 - P", lambda P, N, U: c1() - P), ("P / c2", lambda P, N, U: P / c2()),
            ("c2 / P", lambda P, N, U: c2() / P), ("P ^ c1", lambda P, N, U: P ** c1()), ("c1 ^ f", lambda P, N, U: V3(c1() ** P[0])),
            ("c3 - N", lambda P, N, U: c3() - N), ("(P - c1) / (c2 - N)", lambda P, N, U: (P - c1()) / (c2() - N))]
    # the stack's edge: exactly kNodeStack slots; kNodeStack - 1 and kNodeStack under a three-argument Vec3
    leaves = lambda P, N, U: [P[0], P[1], P[2], N[0], N[1], N[2], U[0], U[1]]  # noqa: E731
    out += [("chain 8", lambda P, N, U: V3(chain(leaves(P, N, U)))),
            ("Vec3 over chain 5", lambda P, N, U: V3(U[1], N[0], chain(leaves(P, N, U)[:5]))),
            ("Vec3 over chain 6", lambda P, N, U: V3(U[1], N[0], chain(leaves(P, N, U)[:6])))]
    return out


def too_deep(api):
    P, N, U = api.Position(), api.Normal(), api.UV()
    return api.Vec3(chain([P[0], P[1], P[2], N[0], N[1], N[2], U[0], U[1], P[0] * N[0]]))  # kNodeStack + 1 slots


def nodes_zoo():
    """-> (scene, [(name, kind)]) through pine_amd.api: the programs, the node-driven materials with every parameter distinct, and
    the constant-parameter materials of the lobe cases."""
    from pine_amd import api
    sc = api.Scene()
    mats = []

    def add(name, m):
        sc.add(f"m{len(mats)}", m)
        mats.append((name, type(m).__name__.lower()))

    P, N, U = api.Position(), api.Normal(), api.UV()
    for name, f in programs(api):
        add(name, api.Diffuse(f(P, N, U)))
    fr = api.node_fract
    add("metal n", api.Metal(api.node_abs(N), fr(P[0])))
    add("glossy n", api.Glossy(fr(P), fr(U[0] * 3.0), 1.0 + fr(P[2])))
    add("glass n", api.Glass(fr(P), fr(U[1] * 5.0), 1.25 + fr(P[1])))
    add("uber n", api.Uber(fr(P), fr(P[0]), fr(P[1]), fr(P[2]), 1.7))
    add("uber n checker", api.Uber(api.node_abs(N), fr(U[0]), api.Checkerboard(U), api.Checkerboard(P, 0.95), 1.3))
    add("emissive", api.Emissive([3.0, 2.0, 1.0]))
    for i, r in enumerate(ROUGHNESS):
        add(f"metal r={r}", api.Metal([0.9, 0.6, 0.3], r))
        add(f"glossy r={r}", api.Glossy([0.2, 0.5, 0.8], r, 1.3 + 0.1 * i))
        add(f"glass r={r}", api.Glass([0.7, 0.8, 0.9], r, 1.2 + 0.1 * i))
        add(f"subsurface r={r}", api.Subsurface([0.8, 0.4, 0.3], r, [2.0, 4.0, 8.0]))
    for i, m in enumerate(PROBS):
        for j, t in enumerate(PROBS):
            add(f"uber m={m} t={t}", api.Uber([0.5, 0.6, 0.7], ROUGHNESS[(i + j) % 6], m, t, 1.45 + 0.01 * j))
    sc.set(api.ThinLenCamera(api.Film((16, 16)), [0, 1, -4], [0, 1, 0], 0.5))
    return sc, mats


# ---- the queries (p, n, uv) -------------------------------------------------------------------------------------------
EDGE = [0.0, -0.0, 1.0, -1.0, 2.0, -3.0, 7.0, -2.0 ** -24, -1e-8, 0.5, _na(0.5, 0), _na(0.5, 1), 0.95, _na(0.95, 0), _na(0.95, 1),
        1e-16, 2e-16, 0.7e-16, 2.0 ** 23, 2.0 ** 24 + 2, 1e30, -1e30, float("inf"), float("-inf"), float("nan"), 1e-40, -1e-40,
        2.0 ** -149, 2.5, -2.5, 0.3, -0.3, 1.5, 0.25]


def node_queries():
    rng = np.random.default_rng(20261018)
    L = len(EDGE)
    q = []
    for k in range(5):  # every edge value in every component, beside other edge values
        for i in range(L):
            e = lambda a, b: EDGE[(a * i + b + 3 * k) % L]  # noqa: E731
            q.append([e(1, 0), e(1, 1 + k), e(1, 2 + 2 * k), e(3, 1), e(5, 2), e(7, 3), e(11, 4), e(1, k)])
    # a product of three factors around 1e-16 underflows to 0 (Checkerboard with ratio 0); exact zeros of a factor; fract = 1
    q += [[1e-16, 2e-16, 0.7e-16, 0, 1, 0, 1e-16, 2e-16], [-1e-16, -2e-16, 0.7e-16, 0, 1, 0, 0.5, 0.5], [0.5, 0.25, 0.75, 0, 1, 0, 0.5, 0.25],
          [0.95, 0.25, 0.75, 0, 0, 1, 0.95, 0.5], [1.5, 2.5, -0.5, 1, 0, 0, 1.95, -0.05], [-2.0 ** -24, -1e-8, -2.0 ** -25, 0, 1, 0, -1e-8, -2.0 ** -24],
          [3.0, -4.0, 5.0, 0, 0, -1, 2.0, -7.0]]
    # negative bases with integer, half-integer and fractional exponents (p ^ n, and n ^ p swapped); 0^0, 0/0, x/0
    for b in (-2.0, -0.5, -8.0, -0.0, 0.0):
        for x in (3.0, 2.0, -3.0, 2.5, -0.5, 0.3, 1.0 / 3.0, 0.0):
            q.append([b, b, b, x, x, x, 0.5, -x])
    assert len(q) <= 230, len(q)
    while len(q) < 480:
        n = rng.normal(size=3)
        q.append([*rng.uniform(-3, 3, 3), *(n / np.linalg.norm(n)), *rng.uniform(0, 1, 2)])
    return np.array(q, dtype=np.float64).astype(F32)


TWIN_QUERIES = list(range(0, 170, 17)) + [171, 172, 175, 180, 200, 231, 300, 400][:6]  # 16 of the queries, edge ones first


def twin_programs(api):
    """about 30 of the programs: what the host's fold and the device's evaluator both have to get right"""
    skip = ("chain", "Vec3 over", "comp 1", "comp 2", "swapped", "lerp(f, f, f)", "f+f", "f*f", "v+v", "abs", "- f")
    return [(i, name, f) for i, (name, f) in enumerate(programs(api)) if not any(s in name for s in skip)]


# ---- the lobe cases ---------------------------------------------------------------------------------------------------
def lobe_cases(mats):
    rng = np.random.default_rng(4242)
    rows = []

    def basis(n):
        t = np.cross(n, [0.3, -0.5, 0.8])
        return t / np.linalg.norm(t)

    def add(m, s, diffused, cos=None):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        c = COSINES[s % 8] * (1.0 if s < 8 else -1.0) if cos is None else cos
        wi = c * n + np.sqrt(max(0.0, 1.0 - c * c)) * basis(n)
        rows.append([m, *rng.uniform(-2, 2, 3), *n, *rng.uniform(0, 1, 2), *wi, diffused, *PAIRS[s]])

    for m, (name, kind) in enumerate(mats):
        if kind == "emissive":
            continue
        constant = "=" in name
        for diffused in (0, 1):
            for s in range(16 if constant or kind != "diffuse" else 3):
                add(m, s, diffused)
    # the pixel RNG's first float of every pair, through a material that draws nothing (the first program)
    for s in range(16):
        add(0, s, 0)
    return np.array(rows, dtype=np.float64).astype(F32)


def lobe_ledger(mats, cases, rec):
    """-> {class: count} of reference records"""
    first = {tuple(int(v) for v in c[13:16]): r[7] for c, r in zip(cases[-16:], rec[-16:])}
    out = {}

    def count(key):
        out[key] = out.get(key, 0) + 1

    for c, r in zip(cases, rec):
        name, kind = mats[int(c[0])]
        count(f"{kind}: {LOBES[int(r[0])]}")
        if kind == "uber":
            count("uber: drew" if r[7].tobytes() != first[tuple(int(v) for v in c[13:16])].tobytes() else "uber: drew nothing")
        if kind == "subsurface":
            count(f"subsurface: sampler dimension {int(r[6])}")
        if "r=" in name and int(r[0]) in (1, 2, 3, 4):
            rough = F32(float(name.split("r=")[1].split()[0]))
            count(f"{kind}: clamp active" if r[4] != rough else f"{kind}: clamp inactive")
    return out


LOBE_CLASSES = (["diffuse: Diffuse", "metal: Conductor", "glossy: DiffusiveDielectric", "glass: RefractiveDielectric", "uber: Conductor",
                 "uber: RefractiveDielectric", "uber: DiffusiveDielectric", "subsurface: Refractive", "subsurface: Diffuse", "subsurface: BSSRDF",
                 "uber: drew", "uber: drew nothing", "subsurface: sampler dimension 1"] +
                [f"{k}: clamp {a}" for k in ("metal", "glossy", "glass", "subsurface") for a in ("active", "inactive")])
CLASS_MIN = 8


def check_lobe_ledger(led):
    for cls in LOBE_CLASSES:
        assert led.get(cls, 0) >= CLASS_MIN, f"only {led.get(cls, 0)} cases reach '{cls}'"
    assert not [k for k in led if k.startswith("uber: ") and k.split(": ")[1] in ("Diffuse", "Refractive", "BSSRDF")], led


# ---- fixtures and the product's side ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo():
    sc, mats = nodes_zoo()
    return sc, mats, open(os.path.join(GOLDEN, "nodes_zoo.pscene")).read()


@pytest.fixture(scope="module")
def node_fixture():
    z = np.load(os.path.join(GOLDEN, "node_evals.npz"))
    return np.ascontiguousarray(z["queries"]), np.ascontiguousarray(z["records"])


@pytest.fixture(scope="module")
def lobe_fixture():
    z = np.load(os.path.join(GOLDEN, "lobe_choice.npz"))
    return np.ascontiguousarray(z["cases"]), np.ascontiguousarray(z["records"])


def node_programs(scene):
    """-> (prog[materials, 4], ops[n, 4] int32 words) or raises PineError"""
    import ctypes as C
    from pine_amd import _lib
    n = _lib.check(_lib.lib.pine_gpu_test_node_programs(scene._h, None, 0), "node programs")
    out = np.zeros(n, np.int32)
    assert _lib.lib.pine_gpu_test_node_programs(scene._h, out.ctypes.data_as(C.POINTER(C.c_int32)), n) == n
    nm = int(out[0])
    return out[2:2 + 4 * nm].reshape(nm, 4), out[2 + 4 * nm:].reshape(int(out[1]), 4)


def material_params(scene, device, queries, nm):
    from pine_amd import _lib
    out = np.full((nm, len(queries), 10), -7.0, F32)
    _lib.check(_lib.lib.pine_gpu_test_material_params(scene._h, device, queries.ctypes.data_as(_lib.c_f_p), len(queries),
                                                      out.ctypes.data_as(_lib.c_f_p)), "pine_gpu_test_material_params")
    return out


def masked(rec, mats):
    """the slots each material has; the others are 0 in the reference's layout"""
    mask = np.array([SLOTS[k] for _, k in mats], F32)[:, None, :]
    return np.where(mask != 0, rec, F32(0)).astype(F32)


def _label(mats, n):
    return lambda i: f"material {i // n} ({mats[i // n][0]}), query {i % n}"


def check_product_node_evals(device, zoo, node_fixture):
    sc, mats, _ = zoo
    queries, rec = node_fixture
    got = material_params(sc, device, queries, len(mats))
    who = "host build" if device < 0 else "device"
    seven = masked(got[:, :, [0, 1, 2, 6, 7, 8, 9]], mats)
    n = len(queries)
    assert_records(who, seven.reshape(-1, 7), rec.reshape(-1, 7), np.tile(queries, (len(mats), 1)), NODE_FIELDS, _label(mats, n))
    # albedo / Pi is the same IEEE division, on the host for a literal and where the program runs for a program
    want = (rec[:, :, 0:3] / F32(np.pi)).astype(F32)
    assert_records(who + ", albedo / Pi", got[:, :, 3:6].reshape(-1, 3), want.reshape(-1, 3), np.tile(queries, (len(mats), 1)),
                   [("albedo / Pi", 0, 3)], _label(mats, n))


def check_constant_twins(device, node_fixture):
    """The same tree with Position / Normal / UV replaced by constants equal to a query: the host folds it whole into the material
    record (glibc powf / sqrtf), and it must equal the reference's evaluation of the original at that query."""
    from pine_amd import api
    queries, rec = node_fixture
    sc = api.Scene()
    want, label = [], []
    for qi in TWIN_QUERIES:
        q = [float(v) for v in queries[qi]]
        P, N, U = api.Node.of(q[0:3]), api.Node.of(q[3:6]), api.Node.of([q[6], q[7], 0.0])
        for i, name, f in twin_programs(api):
            sc.add(f"t{len(want)}", api.Diffuse(f(P, N, U)))
            want.append(rec[i, qi, 0:3])
            label.append(f"twin of '{name}' at query {qi}")
    prog, ops = node_programs(sc)
    assert len(ops) == 0 and (prog == -1).all(), "a constant tree was not folded"
    got = material_params(sc, device, queries[:1], len(want))[:, 0, 0:3]
    assert len(want) >= 400
    assert_records("constant twins, " + ("host build" if device < 0 else "device"), got, np.array(want, F32), np.zeros((len(want), 1), F32),
                   [("albedo", 0, 3)], lambda i: label[i])


def choose_lobe(scene, cases):
    from pine_amd import _lib
    out = np.full((2, len(cases), 8), -7.0, F32)
    _lib.check(_lib.lib.pine_gpu_test_choose_lobe(scene._h, 0, cases.ctypes.data_as(_lib.c_f_p), len(cases), out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_choose_lobe")
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_generators_reproduce_the_stored_cases(zoo, node_fixture, lobe_fixture):
    sc, mats, pscene = zoo
    assert sc.describe() == pscene
    q = node_queries()
    assert q.shape == node_fixture[0].shape and not mismatches(q, node_fixture[0]).any()
    assert node_fixture[1].shape == (len(mats), len(q), 7)
    cases = lobe_cases(mats)
    assert cases.shape == lobe_fixture[0].shape and not mismatches(cases, lobe_fixture[0]).any()
    assert lobe_fixture[1].shape == (len(cases), 8) and len(cases) >= 2000


def test_outcome_classes_all_occur(zoo, node_fixture, lobe_fixture):
    _, mats, _ = zoo
    led = lobe_ledger(mats, *lobe_fixture)
    print(led)
    check_lobe_ledger(led)
    # the node records: most are numbers, and both answers of every Checkerboard occur
    rec = node_fixture[1]
    nan_share = float(np.isnan(rec).any(axis=2).mean())
    print("records with a NaN:", nan_share)
    assert nan_share <= 0.25  # 3 of the 34 edge values are no numbers, and half of the queries are random finite ones
    for m, (name, _) in enumerate(mats):
        if name.startswith("Checkerboard"):
            assert (rec[m, :, 0] == 0).sum() >= CLASS_MIN and (rec[m, :, 0] == 1).sum() >= (0 if name.endswith("1.0)") else CLASS_MIN), name


def test_oracle_node_evals_equal_reference(oracle, zoo, node_fixture):
    _, mats, pscene = zoo
    queries, rec = node_fixture
    got = oracle.node_evals(pscene, queries, len(mats))
    assert_records("oracle", got.reshape(-1, 7), rec.reshape(-1, 7), np.tile(queries, (len(mats), 1)), NODE_FIELDS, _label(mats, len(queries)))


def test_oracle_lobe_choice_equals_reference(oracle, zoo, lobe_fixture):
    _, mats, pscene = zoo
    cases, rec = lobe_fixture
    assert_records("oracle", oracle.lobe_choice(pscene, cases), rec, cases, LOBE_FIELDS, lambda i: f"material {mats[int(cases[i, 0])][0]}")


def test_host_build_node_evals_equal_reference(zoo, node_fixture):
    check_product_node_evals(-1, zoo, node_fixture)
    check_constant_twins(-1, node_fixture)


OVERSIZED = {
    "square_position": "x = api.Position()\nfor _ in range(64): x = x * x\nm = api.Diffuse(x)",
    "square_constant": "x = api.Vec3(api.Node.of(C))\nfor _ in range(64): x = x * x\nm = api.Diffuse(x)",
    "lerp_chain": "t = api.UV()[0]\nfor _ in range(64): t = api.lerp(t, 0.25, 0.75)\nm = api.Diffuse(api.Vec3(t))",
    "one_slot_too_many": "m = api.Diffuse(tnf.too_deep(api))",
}
CHILD = """import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
from pine_amd import api
import test_node_fixtures as tnf
C = float(np.float32(1.0) + np.float32(2.0 ** -23))
{body}
sc = api.Scene()
sc.add("m", m)
try:
    prog, ops = tnf.node_programs(sc)
    print("compiled", len(ops), *[float(v).hex() for v in tnf.material_params(sc, -1, np.zeros((1, 8), np.float32), 1)[0, 0, 0:3]])
except api.PineError as e:
    print("refused:", e)
"""


@pytest.mark.parametrize("case", list(OVERSIZED))
def test_oversized_node_graphs_are_refused_promptly(case):
    """A script's node graph shares operands (the binding memoises nodes): 64 levels of x = x * x are 65 nodes and 2^64 tree
    leaves.  The host does work linear in the number of nodes: the limit of 20 s is a condition, not a measurement."""
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), body=OVERSIZED[case])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=20)
    assert r.returncode == 0, r.stderr
    if case != "square_constant":
        assert r.stdout.startswith("refused:") and "too deep" in r.stdout, r.stdout
        return
    # ... and over a constant the chain folds to what 64 squarings give: numpy float32, and the same chain without sharing
    want = F32(1.0) + F32(2.0 ** -23)
    with np.errstate(over="ignore"):
        for _ in range(64):
            want = F32(want * want)
    assert r.stdout.split() == ["compiled", "0"] + [float(want).hex()] * 3, r.stdout
    from pine_amd import api

    def tree(level, c):
        return api.Vec3(api.Node.of(c)) if level == 0 else tree(level - 1, c) * tree(level - 1, c)

    c = float(F32(1.0) + F32(2.0 ** -23))
    shared = api.Vec3(api.Node.of(c))
    for _ in range(6):
        shared = shared * shared
    sc = api.Scene()
    sc.add("shared", api.Diffuse(shared))
    sc.add("tree", api.Diffuse(tree(6, c)))
    got = material_params(sc, -1, np.zeros((1, 8), F32), 2)[:, 0, 0:3]
    assert not mismatches(got[0], got[1]).any() and got[0, 0] != 1


def test_node_programs_of_the_film_scenes_are_unchanged():
    """The DNodeOp arrays of the two film scenes with node graphs, word for word as recorded before shared operands were memoised."""
    from pine_amd import scenes
    for name, build in (("mats_zoo", lambda: scenes.materials_zoo((64, 64))),
                        ("classic_checker", lambda: scenes.classic_cones((90, 45), 8, checker_floor=True))):
        z = np.load(os.path.join(GOLDEN, f"node_programs_{name}.npz"))
        sc = build()
        assert sc.describe() == str(z["pscene"]), name
        prog, ops = node_programs(sc)
        assert np.array_equal(prog, z["prog"]) and np.array_equal(ops, z["ops"]), name


def test_api_refuses_what_the_reference_refuses():
    """NodeComponent outside 0..2 (node.h:181-182), Nodef / Node3f mismatches (no such overload in node.cpp:29-116) -- and a node
    given to an Emissive or a Subsurface material: the reference takes one there, but the C ABI has no node-driven entry point
    for them, so the binding refuses where it would otherwise try to read the node as three numbers."""
    from pine_amd import _lib, api
    P = api.Position()
    for bad in (lambda: P[3], lambda: P[-1], lambda: P[0][0], lambda: api.Vec3(P), lambda: api.Vec3(P[0], P, P[1])):
        with pytest.raises(api.PineError):
            bad()
    for m in (api.Metal(P, P), api.Glossy(P, 0.5, P), api.Uber(P, 0.5, P), api.Emissive(P), api.Emissive(P * 2.0),
              api.Subsurface(P, 0.5, [1, 1, 1]), api.Subsurface([1, 1, 1], P[0], [1, 1, 1])):
        with pytest.raises(api.PineError):
            api.Scene().add("m", m)
    sc = api.Scene()
    h, lib = sc._h, _lib.lib
    f, v = lib.pine_gpu_scene_node_constf(h, 0.5), lib.pine_gpu_scene_node_input(h, 0)
    assert f >= 0 and v >= 0
    for rc in (lib.pine_gpu_scene_node_component(h, v, 3), lib.pine_gpu_scene_node_component(h, v, -1), lib.pine_gpu_scene_node_component(h, f, 0),
               lib.pine_gpu_scene_node_binary(h, ord("+"), f, v), lib.pine_gpu_scene_node_binary(h, ord("%"), f, f),
               lib.pine_gpu_scene_node_to_vec3(h, v, -1, -1), lib.pine_gpu_scene_node_to_vec3(h, f, f, v), lib.pine_gpu_scene_node_checkerboard(h, f, 0.5),
               lib.pine_gpu_scene_node_splat(h, v), lib.pine_gpu_scene_node_unary(h, ord("a"), 99),
               lib.pine_gpu_scene_add_material_diffuse_n(h, b"m", f), lib.pine_gpu_scene_add_material_metal(h, b"m", v, v)):
        assert rc < 0 and _lib.last_error()


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_node_evals_equal_reference(zoo, node_fixture):
    check_product_node_evals(0, zoo, node_fixture)
    check_constant_twins(0, node_fixture)


@pytest.fixture(scope="module")
def device_lobes(zoo, lobe_fixture):
    return choose_lobe(zoo[0], lobe_fixture[0])


@pytest.mark.gpu
def test_device_lobe_choice_equals_reference(zoo, lobe_fixture, device_lobes):
    _, mats, _ = zoo
    cases, rec = lobe_fixture
    assert_records("device, after_walk = 0", device_lobes[0], rec, cases, LOBE_FIELDS, lambda i: f"material {mats[int(cases[i, 0])][0]}")


@pytest.mark.gpu
def test_after_walk_is_a_bssrdf_and_draws_nothing(zoo, lobe_fixture, device_lobes):
    """The product's own split of the BSSRDF case: a Subsurface vertex that resumes after its walk is a BSSRDF with the material's
    ior, and takes neither a sampler dimension nor an RNG float; every other material answers as it did before."""
    _, mats, _ = zoo
    cases, rec = lobe_fixture
    sss = np.array([mats[int(c[0])][1] == "subsurface" for c in cases])
    assert sss.sum() >= 100
    first = {tuple(int(v) for v in c[13:16]): r[7] for c, r in zip(cases[-16:], rec[-16:])}
    after = device_lobes[1]
    want = np.array([[5, 0.8, 0.4, 0.3, 0, 1.4, 0, first[tuple(int(v) for v in c[13:16])]] for c in cases[sss]], F32)
    want[:, 1:4] = np.array([0.8, 0.4, 0.3], F32)
    assert_records("device, after_walk = 1, Subsurface", after[sss], want, cases[sss], LOBE_FIELDS, lambda i: "subsurface")
    assert_records("device, after_walk = 1, others", after[~sss], rec[~sss], cases[~sss], LOBE_FIELDS, lambda i: "not subsurface")
