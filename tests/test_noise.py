"""Noise nodes (Noisef / Noise3f = NodeNoisef / NodeNoise3f, the reference's fbm) on the host build: material_params against
records made by the real reference (tools/make_golden_noise.py), bit for bit; the host's fold of constant operands; the bound
on the octave loop; the ABI's refusals; the .pscene lines; the Python front; PRL."""
import json
import os
import time

import numpy as np
import pytest

import noise_scenes as X
from test_texture import SLOTS, _lib, assert_records, material_params, pa

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
KINDS = {"diffuse_n": "diffuse", "uber_n": "uber", "metal": "metal", "glossy": "glossy", "glass": "glass"}


@pytest.fixture(scope="module")
def zoo_fixture():
    fx = np.load(os.path.join(GOLDEN, "noise_zoo.npz"))
    return fx["queries"], fx["records"], bytes(fx["pscene"]).decode()


@pytest.fixture(scope="module")
def zoo(zoo_fixture):
    sc, names = X.noise_zoo(zoo_fixture[0])
    kinds = [KINDS[ln.split()[2]] for ln in sc.describe().splitlines() if ln.startswith("material ")]
    return sc, list(zip(names, kinds))


def check_records(device, zoo, zoo_fixture):
    """Bitwise on every material but the oct0_* ones, whose noise-driven slots are 0 / 0: a NaN with whatever bits the
    hardware gives (x86 and gfx950 differ in the sign), so there: NaN where the reference has NaN, bits elsewhere."""
    sc, mats = zoo
    queries, want, _ = zoo_fixture
    assert want.shape == (len(mats), X.NUM_QUERIES, 10)
    got = material_params(sc, device, queries, len(mats))
    who = "host build" if device < 0 else "device"
    oct0 = [i for i, (name, _) in enumerate(mats) if name.startswith("oct0_")]
    assert len(oct0) == 2 and oct0 == [len(mats) - 2, len(mats) - 1]
    assert_records(who, got[:-2], want[:-2], mats[:-2], queries)
    for i in oct0:
        nan = np.isnan(want[i])
        mask = np.array(SLOTS[mats[i][1]], bool)[None, :]
        assert nan.any(axis=1).all(), "the fixture's oct0 records hold a NaN at every query"
        assert np.array_equal(np.isnan(got[i]) & mask, nan & mask), f"{who}: {mats[i][0]}: NaN where the reference has NaN, and only there"
        bad = (got[i].view(np.uint32) != want[i].view(np.uint32)) & mask & ~nan
        assert not bad.any(), f"{who}: {mats[i][0]}: {int(bad.any(axis=1).sum())} records differ outside the NaN slots"


def test_host_records_equal_the_references(zoo, zoo_fixture):
    check_records(-1, zoo, zoo_fixture)


def test_the_fixture_is_the_scene_the_test_builds(zoo, zoo_fixture):
    queries, _, pscene = zoo_fixture
    assert zoo[0].describe() == pscene
    assert np.array_equal(queries.view(np.uint32), X.queries().view(np.uint32))
    listing = json.load(open(os.path.join(GOLDEN, "noise.json")))
    assert listing["calls"]["materials"] == len(zoo[1]) and listing["calls"]["queries"] == len(queries)
    assert listing["calls"]["differ_with_float_interp"] >= 16  # the fixture tells perlin_interp's binary64 step from a binary32 one


def test_constant_twins_fold_and_equal_their_originals(zoo, zoo_fixture):
    sc, mats = zoo
    queries, want, _ = zoo_fixture
    from test_node_fixtures import node_programs
    prog, _ = node_programs(sc)
    tw = X.twins()
    first = tw[0][0]
    assert (prog[:first] >= 0).any(axis=1).all() and (prog[first:first + len(tw)] == -1).all(), "a constant noise node was not folded (or a surface-reading one was)"
    got = material_params(sc, -1, queries[:1], len(mats))
    q = slice(X.TWIN_QUERY, X.TWIN_QUERY + 1)
    for t, o in tw:
        assert mats[t][0] == "twin of " + mats[o][0]
        assert_records(f"{mats[t][0]}", got[t:t + 1], want[o:o + 1, q], mats[t:t + 1], queries[q])


def test_noisef_is_component_0_of_noise3f(zoo_fixture):
    queries = zoo_fixture[0]
    P = pa.Position()
    sc = pa.Scene()
    for i, o in enumerate((1, 4, X.varying_octaves(pa, P))):
        sc.add(f"f{i}", pa.Metal([0.5, 0.5, 0.5], pa.Noisef(P * 1.7, o)))
        sc.add(f"c{i}", pa.Metal([0.5, 0.5, 0.5], pa.Noise3f(P * 1.7, o)[0]))
    got = material_params(sc, -1, queries, 6)
    for k in (0, 2, 4):
        assert np.isfinite(got[k, :, 6]).all() and len(np.unique(got[k, :, 6])) > 300
        assert np.array_equal(got[k, :, 6].view(np.uint32), got[k + 1, :, 6].view(np.uint32))


def _rounds(octaves_node, p):
    """Noisef(p, octaves_node)'s roughness record at the queries p (n, 8), host build."""
    sc = pa.Scene()
    sc.add("m", pa.Metal([0.5, 0.5, 0.5], pa.Noisef(pa.Position(), octaves_node)))
    return material_params(sc, -1, p, 1)[0, :, 6]


def test_the_octave_loop_is_bounded(zoo_fixture):
    """A non-constant octaves value of 1e9, +inf and NaN returns at once: 32, 32 and 0 rounds (kNoiseMaxOctaves = 32)."""
    q = np.ascontiguousarray(zoo_fixture[0][100:164])
    assert (q[:, 6] != 0).all()
    u = pa.UV()[0]
    cases = [(u * 0.0 + 1e9, 32.0), (pa.node_abs(u) / 0.0, 32.0), ((u - u) / (u - u), 0.0)]
    t0 = time.perf_counter()
    for node, same_as in cases:
        got, want = _rounds(node, q), _rounds(u * 0.0 + same_as, q)
        if same_as:
            assert np.isfinite(want).all()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        else:
            assert np.isnan(got).all() and np.isnan(want).all()
    assert time.perf_counter() - t0 < 5.0  # (1e9 rounds of 64 queries would take hours)
    # (round 25 and later add nothing a binary32 sum can hold, so no result tells 32 rounds from more: what the bound buys is
    # the return.)  The value truncates: 2.9 runs 2 rounds, not 3, and -0.5 none
    assert not np.array_equal(_rounds(u * 0.0 + 3.0, q).view(np.uint32), _rounds(u * 0.0 + 2.0, q).view(np.uint32))
    assert np.array_equal(_rounds(u * 0.0 + 2.9, q).view(np.uint32), _rounds(u * 0.0 + 2.0, q).view(np.uint32))
    assert np.isnan(_rounds(u * 0.0 - 0.5, q)).all()


# ---- the ABI's refusals ------------------------------------------------------------------------------------------------------
def _refused(rc, message):
    assert rc < 0
    assert message in _lib.last_error(), _lib.last_error()


def test_refusals():
    lib, sc = _lib.lib, pa.Scene()
    h = sc._h
    p3 = _lib.check(lib.pine_gpu_scene_node_input(h, 0), "position")
    of = _lib.check(lib.pine_gpu_scene_node_constf(h, 3.0), "constf")
    for fn, who in ((lib.pine_gpu_scene_node_noisef, "`Noisef`"), (lib.pine_gpu_scene_node_noise3f, "`Noise3f`")):
        _refused(fn(h, of, of), who + ": p must be a Node3f")
        _refused(fn(h, p3, p3), who + ": octaves must be a Nodef")
        _refused(fn(h, 99, of), who + ": operand id out of range")
        _refused(fn(h, p3, -1), who + ": operand id out of range")
        for bad, message in ((33.0, "constant octaves is above 32"), (1e9, "constant octaves is above 32"), (np.inf, "constant octaves is not finite"),
                             (-np.inf, "constant octaves is not finite"), (np.nan, "constant octaves is not finite")):
            _refused(fn(h, p3, _lib.check(lib.pine_gpu_scene_node_constf(h, bad), "constf")), who + ": " + message)
        # a constant subtree counts as a constant
        big = _lib.check(lib.pine_gpu_scene_node_binary(h, ord("*"), of, _lib.check(lib.pine_gpu_scene_node_constf(h, 11.0), "constf")), "binary")
        _refused(fn(h, p3, big), who + ": constant octaves is above 32")
        for fine in (32.0, 32.9 - 0.9, 0.0, -0.5):
            _lib.check(fn(h, p3, _lib.check(lib.pine_gpu_scene_node_constf(h, fine), "constf")), "node")
    assert lib.pine_gpu_scene_node_is_vec3(h, _lib.check(lib.pine_gpu_scene_node_noisef(h, p3, of), "node")) == 0
    assert lib.pine_gpu_scene_node_is_vec3(h, _lib.check(lib.pine_gpu_scene_node_noise3f(h, p3, of), "node")) == 1


# ---- .pscene -----------------------------------------------------------------------------------------------------------------
def _nodes_of(text):
    return [ln for ln in text.splitlines() if ln.startswith("node ")]


def _rebuild(text):
    """A scene from the node and material lines of a .pscene text, through the C ABI (the kinds this file's scenes use)."""
    lib, sc = _lib.lib, pa.Scene()
    h = sc._h
    for ln in text.splitlines():
        w = ln.split()
        if w[:1] == ["node"]:
            kind, a = w[2], w[3:]
            if kind == "constf":
                r = lib.pine_gpu_scene_node_constf(h, float.fromhex(a[0]))
            elif kind == "const3":
                r = lib.pine_gpu_scene_node_const3(h, (_lib.C.c_float * 3)(*[float.fromhex(v) for v in a]))
            elif kind in ("position", "normal", "uv"):
                r = lib.pine_gpu_scene_node_input(h, ("position", "normal", "uv").index(kind))
            elif kind in ("binf", "bin3"):
                r = lib.pine_gpu_scene_node_binary(h, ord(a[0]), int(a[1]), int(a[2]))
            elif kind in ("unf", "un3"):
                r = lib.pine_gpu_scene_node_unary(h, ord(a[0]), int(a[1]))
            elif kind == "comp":
                r = lib.pine_gpu_scene_node_component(h, int(a[0]), int(a[1]))
            elif kind == "tovec3":
                r = lib.pine_gpu_scene_node_to_vec3(h, int(a[0]), int(a[1]) if len(a) == 3 else -1, int(a[2]) if len(a) == 3 else -1)
            elif kind == "splat":
                r = lib.pine_gpu_scene_node_splat(h, int(a[0]))
            elif kind == "noisef":
                r = lib.pine_gpu_scene_node_noisef(h, int(a[0]), int(a[1]))
            elif kind == "noise3f":
                r = lib.pine_gpu_scene_node_noise3f(h, int(a[0]), int(a[1]))
            else:
                raise AssertionError("unexpected node kind " + kind)
            assert _lib.check(r, ln) == int(w[1])
    return sc


def test_pscene_lines_round_trip(zoo_fixture):
    sc = pa.Scene()
    P = pa.Position()
    sc.add("m", pa.Metal(pa.Noise3f(P, 3), pa.Noisef(pa.UV() * 2.0, X.varying_octaves(pa, P))))
    nodes = _nodes_of(sc.describe())
    assert nodes[:3] == ["node 0 position", "node 1 constf 0x1.8p+1", "node 2 noise3f 0 1"]
    assert nodes[-1].split()[2] == "noisef" and len(nodes[-1].split()) == 5
    assert _nodes_of(_rebuild(sc.describe()).describe()) == nodes
    # ... and the whole zoo: every node line, the two new kinds among them, reads back as the node it describes
    text = zoo_fixture[2]
    assert sum(ln.split()[2] == "noisef" for ln in _nodes_of(text)) >= 10 and sum(ln.split()[2] == "noise3f" for ln in _nodes_of(text)) >= 10
    assert _nodes_of(_rebuild(text).describe()) == _nodes_of(text)


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_python_overloads():
    f, v = pa.Noisef(pa.Position(), 3), pa.Noise3f([0.1, 0.2, 0.3], 2.5)
    assert not f.is_vec3 and v.is_vec3
    assert f.args[1].kind == "constf" and v.args[0].kind == "const3"  # numbers become constants
    assert pa.Noisef(pa.UV()[0], 2).args[0].kind == "splat"  # a Nodef where the Node3f is expected: Node3f(Nodef), node.h:78
    with pytest.raises(pa.PineError, match="a Nodef is required"):
        pa.Noisef(pa.Position(), pa.UV())
    sc = pa.Scene()
    sc.add("m", pa.Metal(v * 2.0, f ** 2.0))
    text = sc.describe()
    assert " noisef " in text and " noise3f " in text
    with pytest.raises(pa.PineError, match="`Noise3f`: constant octaves is above 32"):
        pa.Scene().add("m", pa.Diffuse(pa.Noise3f(pa.Position(), 40)))


# ---- PRL ---------------------------------------------------------------------------------------------------------------------
def _prl():
    from pine_amd import prl
    return prl


def _script():
    root = os.path.dirname(os.path.dirname(GOLDEN))
    return open(os.path.join(root, "examples", "noise.pine")).read()


def test_prl_example_builds_the_python_scene():
    """examples/noise.pine builds the scene noise_scenes.script_room builds, line for line -- the scene of the fixture."""
    prl = _prl()
    ps, spp, depth = prl.scene_of_dry_run(prl.interpret(_script(), dry_run=True))
    assert (ps, spp, depth) == (X.script_room().describe(), 8, 4)
    name = "noise_script_room_48x32_s8_d4"
    assert ps == bytes(np.load(os.path.join(GOLDEN, f"noise_film_{name}.npz"))["pscene"]).decode()
    assert "BVH()" in _script()


def _prl_scene(body):
    prl = _prl()
    src = ("world := Scene();\n" + body + "\nworld.add(Sphere([0, 0, 0], 1.0), \"m\");\n"
           "world.set(ThinLenCamera(Film([8, 8], Uncharted2()), [0, 0, -3], [0, 0, 0], 0.5));\n"
           "PathIntegrator(BVH(), BlueSampler(1), UniformLightSampler(), 1).render(world);\n")
    return prl.scene_of_dry_run(prl.interpret(src, dry_run=True))[0]


def test_prl_names_and_script_functions_agree_with_the_host_function(zoo_fixture):
    # the node constructors: as Python's
    sc = pa.Scene()
    sc.add("m", pa.Metal(pa.Noise3f(pa.Position() * 2.0, 3), pa.Noisef(pa.UV(), 2)))
    sc.add(pa.Sphere([0, 0, 0], 1.0), "m")
    sc.set(pa.ThinLenCamera(pa.Film([8, 8], pa.Uncharted2()), [0, 0, -3], [0, 0, 0], 0.5))
    assert _prl_scene('world.add("m", Metal(Noise3f(Position() * 2.0, 3), Noisef(UV(), 2)));') == sc.describe()
    # the script functions: a literal the script computed against the host's fold of the same constant node
    p = [float(v) for v in zoo_fixture[0][X.TWIN_QUERY, 0:3]]
    lit = "[" + ", ".join(repr(float(F32(v))) for v in p) + "]"
    folded = pa.Scene()
    folded.add("a", pa.Diffuse(pa.Noise3f(p, 4)))
    folded.add("b", pa.Metal([0.5, 0.5, 0.5], pa.Noisef(p, 3)))
    want = material_params(folded, -1, zoo_fixture[0][:1], 2)
    text = _prl_scene(f'world.add("m", Metal(fbm3d({lit}, 4), fbm({lit}, 3)));')
    node = {int(ln.split()[1]): ln.split()[2:] for ln in text.splitlines() if ln.startswith("node ")}
    mat = [ln.split() for ln in text.splitlines() if ln.startswith("material m ")][0]
    albedo, rough = node[int(mat[3])], node[int(mat[4])]
    assert albedo[0] == "const3" and rough[0] == "constf"
    assert np.array_equal(np.array([float.fromhex(v) for v in albedo[1:]], F32).view(np.uint32), want[0, 0, 0:3].view(np.uint32))
    assert F32(float.fromhex(rough[1])).view(np.uint32) == want[1, 0, 6].view(np.uint32)
    # pnoise / pnoise3d: one round of fbm is sqr(pnoise(p, 0) / 1), and pnoise3d's channels are the seeds 0, 1, 2
    text = _prl_scene(f'world.add("m", Metal(pnoise3d({lit}, 0) * pnoise3d({lit}, 0), pnoise({lit}, 0) * pnoise({lit}, 0)));\n'
                      f'world.add("n", Metal([pnoise({lit}, 0), pnoise({lit}, 1), pnoise({lit}, 2)] * pnoise3d({lit}, 0), fbm({lit}, 1)));')
    node = {int(ln.split()[1]): ln.split()[2:] for ln in text.splitlines() if ln.startswith("node ")}
    m, n = ([ln.split() for ln in text.splitlines() if ln.startswith(f"material {k} ")][0] for k in "mn")
    assert node[int(m[3])] == node[int(n[3])] and node[int(m[4])] == node[int(n[4])]
    one = pa.Scene()
    one.add("a", pa.Diffuse(pa.Noise3f(p, 1)))
    assert np.array_equal(np.array([float.fromhex(v) for v in node[int(m[3])][1:]], F32).view(np.uint32),
                          material_params(one, -1, zoo_fixture[0][:1], 1)[0, 0, 0:3].view(np.uint32))


@pytest.mark.parametrize("call", ["fbm(0.5, 3)", "fbm([0.5, 0.25], 3)", "fbm3d(0.5, 3)", "pnoise(0.5, 0)", "pnoise3d([0.5, 0.25], 0)", "fbm2d([1, 2, 3], 2)"])
def test_prl_refuses_the_other_overloads_by_name(call):
    prl = _prl()
    with pytest.raises(Exception, match=call.split("(")[0]):
        prl.interpret(f"x := {call};\n", dry_run=True)
