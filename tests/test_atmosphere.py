"""Atmosphere on the host: the glibc-exact expf, atmosphere_color, the light's tables, tree and per-call functions (host build),
the refusals, the .pscene line and the front ends, against fixtures made by the real reference
(tools/make_golden_atmosphere.py).  Everything is compared bit for bit; nothing here needs a GPU."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import atmosphere_scenes as A
from test_device_math import ALL, EDGE
from test_envsky import _Lazy, env_records, env_tree, first_difference

pa, _lib = _Lazy("pine_amd"), _Lazy("pine_amd._lib")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
LISTING = json.load(open(os.path.join(GOLDEN, "atmos.json")))
MATH_EXP = 13  # PINE_GPU_MATH_EXP
_scenes = {}


def sky_scene(name, device=None):
    """A scene whose only content is the configuration's Atmosphere (built once per configuration and device)."""
    if (name, device) not in _scenes:
        s = pa.Scene()
        s.set(A.light(name, device))
        _scenes[(name, device)] = s
    return _scenes[(name, device)]


def env_table(scene):
    """(density (h, w), colours (h + 1, w + 1, 3)) of the scene's Atmosphere."""
    n = _lib.check(_lib.lib.pine_gpu_test_env_table(scene._h, None, 0), "pine_gpu_test_env_table")
    out = np.zeros(n, dtype=np.float32)
    _lib.check(_lib.lib.pine_gpu_test_env_table(scene._h, out.ctypes.data_as(_lib.c_f_p), n), "pine_gpu_test_env_table")
    w, h = [int(t) for t in [ln for ln in scene.describe().splitlines() if ln.startswith("envlight")][0].split()[-2:]]
    assert n == w * h + (w + 1) * (h + 1) * 3
    return out[:w * h].reshape(h, w), out[w * h:].reshape(h + 1, w + 1, 3)


def atmosphere_colors(queries, device):
    q = np.ascontiguousarray(queries, dtype=np.float32)
    out = np.zeros((len(q), 3), dtype=np.float32)
    _lib.check(_lib.lib.pine_gpu_test_atmosphere_color(device, q.ctypes.data_as(_lib.c_f_p), len(q), out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_atmosphere_color")
    return out


def exp_sweep(device, first=0, count=ALL, stride=1, cap=8):
    """pexp at first + k * stride (k < count) against the host's expf: (checked, message of the mismatches or None)."""
    stats = np.zeros(4, np.int64)
    ex = np.zeros((cap, 5), np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_math_sweep(device, MATH_EXP, 0, 0, int(first), count, stride, stats.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 ex.ctypes.data_as(C.POINTER(C.c_uint32)), cap), "pine_gpu_test_math_sweep")
    if stats[1] == 0:
        return int(stats[0]), None
    shown = [f"exp({np.uint32(a).view(np.float32)!r} = {a:08x}): got {g:08x}, want {w_:08x}" for a, _, _, g, w_ in ex[:min(cap, int(stats[1]))].tolist()]
    return int(stats[0]), f"{int(stats[1])} mismatches of {int(stats[0])}, max ulp {int(stats[3])}: " + "; ".join(shown)


def test_expf_host_build():
    """The strides of test_device_math.py's host sweeps (251 over all bit patterns), then its edge set, then every argument
    around the four thresholds of e_expf.c's special cases."""
    checked, bad = exp_sweep(-1, first=0x1234567, count=ALL // 251 + 1, stride=251)
    assert bad is None and checked == ALL // 251 + 1, bad
    around = np.concatenate([np.arange(int(t) - 64, int(t) + 64, dtype=np.int64) for t in
                             np.array([88.0, -88.0] + [float.fromhex(t) for t in ("0x1.62e42ep6", "-0x1.9fe368p6", "-0x1.9d1d9ep6")], dtype=np.float32).view(np.uint32)])
    args = np.concatenate([EDGE, around.astype(np.uint32), np.float32([-104.0, 89.0]).view(np.uint32)])
    got, stats, ex = np.zeros(args.size, np.uint32), np.zeros(4, np.int64), np.zeros((8, 5), np.uint32)
    p32 = C.POINTER(C.c_uint32)
    _lib.check(_lib.lib.pine_gpu_test_math_eval(-1, MATH_EXP, args.ctypes.data_as(p32), None, None, args.size, got.ctypes.data_as(p32)), "eval")
    _lib.check(_lib.lib.pine_gpu_test_math_compare(MATH_EXP, args.ctypes.data_as(p32), None, None, got.ctypes.data_as(p32), args.size,
                                                   stats.ctypes.data_as(C.POINTER(C.c_int64)), ex.ctypes.data_as(p32), 8), "compare")
    assert stats[0] == args.size and stats[1] == 0, ex[:int(stats[1])]
    # (the special cases themselves, so that a host libm that changed them is noticed here)
    value = dict(zip(args.tolist(), got.view(np.float32).tolist()))
    assert value[0xff800000] == 0.0 and value[0x7f800000] == np.inf and value[0] == 1.0 and np.isnan(value[0x7fc00000])
    assert value[int(np.float32(-104.0).view(np.uint32))] == 0.0 and value[int(np.float32(89.0).view(np.uint32))] == np.inf


def test_atmosphere_color_equals_the_references():
    fx = np.load(os.path.join(GOLDEN, "atmos_color.npz"))
    assert len(fx["queries"]) == LISTING["color"]["queries"] >= 2000 and set(np.unique(fx["queries"][:, 6])) == {0.0, 1.0}
    assert first_difference(atmosphere_colors(fx["queries"], -1), fx["colors"]) is None
    assert np.array_equal(fx["queries"], A.color_queries())


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_tables_and_tree_equal_the_references(name):
    fx, entry = np.load(os.path.join(GOLDEN, f"atmos_{name}.npz")), LISTING["configs"][name]
    density, colors = env_table(sky_scene(name))
    w, h = A.CONFIGS[name][:2]
    assert density.shape == (h, w) and colors.shape == (h + 1, w + 1, 3)
    assert hashlib.md5(density.tobytes()).hexdigest() == entry["density_md5"]
    tree = env_tree(sky_scene(name))
    assert len(tree) == entry["nodes"]
    assert np.array_equal(tree[:len(fx["tree"])], fx["tree"])
    assert hashlib.md5(tree.tobytes()).hexdigest() == entry["tree_md5"]
    if name in A.SMALL:
        assert first_difference(density, fx["density"]) is None and len(fx["tree"]) == len(tree)
    # the density is the length of the colour at the texel, and a zero-weight half exists
    assert round(float((density == 0).mean()), 4) == entry["zero_density"]
    assert np.isfinite(density).all() and (density >= 0).all()


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_host_records_equal_the_references(name):
    fx = np.load(os.path.join(GOLDEN, f"atmos_{name}.npz"))
    assert fx["queries"].shape == (A.NUM_QUERIES, 5)
    got = env_records(sky_scene(name), fx["queries"], -1)
    assert first_difference(got, fx["records"]) is None


def test_queries_are_the_definitions():
    """The stored queries are atmosphere_scenes.base_queries but for the directions of [384, 448) and the u2 the search found."""
    for name in A.CONFIGS:
        q, base = np.load(os.path.join(GOLDEN, f"atmos_{name}.npz"))["queries"], A.base_queries(name)
        same = np.ones(len(q), dtype=bool)
        same[384:448] = False
        assert np.array_equal(q[same, 2:5].view(np.uint32), base[same, 2:5].view(np.uint32))
        found = LISTING["configs"][name].get("search", {}).get("found", 0)
        same = np.ones(len(q), dtype=bool)
        same[448:448 + found] = False
        assert np.array_equal(q[same, 0:2].view(np.uint32), base[same, 0:2].view(np.uint32))


@pytest.mark.parametrize("name", ["noon", "zenith", "tall"])
def test_color_table_rows_and_columns(name):
    """Every entry of the (w + 1) x (h + 1) table -- row h and column w among them -- is the colour hook's value at the
    direction of sc = (x / w, y / h): uniform_sphere(sc) with y and z swapped, computed here in binary32 by the host's
    libm (the one the device restates)."""
    w, h, sun = A.CONFIGS[name]
    _, colors = env_table(sky_scene(name))
    y, x = np.mgrid[0:h + 1, 0:w + 1]
    # phi = sc.x * Pi * 2, cos_theta = 1 - 2 * sc.y, sin_theta = sqrt(1 - cos_theta^2) (sampling.h:44-50), in binary32
    f = np.float32
    sx, sy = x.astype(f) / f(w), y.astype(f) / f(h)
    phi = sx * f(np.pi) * f(2)
    ct = f(1) - f(2) * sy
    st = np.sqrt(f(1) - ct * ct)
    libm = C.CDLL("libm.so.6")
    libm.sinf.restype = libm.cosf.restype = C.c_float
    libm.sinf.argtypes = libm.cosf.argtypes = [C.c_float]
    sn = np.array([libm.sinf(float(v)) for v in phi.ravel()], dtype=f).reshape(phi.shape)
    cs = np.array([libm.cosf(float(v)) for v in phi.ravel()], dtype=f).reshape(phi.shape)
    d = np.stack([st * cs, ct, st * sn], axis=2).reshape(-1, 3)  # (d.x, d.z, d.y) of uniform_sphere
    s = A.normalized(sun)
    q = np.concatenate([d, np.tile(s, (len(d), 1)), np.ones((len(d), 1), dtype=f)], axis=1)
    want = atmosphere_colors(q, -1).reshape(h + 1, w + 1, 3)
    assert first_difference(colors, want) is None
    # sin(2 pi) is not 0 in binary32: where the sun has a z component column w is not column 0, which is why the table has it
    if sun[2] != 0:
        assert (colors[:h // 2, w] != colors[:h // 2, 0]).any()


def env_light_samples(scene, queries, device):
    """The environment light through the light sampler's own call: per query (p, u2) the 9 floats sampled, w, distance, pdf, le."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    out = np.zeros((len(q), 9), dtype=np.float32)
    _lib.check(_lib.lib.pine_gpu_test_env_light_sample(scene._h, device, q.ctypes.data_as(_lib.c_f_p), len(q), out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_env_light_sample")
    return out


FLOAT_MAX_BITS = 0x7f7fffff  # float_max (src/pine/core/math.h:15)


def two_light_scene(device=None):
    s = pa.Scene()
    s.add(pa.PointLight([0, 1, 0], [1, 1, 1]))
    s.add(pa.Sphere([0, 0, 0], 1.0), pa.Emissive([1, 1, 1]))
    s.set(A.light("noon", device))
    return s


def check_reference_conventions(scene, device):
    """What the light sampler gets from the light: sampled, the record's wo, pdf and le, and distance = float_max bit for bit."""
    fx = np.load(os.path.join(GOLDEN, "atmos_noon.npz"))
    q = np.zeros((A.NUM_QUERIES, 5), dtype=np.float32)
    q[:, 0:3] = fx["queries"][:, 2:5] * np.float32(3)  # (some point p: the light does not read it)
    q[:, 3:5] = fx["queries"][:, 0:2]
    got = env_light_samples(scene, q, device)
    assert (got[:, 0] == 1).all()
    assert (got[:, 4].view(np.uint32) == FLOAT_MAX_BITS).all(), got[:, 4][got[:, 4].view(np.uint32) != FLOAT_MAX_BITS][:4]
    assert first_difference(np.ascontiguousarray(got[:, 1:4]), np.ascontiguousarray(fx["records"][:, 3:6])) is None
    assert first_difference(np.ascontiguousarray(got[:, 5:9]), np.ascontiguousarray(fx["records"][:, [2, 6, 7, 8]])) is None


def test_reference_conventions():
    """sample()'s pdf is ds.pdf / 4 pi, not divided by the light count -- the records of a scene with three lights are those of
    the reference's light alone -- and its distance is float_max."""
    fx = np.load(os.path.join(GOLDEN, "atmos_noon.npz"))
    s = two_light_scene()
    assert first_difference(env_records(s, fx["queries"], -1), fx["records"]) is None
    check_reference_conventions(s, -1)
    # the leaves of the tree tile the image: every texel's pdf is some leaf's
    tree = env_tree(sky_scene("noon"))
    leaves = tree[tree[:, 6] == 1]
    assert ((leaves[:, 4] - leaves[:, 2]) * (leaves[:, 5] - leaves[:, 3])).sum() == 64 * 32


def test_describe_line_and_replacement():
    s = pa.Scene()
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    sky_text = s.describe()
    s.set(pa.ImageSky(np.ones((2, 4, 3), dtype=np.float32)))
    assert s.describe().count("envlight") == 1 and "envlight image 4 2" in s.describe()
    s.set(pa.Atmosphere((0.3, 1.0, 0.2), (4.0, 3.0, 2.5), (16, 8)))
    env = [ln.split() for ln in s.describe().splitlines() if ln.startswith("envlight")]
    assert len(env) == 1 and env[0][:2] == ["envlight", "atmosphere"] and env[0][8:] == ["16", "8"]
    # hex floats; the direction as given, not normalised
    assert [float.fromhex(t) for t in env[0][2:8]] == [float(np.float32(v)) for v in (0.3, 1.0, 0.2, 4.0, 3.0, 2.5)]
    assert len(env_tree(s)) > 1
    s.set(pa.ImageSky(np.ones((2, 4, 3), dtype=np.float32)))
    assert s.describe().count("envlight") == 1 and "envlight image 4 2" in s.describe()
    with pytest.raises(pa.PineError, match="no Atmosphere"):
        env_table(s)
    s.set(pa.Atmosphere((0.3, 1.0, 0.2), (4.0, 3.0, 2.5), (16, 8)))
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    assert s.describe() == sky_text
    with pytest.raises(pa.PineError, match="no ImageSky and no Atmosphere"):
        env_tree(s)
    assert pa.Atmosphere((0, 1, 0), (1, 1, 1)).image_size == (1024, 1024)


def test_refusals():
    s = pa.Scene()
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    before = s.describe()
    for sun, why in (((0.0, 0.0, 0.0), "sun direction is zero"), ((np.nan, 1.0, 0.0), "sun direction is not finite"),
                     ((0.0, np.inf, 0.0), "sun direction is not finite")):
        with pytest.raises(pa.PineError, match=why):
            s.set(pa.Atmosphere(sun, (1, 1, 1), (8, 4)))
    for color in ((np.nan, 1.0, 1.0), (1.0, -np.inf, 1.0)):
        with pytest.raises(pa.PineError, match="sun colour is not finite"):
            s.set(pa.Atmosphere((0, 1, 0), color, (8, 4)))
    for size in ((0, 4), (4, 0), (-1, -1)):
        with pytest.raises(pa.PineError, match="1 x 1"):
            s.set(pa.Atmosphere((0, 1, 0), (1, 1, 1), size))
    with pytest.raises(pa.PineError, match="2\\^22"):
        s.set(pa.Atmosphere((0, 1, 0), (1, 1, 1), (4096, 1025)))
    assert s.describe() == before  # a refused light leaves the scene as it was
    s.set(pa.Atmosphere((0, 1, 0), (1, 1, 1), (1, 1)))  # the smallest
    assert "envlight atmosphere" in s.describe()


def test_oracle_refuses_the_line():
    """The CPU restatement does not cover Atmosphere: it refuses the scene as it refuses any unknown environment light."""
    from oracle import oracle
    scene = A.film_scene("noon_blue_s16_d5")
    with pytest.raises(RuntimeError, match="unknown environment light atmosphere"):
        oracle.render(scene.describe(), A.FILM_SIZE, 16, 5)


def test_no_device_is_a_loud_failure():
    """No quiet fall-back: tables asked of a device that is not there are an error, and so is rendering."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    s = pa.Scene()
    with pytest.raises(pa.PineError, match="no HIP device"):
        s.set(pa.Atmosphere((0, 1, 0), (1, 1, 1), (8, 4), device=0))
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.PathIntegrator(A.film_sampler("noon_blue_s16_d5"), 5, device=0).render(A.film_scene("noon_blue_s16_d5"))
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        atmosphere_colors(np.zeros((1, 7), dtype=np.float32), 0)


def test_fixture_listing_is_complete():
    files = sorted(f for f in os.listdir(GOLDEN) if f.startswith("atmos"))
    want = sorted(["atmos.json", "atmos_color.npz"] + [f"atmos_{n}.npz" for n in A.CONFIGS] + [f"atmos_film_{n}.npz" for n in A.FILMS])
    assert files == want
    assert sorted(LISTING["configs"]) == sorted(A.CONFIGS) and sorted(LISTING["films"]) == sorted(A.FILMS)
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 100 * 1024, f
    for name in A.FILMS:
        fx = np.load(os.path.join(GOLDEN, f"atmos_film_{name}.npz"))
        if A.FILMS[name][0] != "default":  # (the default light's tables are built by the record tests; the text needs none)
            assert bytes(fx["pscene"]).decode() == A.film_scene(name).describe()
        assert fx["film"].shape == (A.FILM_SIZE[1], A.FILM_SIZE[0], 4)
        assert LISTING["films"][name]["centre_ray_misses"] >= 0.2 and LISTING["films"][name]["distinct_pixels"] >= 100


def prl_example():
    """examples/atmosphere.pine.  The script's decimal literals are read as the reference's parser reads them, digit by digit in
    binary32, which makes its 0.9 one ulp more than the 0.9 of the fixtures' scene; `9.0 / 10.0` is that one."""
    src = open(os.path.join(ROOT, "examples", "atmosphere.pine")).read()
    assert src.count("0.9") == 4
    return src, src.replace("0.9", "9.0 / 10.0")


def test_prl_dry_run_of_the_example():
    """examples/atmosphere.pine -- Atmosphere([x, y, z], [r, g, b]), the conversion to EnvironmentLight, scene.set -- yields the
    line with the script's sun direction and colour and the reference's 1024 x 1024."""
    prl = _Lazy("pine_amd.prl")
    src, exact = prl_example()
    ps, spp, depth = prl.scene_of_dry_run(prl.interpret(src, dry_run=True))
    env = [ln.split() for ln in ps.splitlines() if ln.startswith("envlight")]
    assert len(env) == 1 and env[0][:2] == ["envlight", "atmosphere"] and env[0][8:] == ["1024", "1024"]
    assert [float.fromhex(t) for t in env[0][2:8]] == [float(np.float32(v)) for v in (0.3, 1.0, 0.2, 4.0, 4.0, 4.0)]
    assert (spp, depth) == (16, 5)
    # ... and with its 0.9 spelt exactly it is the scene of the `default` film
    ps = prl.scene_of_dry_run(prl.interpret(exact, dry_run=True))[0]
    assert ps == bytes(np.load(os.path.join(GOLDEN, "atmos_film_default_blue_s16_d5.npz"))["pscene"]).decode()


def test_cpp_facade_example(tmp_path):
    """examples/atmosphere.cpp compiles against the facade (pine::Atmosphere, Scene::set) and sets the light the API sets."""
    lib_dir = os.path.join(ROOT, "pine_amd", "lib")
    exe = str(tmp_path / "atmosphere")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "examples", "atmosphere.cpp"), "-L" + lib_dir, "-lpine_gpu",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    # (the facade creates a material's constant nodes in its own order, so the node numbers differ: everything else is compared)
    def rest(text):
        return [ln for ln in text.splitlines() if not ln.startswith(("node ", "material "))]
    got, want = subprocess.check_output([exe, "--describe"], text=True), A.film_scene("noon_blue_s16_d5").describe()
    assert rest(got) == rest(want) and len(got.splitlines()) == len(want.splitlines())
    assert [ln for ln in got.splitlines() if ln.startswith("envlight")] == [ln for ln in want.splitlines() if ln.startswith("envlight")] != []
