"""ImageSky on the host: the density tree, the per-call functions (host build), the Radiance reader, the 8-bit conversion, the
refusals and the .pscene line, against fixtures made by the real reference (tools/make_golden_envsky.py).  Everything is
compared bit for bit; nothing here needs a GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import envsky_scenes as E


class _Lazy:
    """pine_amd (or one of its modules), imported at first use: a GPU run imports torch -- and with it the HIP runtime -- first."""
    def __init__(self, name):
        self._name = name

    def __getattr__(self, attr):
        if attr.startswith("_") or attr.startswith("pytest"):  # (what pytest's collection probes every module attribute for)
            raise AttributeError(attr)
        import importlib
        return getattr(importlib.import_module(self._name), attr)


pa, _lib, hdr = _Lazy("pine_amd"), _Lazy("pine_amd._lib"), _Lazy("pine_amd.hdr")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LISTING = json.load(open(os.path.join(GOLDEN, "envsky.json")))
_scenes = {}


def sky_scene(name):
    """A scene whose only content is the image's ImageSky (built once per image: `deep` takes a moment)."""
    if name not in _scenes:
        s = pa.Scene()
        s.set(E.image_sky(name))
        _scenes[name] = s
    return _scenes[name]


def env_records(scene, queries, device):
    q = np.ascontiguousarray(queries, dtype=np.float32)
    out = np.zeros((len(q), 13), dtype=np.float32)
    _lib.check(_lib.lib.pine_gpu_test_env_light(scene._h, device, q.ctypes.data_as(_lib.c_f_p), len(q), out.ctypes.data_as(_lib.c_f_p)),
               "pine_gpu_test_env_light")
    return out


def env_tree(scene):
    n = _lib.check(_lib.lib.pine_gpu_test_env_tree(scene._h, None, 0), "pine_gpu_test_env_tree")
    out = np.zeros(n, dtype=np.int32)
    _lib.check(_lib.lib.pine_gpu_test_env_tree(scene._h, out.ctypes.data_as(C.POINTER(C.c_int32)), n), "pine_gpu_test_env_tree")
    return out.reshape(-1, 7)


def first_difference(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return None if len(bad) == 0 else (tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))


@pytest.mark.parametrize("name", list(E.IMAGES))
def test_tree_equals_the_references(name):
    fx = np.load(os.path.join(GOLDEN, f"envsky_{name}.npz"))
    tree = env_tree(sky_scene(name))
    assert len(tree) == LISTING["images"][name]["nodes"]
    assert np.array_equal(tree[:len(fx["tree"])], fx["tree"])
    assert hashlib.md5(tree.tobytes()).hexdigest() == LISTING["images"][name]["tree_md5"]


@pytest.mark.parametrize("name", list(E.IMAGES))
def test_host_records_equal_the_references(name):
    fx = np.load(os.path.join(GOLDEN, f"envsky_{name}.npz"))
    assert fx["queries"].shape == (E.NUM_QUERIES, 5)
    got = env_records(sky_scene(name), fx["queries"], -1)
    assert first_difference(got, fx["records"]) is None


def test_queries_are_the_definitions():
    """The stored queries are envsky_scenes.base_queries but for the directions and the halved u2 the generator put in."""
    for name in E.IMAGES:
        q, base = np.load(os.path.join(GOLDEN, f"envsky_{name}.npz"))["queries"], E.base_queries(name)
        same = np.ones(len(q), dtype=bool)
        same[384:448] = False
        assert np.array_equal(q[same, 2:5].view(np.uint32), base[same, 2:5].view(np.uint32))
        changed = (q[:, 0:2].view(np.uint32) != base[:, 0:2].view(np.uint32)).any(axis=1)
        assert np.array_equal(q[changed, 0:2], base[changed, 0:2] * np.float32(0.5)) and changed.sum() <= 16


@pytest.mark.parametrize("kind", ["flat", "rle"])
def test_reader_returns_the_references_floats(kind):
    want = np.load(os.path.join(GOLDEN, "envsky_reader.npz"))[kind]
    got = hdr.read_hdr(os.path.join(GOLDEN, f"envsky_reader_{kind}.hdr"))
    assert got.dtype == np.float32 and got.shape == want.shape
    assert first_difference(got, want) is None
    assert (got == 0).all(axis=2).sum() >= 4  # the e = 0 texels


def test_reader_refuses_other_files(tmp_path):
    png = tmp_path / "picture.png"
    png.write_bytes(b"\x89PNG\r\n\x1a\n" + bytes(64))
    with pytest.raises(pa.PineError, match="picture.png"):
        pa.ImageSky(str(png))
    good = open(os.path.join(GOLDEN, "envsky_reader_flat.hdr"), "rb").read()
    for bad in (good.replace(b"32-bit_rle_rgbe", b"32-bit_rle_xyze"), good.replace(b"-Y 5 +X 9", b"+Y 5 +X 9"), good[:-7],
                open(os.path.join(GOLDEN, "envsky_reader_rle.hdr"), "rb").read()[:-3]):
        with pytest.raises(pa.PineError):
            hdr.read_hdr_bytes(bad, "bad.hdr")


def test_image_sky_from_a_file():
    path = os.path.join(GOLDEN, "envsky_reader_rle.hdr")
    a, b = pa.Scene(), pa.Scene()
    a.set(pa.ImageSky(path))
    b.set(pa.ImageSky(hdr.read_hdr(path)))
    assert a.describe() == b.describe() and "envlight image 9 5 " in a.describe()


def test_u8_texels_equal_the_references():
    """The 8-bit setter's texels are the reference's image[p]: color() at a texel's own direction returns tint * texel, and the
    describe() line carries the md5 of exactly those floats."""
    want = np.load(os.path.join(GOLDEN, "envsky_ldr.npz"))["texels"]
    line = [ln for ln in sky_scene("ldr").describe().splitlines() if ln.startswith("envlight image")][0]
    assert line.split()[-1] == hashlib.md5(np.ascontiguousarray(want).tobytes()).hexdigest()
    # ... and the float setter given those floats builds the same light
    s = pa.Scene()
    w, h, _, tint, elevation, rotation = E.IMAGES["ldr"]
    s.set(pa.ImageSky(want, tint, elevation, rotation))
    assert s.describe() == sky_scene("ldr").describe()
    q = np.load(os.path.join(GOLDEN, "envsky_ldr.npz"))["queries"]
    assert np.array_equal(env_records(s, q, -1).view(np.uint32), env_records(sky_scene("ldr"), q, -1).view(np.uint32))


def test_describe_line():
    w, h, _, tint, elevation, rotation = E.IMAGES["sun"]
    img = E.image("sun")
    s = pa.Scene()
    s.set(pa.ImageSky(img, (1.0, 0.5, 0.25), 0.125, -0.5))
    lines = s.describe().splitlines()
    env = [ln.split() for ln in lines if ln.startswith("envlight")]
    assert len(env) == 1 and env[0][:4] == ["envlight", "image", "16", "8"] and len(env[0]) == 10
    assert [float.fromhex(t) for t in env[0][4:9]] == [1.0, 0.5, 0.25, 0.125, -0.5]  # tint, elevation, rotation as hexfloat
    assert env[0][9] == hashlib.md5(img.tobytes()).hexdigest()
    assert not any("1e4" in ln or "0x1.388p+13" in ln for ln in lines)  # texels are not part of the text


def test_refusals():
    s = pa.Scene()
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    before = s.describe()
    img = E.image("sun")
    for bad, why in ((-1e-3, "negative"), (np.nan, "negative or not finite"), (np.inf, "not finite")):
        broken = img.copy()
        broken[3, 5, 1] = bad
        with pytest.raises(pa.PineError, match=why):
            s.set(pa.ImageSky(broken))
    for shape in ((0, 4, 3), (4, 0, 3)):
        with pytest.raises(pa.PineError, match="1 x 1"):
            s.set(pa.ImageSky(np.zeros(shape, dtype=np.float32)))
        with pytest.raises(pa.PineError, match="1 x 1"):
            s.set(pa.ImageSky(np.zeros(shape, dtype=np.uint8)))
    with pytest.raises(pa.PineError):
        pa.ImageSky(np.zeros((4, 4), dtype=np.float32))
    f3 = _lib.f3(1, 1, 1)
    one = np.zeros(3, dtype=np.float32)
    assert _lib.lib.pine_gpu_scene_set_env_image(s._h, one.ctypes.data_as(_lib.c_f_p), 1 << 14, (1 << 12) + 1, f3, 0.0, 0.0) < 0
    assert "2^26" in _lib.last_error()
    assert s.describe() == before  # a refused image leaves the scene as it was


def test_replacing_sky_by_image_sky_and_back():
    s = pa.Scene()
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    sky_text = s.describe()
    assert sky_text.count("envlight") == 1 and "envlight sky" in sky_text
    s.set(E.image_sky("ragged"))
    text = s.describe()
    assert text.count("envlight") == 1 and "envlight image 13 7" in text
    assert len(env_tree(s)) == LISTING["images"]["ragged"]["nodes"]
    s.set(pa.Sky([1.0, 2.0, 3.0]))
    assert s.describe() == sky_text
    with pytest.raises(pa.PineError, match="no ImageSky"):
        env_tree(s)


def test_oracle_refuses_the_line():
    """The CPU restatement does not cover ImageSky: it refuses the scene as it refuses any unknown environment light."""
    from oracle import oracle
    scene = E.film_scene("const_24_s8_d3")
    with pytest.raises(Exception):
        oracle.render(scene.describe(), (24, 24), 8, 3)


def test_no_device_is_a_loud_failure():
    """No CPU path behind ImageSky either: without a device, rendering and the device leg of the hook raise."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    scene = E.film_scene("black_24_s4_d3")
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        pa.PathIntegrator(E.film_sampler("black_24_s4_d3"), 3, device=0).render(scene)
    with pytest.raises(pa.PineError, match="no HIP device|hip"):
        env_records(sky_scene("const"), np.zeros((1, 5), dtype=np.float32), 0)


def test_fixture_listing_is_complete():
    files = sorted(f for f in os.listdir(GOLDEN) if f.startswith("envsky"))
    want = sorted(["envsky.json", "envsky_reader.npz", "envsky_reader_flat.hdr", "envsky_reader_rle.hdr"] +
                  [f"envsky_{n}.npz" for n in E.IMAGES] + [f"envsky_film_{n}.npz" for n in E.FILMS])
    assert files == want
    assert sorted(LISTING["images"]) == sorted(E.IMAGES) and sorted(LISTING["films"]) == sorted(E.FILMS)
    for f in files:
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 100 * 1024, f
    for name in E.FILMS:
        fx = np.load(os.path.join(GOLDEN, f"envsky_film_{name}.npz"))
        assert bytes(fx["pscene"]).decode() == E.film_scene(name).describe()
        w, h = E.FILMS[name][1]
        assert fx["film"].shape == (h, w, 4)


ROOT = os.path.dirname(os.path.dirname(GOLDEN))


def test_prl_dry_run_of_the_example():
    """examples/image_sky.pine -- ImagePtr([r, g, b]), ImageSky(ImagePtr), the conversion to EnvironmentLight, scene.set -- builds
    the scene of the const film; the four-argument ImageSky and a file that is no Radiance image are refused by name."""
    prl = _Lazy("pine_amd.prl")
    src = open(os.path.join(ROOT, "examples", "image_sky.pine")).read()
    ps, spp, depth = prl.scene_of_dry_run(prl.interpret(src, dry_run=True))
    assert (ps, spp, depth) == (E.film_scene("const_24_s8_d3").describe(), 8, 3)
    turned = src.replace("ImageSky(ImagePtr([0.75, 1.0, 1.5]))", "ImageSky(ImagePtr([0.75, 1.0, 1.5]), [1, 0.5, 0.25], 0.125, -0.5)")
    env = [ln.split() for ln in prl.scene_of_dry_run(prl.interpret(turned, dry_run=True))[0].splitlines() if ln.startswith("envlight")]
    assert len(env) == 1 and [float.fromhex(t) for t in env[0][4:9]] == [1.0, 0.5, 0.25, 0.125, -0.5]
    hdr_path = os.path.join(GOLDEN, "envsky_reader_flat.hdr")
    for ctor in ("ImagePtr", "load_image"):
        from_file = src.replace("ImagePtr([0.75, 1.0, 1.5])", f'{ctor}("{hdr_path}")')
        assert "envlight image 9 5 " in prl.scene_of_dry_run(prl.interpret(from_file, dry_run=True))[0]
    with pytest.raises(prl.PrlError, match="envsky.json"):
        prl.interpret(src.replace("ImagePtr([0.75, 1.0, 1.5])", 'ImagePtr("%s")' % os.path.join(GOLDEN, "envsky.json")), dry_run=True)


def test_cpp_facade_example_and_reader(tmp_path):
    """examples/image_sky.cpp compiles against the facade (pine::Image, pine::ImageSky, Scene::set), builds the scene the API
    builds, and the C++ reader returns the reference's floats for both .hdr files; an LDR file is refused by name."""
    import subprocess
    lib_dir = os.path.join(ROOT, "pine_amd", "lib")
    exe = str(tmp_path / "image_sky")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "examples", "image_sky.cpp"), "-L" + lib_dir, "-lpine_gpu",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    assert subprocess.check_output([exe, "--describe"], text=True) == E.film_scene("const_24_s8_d3").describe()
    golden = np.load(os.path.join(GOLDEN, "envsky_reader.npz"))
    for kind in ("flat", "rle"):
        lines = subprocess.check_output([exe, os.path.join(GOLDEN, f"envsky_reader_{kind}.hdr"), "--describe"], text=True).splitlines()
        at = max(i for i, ln in enumerate(lines) if ln.startswith("camera "))
        got = np.array([float.fromhex(t) for t in lines[at + 1:]], dtype=np.float32).reshape(5, 9, 3)
        assert first_difference(got, golden[kind]) is None
        env = [ln.split() for ln in lines if ln.startswith("envlight")][0]
        assert env[9] == hashlib.md5(golden[kind].tobytes()).hexdigest() and float.fromhex(env[8]) == 0.25
    png = tmp_path / "picture.png"
    png.write_bytes(b"\x89PNG\r\n\x1a\n" + bytes(64))
    r = subprocess.run([exe, str(png), "--describe"], capture_output=True, text=True)
    assert r.returncode == 1 and "picture.png" in r.stderr
