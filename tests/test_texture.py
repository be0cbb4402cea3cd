"""Image texture nodes (Texture / Texturef = NodeImage / NodeImagef) on the host build: material_params against records made by
the real reference (tools/make_golden_texture.py), bit for bit; the host's fold of constant coordinates; storage; the ABI's
refusals; the .pscene lines; the Python front."""
import ctypes as C
import os

import numpy as np
import pytest

import texture_scenes as X
from test_envsky import _lib, pa  # (imported at first use: a GPU run imports torch first)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
# the slots of pine_gpu_test_material_params' record a material kind has; the reference's record holds 0 in the others
SLOTS = {"diffuse": (1, 1, 1, 1, 1, 1, 0, 0, 0, 0), "metal": (1, 1, 1, 1, 1, 1, 1, 0, 0, 0), "glossy": (1, 1, 1, 1, 1, 1, 1, 0, 0, 1),
         "glass": (1, 1, 1, 1, 1, 1, 1, 0, 0, 1), "uber": (1, 1, 1, 1, 1, 1, 1, 1, 1, 1)}
FIELDS = ("albedo.x", "albedo.y", "albedo.z", "albedo/Pi.x", "albedo/Pi.y", "albedo/Pi.z", "roughness", "metallic", "transmission", "ior")


@pytest.fixture(scope="module")
def zoo_fixture():
    z = np.load(os.path.join(GOLDEN, "texture_zoo.npz"))
    return np.ascontiguousarray(z["queries"]), np.ascontiguousarray(z["records"]), bytes(z["pscene"]).decode()


@pytest.fixture(scope="module")
def zoo(zoo_fixture):
    sc, mats = X.texture_zoo(zoo_fixture[0])
    return sc, mats


def material_params(scene, device, queries, nm):
    out = np.full((nm, len(queries), 10), -7.0, F32)
    _lib.check(_lib.lib.pine_gpu_test_material_params(scene._h, device, queries.ctypes.data_as(_lib.c_f_p), len(queries),
                                                      out.ctypes.data_as(_lib.c_f_p)), "pine_gpu_test_material_params")
    return out


def assert_records(who, got, want, mats, queries):
    mask = np.array([SLOTS[k] for _, k in mats], bool)[:, None, :]
    bad = (got.view(np.uint32) != want.view(np.uint32)) & mask
    if not bad.any():
        return
    m, q, s = (int(v) for v in np.argwhere(bad)[0])
    raise AssertionError(f"{who}: {int(bad.any(axis=2).sum())} of {bad.shape[0] * bad.shape[1]} records differ; first: material {m} ({mats[m][0]}), "
                         f"query {q} p {[float(v).hex() for v in queries[q, 0:3]]} uv {[float(v).hex() for v in queries[q, 6:8]]}, {FIELDS[s]}: "
                         f"got {float(got[m, q, s]).hex()}, want {float(want[m, q, s]).hex()}")


def check_records(device, zoo, zoo_fixture):
    sc, mats = zoo
    queries, want, _ = zoo_fixture
    assert want.shape == (len(mats), X.NUM_QUERIES, 10)
    assert_records("host build" if device < 0 else "device", material_params(sc, device, queries, len(mats)), want, mats, queries)


def tex_words(scene):
    return _lib.check(_lib.lib.pine_gpu_test_tex_words(scene._h), "pine_gpu_test_tex_words")


# ---- the node against the reference ------------------------------------------------------------------------------------------
def test_host_records_equal_the_references(zoo, zoo_fixture):
    check_records(-1, zoo, zoo_fixture)


def test_the_fixture_is_the_scene_the_test_builds(zoo, zoo_fixture):
    assert zoo[0].describe() == zoo_fixture[2]
    assert np.array_equal(X.queries().view(np.uint32), zoo_fixture[0].view(np.uint32))


def test_constant_twins_fold_and_equal_their_originals(zoo, zoo_fixture):
    """A twin's coordinate is a literal equal to one query: the host folds the lookup into the material record (no program), and
    the reference's record of the twin -- at any query -- is its record of the original at that query."""
    sc, mats = zoo
    queries, want, _ = zoo_fixture
    n = X.num_programs()
    from test_node_fixtures import node_programs
    prog, ops = node_programs(sc)
    assert (prog[:n] >= 0).any(axis=1).all() and (prog[n:] == -1).all(), "a constant lookup was not folded (or a surface-reading one was)"
    got = material_params(sc, -1, queries[:1], len(mats))
    for t, qi in enumerate(X.TWIN_QUERIES):
        twins = slice(n * (t + 1), n * (t + 2))
        assert_records(f"twins at query {qi}", got[twins], want[:n, qi:qi + 1], mats[twins], queries[qi:qi + 1])
        assert np.array_equal(want[twins, 0].view(np.uint32), want[twins, 300].view(np.uint32))


def test_eight_bit_texels_read_as_the_same_floats_uploaded(zoo_fixture):
    """The table path against the float path: the same image uploaded as pre-linearised floats."""
    queries = zoo_fixture[0]
    got = []
    for as_float in (False, True):
        sc = pa.Scene()
        for name in ("ramp8_16x16", "rgba8_7x4"):
            a = X.image(name)
            if as_float:
                a = _linear(a)
            im = pa.Image(a)
            sc.add(f"uv {name}", pa.Diffuse(pa.Texture(pa.UV(), im)))
            sc.add(f"pos {name}", pa.Metal(pa.Texture(pa.Position() * 1.7, im), pa.Texturef(pa.UV(), im)))
        got.append(material_params(sc, -1, queries, 4))
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))


def _linear(u8):
    """Image::operator[] of an 8-bit image (image.cpp:10-13) through the library's own table: a 256 x 1 ramp read texel by texel."""
    ramp = np.zeros((1, 256, 3), np.uint8)
    ramp[0, :, 0] = np.arange(256)
    sc = pa.Scene()
    sc.add("ramp", pa.Diffuse(pa.Texture(pa.UV(), pa.Image(ramp))))
    q = np.zeros((256, 8), F32)
    q[:, 6] = (np.arange(256, dtype=F32) + F32(0.5)) / F32(256)
    table = material_params(sc, -1, q, 1)[0, :, 0]
    assert table[0] == 0 and table[255] == 1 and (np.diff(table) > 0).all()
    return np.ascontiguousarray(table[u8[..., :3]], dtype=F32)


def test_an_image_under_several_nodes_is_stored_once(zoo):
    sizes = {name: w * h * (3 if kind == "f32" else 1) for name, (w, h, kind) in X.IMAGES.items()}
    assert tex_words(zoo[0]) == 256 + sum(sizes.values())  # 112 image nodes, 6 images
    sc = pa.Scene()
    im = pa.Image(X.image("f32_3x5"))
    sc.add("a", pa.Diffuse(pa.Texture(pa.UV(), im)))
    assert tex_words(sc) == 256 + 45
    sc.add("b", pa.Metal(pa.Texture(pa.Position(), im), pa.Texturef(pa.UV() * 2.0, im)))
    assert tex_words(sc) == 256 + 45 and sc.describe().count("\nimage ") == 1
    sc.add("c", pa.Diffuse(pa.Texture(pa.UV(), pa.Image(X.image("f32_3x5")))))  # another Image object: another image
    assert tex_words(sc) == 256 + 90
    plain = pa.Scene()
    plain.add("a", pa.Diffuse(pa.lerp(pa.Checkerboard(pa.UV()), [0.5, 0.5, 0.5], [0.1, 0.1, 0.1])))
    plain.add("b", pa.Diffuse(pa.Texture([0.2, 0.7, 0.0], im)))  # folded: nothing for the device to read
    assert tex_words(plain) == 0


def test_non_finite_coordinates_read_texel_zero():
    """The reference converts a NaN to an int there (undefined; it reads outside its array): the library reads texel 0 on that
    axis.  Host build only."""
    img = X.image("f32_3x5")
    sc = pa.Scene()
    sc.add("uv", pa.Diffuse(pa.Texture(pa.UV(), pa.Image(img))))
    q = np.zeros((6, 8), F32)
    q[:, 6:8] = [[np.nan, 0.5], [np.inf, 0.5], [-np.inf, 0.5], [0.5, np.nan], [0.5, np.inf], [np.nan, -np.inf]]
    got = material_params(sc, -1, q, 1)[0, :, 0:3]
    want = [img[2, 0], img[2, 0], img[2, 0], img[0, 1], img[0, 1], img[0, 0]]
    assert np.array_equal(got.view(np.uint32), np.array(want, F32).view(np.uint32))


# ---- the ABI's refusals ------------------------------------------------------------------------------------------------------
def _refused(rc, message):
    assert rc < 0
    assert message in _lib.last_error(), _lib.last_error()


def test_refusals():
    lib, sc = _lib.lib, pa.Scene()
    h = sc._h
    f = np.ones((2, 2, 3), F32)
    fp = f.ctypes.data_as(_lib.c_f_p)
    u = np.ones((2, 2, 4), np.uint8)
    up = u.ctypes.data_as(C.POINTER(C.c_uint8))
    _refused(lib.pine_gpu_scene_add_image(h, fp, 0, 2), "at least 1 x 1 texels")
    _refused(lib.pine_gpu_scene_add_image(h, fp, 2, -1), "at least 1 x 1 texels")
    _refused(lib.pine_gpu_scene_add_image_u8(h, up, 3, 2, 0), "at least 1 x 1 texels")
    _refused(lib.pine_gpu_scene_add_image(h, fp, 8193, 8192), "more than 2^26 texels")  # (refused before a texel is read)
    _refused(lib.pine_gpu_scene_add_image_u8(h, up, 4, 1 << 14, (1 << 12) + 1), "more than 2^26 texels")
    for bad in (np.nan, np.inf, -np.inf):
        g = f.copy()
        g[1, 0, 2] = bad
        _refused(lib.pine_gpu_scene_add_image(h, g.ctypes.data_as(_lib.c_f_p), 2, 2), "not finite")
    for ch in (0, 1, 2, 5):
        _refused(lib.pine_gpu_scene_add_image_u8(h, up, ch, 2, 2), "3 or 4 channels")
    _refused(lib.pine_gpu_scene_add_image(h, None, 2, 2), "null")
    assert sc.describe().count("\nimage ") == 0
    image = _lib.check(lib.pine_gpu_scene_add_image(h, fp, 2, 2), "image")
    p3 = _lib.check(lib.pine_gpu_scene_node_input(h, 2), "uv")
    pf = _lib.check(lib.pine_gpu_scene_node_constf(h, 0.5), "constf")
    for fn in (lib.pine_gpu_scene_node_image, lib.pine_gpu_scene_node_imagef):
        _refused(fn(h, p3, image + 1), "image id out of range")
        _refused(fn(h, p3, -1), "image id out of range")
        _refused(fn(h, pf, image), "a Node3f operand is required")
        _refused(fn(h, 99, image), "operand id out of range")
    assert lib.pine_gpu_scene_node_is_vec3(h, _lib.check(lib.pine_gpu_scene_node_image(h, p3, image), "node")) == 1
    assert lib.pine_gpu_scene_node_is_vec3(h, _lib.check(lib.pine_gpu_scene_node_imagef(h, p3, image), "node")) == 0


# ---- .pscene -----------------------------------------------------------------------------------------------------------------
def test_pscene_lines():
    import hashlib
    f, u3, u4 = X.image("f32_3x5"), X.image("ramp8_16x16"), X.image("rgba8_7x4")
    sc = pa.Scene()
    a, b, c = pa.Image(f), pa.Image(u3), pa.Image(u4)
    sc.add("m", pa.Uber(pa.Texture(pa.UV(), a), pa.Texturef(pa.Position(), b), pa.Texture(pa.UV(), c)[2], 0.0))
    lines = sc.describe().splitlines()
    md5 = lambda x: hashlib.md5(x.tobytes()).hexdigest()  # noqa: E731
    assert lines[1:4] == [f"image 0 3 5 f32 {md5(f)}", f"image 1 16 16 u8x3 {md5(u3)}", f"image 2 7 4 u8x4 {md5(u4)}"]
    assert lines[4:12] == ["node 0 uv", "node 1 image 0 0", "node 2 position", "node 3 imagef 2 1", "node 4 uv", "node 5 image 4 2", "node 6 comp 5 2",
                           "node 7 constf 0x0p+0"]


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_python_image_sources_and_overloads(tmp_path):
    f = X.image("f32_3x5")
    assert pa.Image(f).texels.dtype == np.float32 and pa.Image(f.astype(np.float64)).texels.dtype == np.float32
    assert pa.Image(X.image("rgba8_7x4")).texels.shape == (4, 7, 4)
    for bad in (np.zeros((4, 4), F32), np.zeros((4, 4, 4), F32), np.zeros((4, 4, 2), np.uint8)):
        with pytest.raises(pa.PineError, match="expected"):
            pa.Image(bad)
    # a Radiance file: the texels ImageSky's reader returns
    hdr = os.path.join(GOLDEN, "envsky_reader_flat.hdr")
    want = np.load(os.path.join(GOLDEN, "envsky_reader.npz"))["flat"]
    assert np.array_equal(pa.Image(hdr).texels.view(np.uint32), want.view(np.uint32))
    # a PNG: 3 channels, as the reference's image_from asks stb for
    png = np.load(os.path.join(GOLDEN, "texture_png.npz"))
    for name in ("palette_trns", "grey_alpha", "rgba"):
        assert np.array_equal(pa.Image(os.path.join(GOLDEN, f"texture_png_{name}.png")).texels, png[name + "_3"])
    with pytest.raises(pa.PineError, match="16-bit"):
        pa.Image(os.path.join(GOLDEN, "texture_png_refused_16bit.png"))
    junk = tmp_path / "x.bin"
    junk.write_bytes(b"GIF89a" + bytes(32))
    with pytest.raises(pa.PineError, match="neither a PNG nor a Radiance"):
        pa.Image(str(junk))
    jpeg = tmp_path / "x.jpg"
    jpeg.write_bytes(b"\xff\xd8\xff\xe0" + bytes(32))
    with pytest.raises(pa.PineError, match="JPEG"):
        pa.Image(str(jpeg))
    # Texture: Node3f, Texturef: Nodef; a plain array or a path where an image is expected; a constant coordinate
    t, tf = pa.Texture(pa.UV(), f), pa.Texturef([0.1, 0.2, 0.0], hdr)
    assert t.is_vec3 and not tf.is_vec3
    assert pa.Texture(tf, f).args[0].kind == "splat"  # a Nodef where the Node3f is expected: Node3f(Nodef), node.h:78
    sc = pa.Scene()
    sc.add("m", pa.Metal(t, tf))
    assert "node 1 image 0 0" in sc.describe() and "imagef" in sc.describe()


# ---- PRL and the C++ facade --------------------------------------------------------------------------------------------------
def _prl():
    from pine_amd import prl
    return prl


def _script():
    root = os.path.dirname(os.path.dirname(GOLDEN))
    return open(os.path.join(root, "examples", "textured.pine")).read().replace("tests/golden/", GOLDEN + "/")


def test_prl_example_builds_the_python_scene():
    """examples/textured.pine -- ImagePtr("x.png"), load_image, Texture in Node3f and Nodef slots -- builds the scene
    texture_scenes.script_room builds, line for line."""
    prl = _prl()
    ps, spp, depth = prl.scene_of_dry_run(prl.interpret(_script(), dry_run=True))
    assert (ps, spp, depth) == (X.script_room().describe(), 8, 4)
    assert ps.count("\nimage ") == 3  # two PNG files and the 1 x 1 image, each once, under five Texture nodes


def test_prl_texture_type_resolution():
    """What the reference's double registration of `Texture` (node.cpp:66-67) resolves to, as read from context.cpp: one value that
    converts to Node3f (the rgb) and to Nodef (the first component); ambiguous where both fit equally well."""
    prl = _prl()
    png = os.path.join(GOLDEN, "texture_ramp8_16x16.png")
    head = f'img := ImagePtr("{png}"); s := Scene(); '
    tail = ' s.set(ThinLenCamera(Film([8, 8], Uncharted2()), [0, 1, -4], [0, 1, 0], 0.4)); PathIntegrator(BlueSampler(1), 1).render(s);'
    nodes = lambda body: [ln.split()[2] for ln in prl.scene_of_dry_run(prl.interpret(head + body + tail, dry_run=True))[0].splitlines()  # noqa: E731
                          if ln.startswith("node ")]
    assert nodes('s.add(Sphere([0, 1, 0], 1.0), Diffuse(Texture(UV(), img)));') == ["uv", "image"]
    assert nodes('s.add(Sphere([0, 1, 0], 1.0), Metal(Texture(UV(), img), Texture(Position(), img)));') == ["uv", "image", "position", "imagef"]
    assert nodes('t := Texture(UV(), img); s.add(Sphere([0, 1, 0], 1.0), Uber(t, t, t[2], 0.0, 1.5));') == ["uv", "image", "imagef", "comp", "constf"]
    assert nodes('s.add(Sphere([0, 1, 0], 1.0), Diffuse(Node3f(Texture(UV(), img)) * 0.5));')[:2] == ["uv", "image"]
    assert nodes('s.add(Sphere([0, 1, 0], 1.0), Metal([1, 1, 1], Nodef(Texture(UV(), img)) * 0.5));')[1:3] == ["uv", "imagef"]
    with pytest.raises(prl.PrlError, match=r"Ambiguous function call `\*\(Texture, f32\)`"):
        nodes('s.add(Sphere([0, 1, 0], 1.0), Diffuse(Texture(UV(), img) * 0.5));')
    with pytest.raises(prl.PrlError, match="Texture"):
        nodes('s.add(Sphere([0, 1, 0], 1.0), Diffuse(Texture(0.5, img)));')  # the coordinate is a Node3f
    for ctor in ("ImagePtr", "load_image"):
        rgba = os.path.join(GOLDEN, "texture_png_rgba.png")
        ps = prl.scene_of_dry_run(prl.interpret(f'img := {ctor}("{rgba}"); s := Scene(); s.add(Sphere([0, 1, 0], 1.0), Diffuse(Texture(UV(), img)));' + tail,
                                                dry_run=True))[0]
        assert "image 0 9 7 u8x3 " in ps
    with pytest.raises(prl.PrlError, match="16-bit"):
        prl.interpret(f'img := ImagePtr("{os.path.join(GOLDEN, "texture_png_refused_16bit.png")}");', dry_run=True)


def test_cpp_facade_example_and_png_image(tmp_path):
    """examples/textured.cpp compiles against the facade, imports the textured .glb as pine_amd/gltf.py does, and pine::Image reads
    a .png file to the bytes the reference's image_from returns."""
    import subprocess
    from pine_amd import gltf
    root = os.path.dirname(os.path.dirname(GOLDEN))
    lib_dir = os.path.join(root, "pine_amd", "lib")
    exe = str(tmp_path / "textured")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(root, "examples", "textured.cpp"), "-L" + lib_dir, "-lpine_gpu",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    glb = os.path.join(GOLDEN, "textured_quad.glb")
    assert subprocess.check_output([exe, glb, "--describe"], text=True) == gltf.load(glb).describe()
    golden = np.load(os.path.join(GOLDEN, "texture_png.npz"))
    for name in ("grey", "rgb", "palette", "palette_trns", "grey_alpha", "rgba"):
        out = subprocess.check_output([exe, glb, os.path.join(GOLDEN, f"texture_png_{name}.png"), "--texels"], text=True).split()
        assert out[:2] == ["9", "7"] and bytes.fromhex(out[2]) == golden[name + "_3"].tobytes(), name
    sky = subprocess.check_output([exe, glb, os.path.join(GOLDEN, "texture_png_rgb.png"), "--describe"], text=True)
    assert "envlight image 9 7 " in sky
    r = subprocess.run([exe, glb, os.path.join(GOLDEN, "texture_png_refused_interlaced.png"), "--texels"], capture_output=True, text=True)
    assert r.returncode == 1 and "interlaced" in r.stderr
