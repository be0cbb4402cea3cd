"""The images, queries and scenes of the image-texture fixtures (tests/golden/texture_*.npz, listed in texture.json): shared by
tools/make_golden_texture.py, which runs them through the real reference, and tests/test_texture.py / test_texture_gpu.py.
Images come from seeded integer arithmetic, so their texels are not committed."""
import numpy as np

F32 = np.float32
# name: (w, h, kind)
IMAGES = {
    "ramp8_16x16": (16, 16, "u8x3"),   # r runs through all 256 byte values: the whole table
    "rgba8_7x4": (7, 4, "u8x4"),       # alpha varies and must not matter
    "f32_3x5": (3, 5, "f32"),          # values above 1, zeros, a denormal
    "one_1x1": (1, 1, "f32"),          # ImagePtr(vec3)
    "wide_4099x1": (4099, 1, "f32"),   # the clamp (fract == 1.0: the product is the size) at a size that is no power of two
    "tall_1x257": (1, 257, "f32"),     # the same on the other axis
}
NUM_QUERIES = 512
TWIN_QUERIES = (9, 70, 400)  # -1e-9 (the clamp), a k / size boundary, an ordinary value


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


def image(name):
    """(h, w, 3 | 4) float32 or uint8, rows as the reference keeps them."""
    w, h, kind = IMAGES[name]
    if name == "ramp8_16x16":
        img = (_hash(w * h * 3, 21) >> np.uint32(24)).astype(np.uint8).reshape(h, w, 3)
        img[..., 0] = np.arange(256, dtype=np.uint8).reshape(h, w)
        return img
    if name == "rgba8_7x4":
        return (_hash(w * h * 4, 22) >> np.uint32(24)).astype(np.uint8).reshape(h, w, 4)
    if name == "f32_3x5":
        img = (_unit(w * h * 3, 23) * F32(3)).reshape(h, w, 3)
        img[0, 0] = 0.0
        img[2, 1, 1] = 0.0
        img[4, 2, 2] = F32(1e-41)  # a denormal
        img[1, 2] = [7.5, 12.0, 100.0]
        return img.astype(F32)
    if name == "one_1x1":
        return np.array([[[0.25, 0.5, 0.75]]], dtype=F32)
    if name in ("wide_4099x1", "tall_1x257"):
        return _unit(w * h * 3, 24 + h).reshape(h, w, 3).astype(F32)
    raise KeyError(name)


def images(pa):
    """One pa.Image per name: an Image object is one image of a scene however many nodes read it."""
    return {name: pa.Image(image(name)) for name in IMAGES}


# ---- the per-call zoo --------------------------------------------------------------------------------------------------------
def programs(pa, im, P, U):
    """(name, material kind, material) over Position-like P and UV-like U (nodes, or constants for the twins)."""
    T, Tf = pa.Texture, pa.Texturef
    P, U = pa.Node.of(P), pa.Node.of(U)
    out = []
    for name in IMAGES:
        out.append((f"uv {name}", "diffuse", pa.Diffuse(T(U, im[name]))))
        out.append((f"position {name}", "diffuse", pa.Diffuse(T(P, im[name]))))
    affine = U * -2.5 + [0.3, -1.7, 0.0]  # (negative results)
    out += [
        ("affine ramp8", "diffuse", pa.Diffuse(T(affine, im["ramp8_16x16"]))),
        ("affine wide", "diffuse", pa.Diffuse(T(P * 0.37 - [5.0, 0.25, 0.0], im["wide_4099x1"]))),
        ("uber comps", "uber", pa.Uber(T(U, im["rgba8_7x4"]), T(P, im["rgba8_7x4"])[1], T(U, im["ramp8_16x16"])[2], T(affine, im["f32_3x5"])[0], 1.45)),
        ("metal texf", "metal", pa.Metal(T(P, im["f32_3x5"]), Tf(U, im["ramp8_16x16"]))),
        ("glossy lerp", "glossy", pa.Glossy(pa.lerp(Tf(U, im["rgba8_7x4"]), T(U, im["ramp8_16x16"]), T(P, im["f32_3x5"])), Tf(P, im["tall_1x257"]), Tf(U, im["one_1x1"]) + 1.0)),
        ("glass", "glass", pa.Glass(T(U, im["wide_4099x1"]), Tf(U * 3.0, im["rgba8_7x4"]), Tf(P, im["f32_3x5"]) + 1.0)),
    ]
    return out


def texture_zoo(queries, twins=True):
    """-> (scene, [(name, kind)]): every program over Position() / UV(), then its constant twins at TWIN_QUERIES."""
    import pine_amd as pa
    im = images(pa)
    sc, mats = pa.Scene(), []
    for name, kind, m in programs(pa, im, pa.Position(), pa.UV()):
        sc.add(f"m{len(mats)}", m)
        mats.append((name, kind))
    for qi in TWIN_QUERIES if twins else ():
        q = [float(v) for v in queries[qi]]
        for name, kind, m in programs(pa, im, q[0:3], [q[6], q[7], 0.0]):
            sc.add(f"m{len(mats)}", m)
            mats.append((f"twin at {qi} of {name}", kind))
    return sc, mats


def num_programs():
    return 2 * len(IMAGES) + 6


def queries():
    """(NUM_QUERIES, 8): p, n, uv.  uv and p.xy carry the coordinates under test (differently dealt, so that UV() and Position()
    programs read different texels); p.z and n are ordinary."""
    n = NUM_QUERIES
    r = _unit(n * 8, 31).reshape(n, 8)
    q = (r * F32(6) - F32(3)).astype(F32)
    nn = q[:, 3:6] / np.maximum(np.linalg.norm(q[:, 3:6], axis=1, keepdims=True), F32(1e-6))
    q[:, 3:6] = nn.astype(F32)
    special = [F32(0), F32(1), F32(-0.0), F32(-1e-9), F32(1e7), F32(-1e7), F32(-1e-10), F32(-2.0 ** -30), F32(-1e-20), F32(-3e-9),
               F32(-1e-38), F32(-7e-12)]
    i = 0
    for a in special:  # each special value on x, on y, and on both
        for mode in range(3):
            for cols in ((6, 7), (0, 1)):
                if mode != 1:
                    q[i, cols[0]] = a
                if mode != 0:
                    q[i, cols[1]] = a
            i += 1
    assert i == 36

    def boundaries(size, ks):
        out = []
        for k in ks:
            b = F32(k) / F32(size)
            out += [b, np.nextafter(b, F32(-1)), np.nextafter(b, F32(2))]
        return out

    some = lambda size: sorted({0, 1, 2, size // 3, size // 2, size - 2, size - 1, size} | {int(v) % (size + 1) for v in _hash(12, size)})  # noqa: E731
    xs = boundaries(16, range(17)) + boundaries(7, range(8)) + boundaries(3, range(4)) + boundaries(4099, some(4099))
    ys = boundaries(16, range(17)) + boundaries(4, range(5)) + boundaries(5, range(6)) + boundaries(257, some(257))
    for k, b in enumerate(xs):  # x on a boundary (uv of one query, p of the next-but-one), y ordinary
        q[i, 6] = b
        q[i, 0] = xs[(k + 2) % len(xs)]
        i += 1
    for k, b in enumerate(ys):
        q[i, 7] = b
        q[i, 1] = ys[(k + 2) % len(ys)]
        i += 1
    assert i <= n - 100, i  # the rest stay ordinary values in [-3, 3)
    return np.ascontiguousarray(q, dtype=F32)


# ---- films -------------------------------------------------------------------------------------------------------------------
# name: (size, spp, depth)
FILMS = {"tex_room_48x32_s8_d4": ((48, 32), 8, 4), "tex_script_room_48x32_s8_d4": ((48, 32), 8, 4)}
GUIDES_SIZE = (32, 24)
TEXTURED = ("floor", "back", "ball", "quad")  # the room's materials that read an image


def room(size=None, flat=False, as_float=False):
    """A closed room with an area light.  flat: every texture replaced by its mean colour; as_float: the 8-bit images uploaded
    as the floats they read as (tools/texture_speed.py)."""
    import pine_amd as pa
    im = {}
    for name in ("ramp8_16x16", "rgba8_7x4", "f32_3x5"):
        a = image(name)
        if as_float and a.dtype == np.uint8:
            a = np.power(a[..., :3].astype(F32) / F32(255), F32(2.2)).astype(F32)
        im[name] = pa.Image(a)
    T = pa.Texture
    if flat:
        mean = {k: [float(v) for v in np.power(image(k)[..., :3].astype(F32) / F32(255), F32(2.2)).mean(axis=(0, 1))] if image(k).dtype == np.uint8
                else [float(v) for v in image(k).mean(axis=(0, 1))] for k in im}
        T = lambda p, i: pa.Node.of(mean[[k for k in im if im[k] is i][0]])  # noqa: E731
    s = pa.Scene()
    s.add("floor", pa.Diffuse(T(pa.UV() * 3.0, im["ramp8_16x16"])))
    back = T(pa.UV(), im["rgba8_7x4"])
    s.add("back", pa.Uber([0.8, 0.7, 0.6], back[1], back[2], 0.0, 1.45))
    s.add("ball", pa.Diffuse(T(pa.Position(), im["f32_3x5"]) * 0.25))
    s.add("quad", pa.Diffuse(T(pa.UV(), im["ramp8_16x16"])))
    s.add("white", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add("lamp", pa.Emissive([12.0, 11.0, 9.0]))
    s.add(pa.Rect([0, 0, 0], [4, 0, 0], [0, 0, 4], True), "floor")
    s.add(pa.Rect([0, 3, 0], [4, 0, 0], [0, 0, 4], False), "white")
    s.add(pa.Rect([0, 1.5, 2], [4, 0, 0], [0, 3, 0], True), "back")
    s.add(pa.Rect([0, 1.5, -2], [4, 0, 0], [0, 3, 0], False), "white")
    s.add(pa.Rect([-2, 1.5, 0], [0, 0, 4], [0, 3, 0], False), "white")
    s.add(pa.Rect([2, 1.5, 0], [0, 0, 4], [0, 3, 0], True), "white")
    s.add(pa.Rect([0, 2.99, 0], [1.2, 0, 0], [0, 0, 1.2], False), "lamp")
    s.add(pa.Sphere([-0.8, 0.6, 0.4], 0.6), "ball")
    verts = np.array([[0.3, 0.2, 0.9], [1.6, 0.2, 0.3], [1.6, 1.5, 0.3], [0.3, 1.5, 0.9]], F32)
    uvs = np.array([[-0.5, -0.25], [1.75, -0.25], [1.75, 2.5], [-0.5, 2.5]], F32)  # outside [0, 1]: the lookup repeats
    s.add(pa.Mesh(verts, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), texcoords=uvs), "quad")
    s.set(pa.ThinLenCamera(pa.Film(list(size or FILMS["tex_room_48x32_s8_d4"][0]), pa.Uncharted2()), [0, 1.5, -1.9], [0, 1.2, 2], 0.9))
    return s


# name: (size, spp, depth) -- tests/golden/textured_quad.glb (tools/make_texture_glb.py), loaded by the reference's own importer
GLB_FILMS = {"tex_glb_40x30_s4_d3": ((40, 30), 4, 3)}


def glb_scene(gltf, path, size):
    """The import of `path` with the camera the importer set -- its film is 640 high -- on a film of `size`."""
    import pine_amd as pa
    s = gltf.load(path)
    c = s.camera
    s.set(pa.ThinLenCamera(pa.Film(list(size), pa.Uncharted2()), c.frm, c.to, c.fov))
    return s


SCRIPT_PNGS = {"ramp8_16x16": "texture_ramp8_16x16.png", "rgba8_7x4": "texture_rgba8_7x4.png"}  # under tests/golden/


def script_room(size=None):
    """The room as examples/textured.pine builds it: a script has no Mesh constructor, so there is no quad; its 8-bit images are
    PNG files (ImagePtr("x.png"): 3 channels, an RGBA file's alpha dropped), its float image ImagePtr(vec3); a Texture stands in a
    Nodef slot (Metal's roughness), where it reads as the texel's first component."""
    import os
    import pine_amd as pa
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ramp = pa.Image(os.path.join(golden, SCRIPT_PNGS["ramp8_16x16"]))
    rgba = pa.Image(os.path.join(golden, SCRIPT_PNGS["rgba8_7x4"]))
    one = pa.Image(np.array([[[0.875, 0.5, 0.25]]], F32))
    s = pa.Scene()
    s.add("floor", pa.Diffuse(pa.Texture(pa.UV() * 3.0, ramp)))
    back = pa.Texture(pa.UV(), rgba)
    s.add("back", pa.Uber([0.8, 0.7, 0.6], back[1], back[2], 0.0, 1.5))
    s.add("ball", pa.Diffuse(pa.Texture(pa.Position(), one) * 0.25))
    s.add("chrome", pa.Metal(pa.Texture(pa.UV(), ramp), pa.Texturef(pa.UV(), rgba)))
    s.add("white", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add("lamp", pa.Emissive([12.0, 11.0, 9.0]))
    s.add(pa.Rect([0, 0, 0], [4, 0, 0], [0, 0, 4], True), "floor")
    s.add(pa.Rect([0, 3, 0], [4, 0, 0], [0, 0, 4], False), "white")
    s.add(pa.Rect([0, 1.5, 2], [4, 0, 0], [0, 3, 0], True), "back")
    s.add(pa.Rect([0, 1.5, -2], [4, 0, 0], [0, 3, 0], False), "white")
    s.add(pa.Rect([-2, 1.5, 0], [0, 0, 4], [0, 3, 0], False), "white")
    s.add(pa.Rect([2, 1.5, 0], [0, 0, 4], [0, 3, 0], True), "white")
    s.add(pa.Rect([0, 2.99, 0], [1.2, 0, 0], [0, 0, 1.2], False), "lamp")
    s.add(pa.Sphere([-0.8, 0.6, 0.4], 0.6), "ball")
    s.add(pa.Sphere([0.875, 0.5, 0.25], 0.5), "chrome")
    s.set(pa.ThinLenCamera(pa.Film(list(size or FILMS["tex_script_room_48x32_s8_d4"][0]), pa.Uncharted2()), [0, 1.5, -1.875], [0, 1.2, 2], 0.875))
    return s


def film_scene(name):
    return script_room(FILMS[name][0]) if name.startswith("tex_script_room") else room(FILMS[name][0])


def film_images(name):
    """The texels of the film scene's images, in the scene's order, as the reference's driver takes them."""
    if name.startswith("tex_script_room"):
        return [image("ramp8_16x16"), np.ascontiguousarray(image("rgba8_7x4")[..., :3]), np.array([[[0.875, 0.5, 0.25]]], F32)]
    return [image(n) for n in ("ramp8_16x16", "rgba8_7x4", "f32_3x5")]
