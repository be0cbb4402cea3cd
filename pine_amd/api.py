"""Host-side mirror of the reference's script-visible interface for the PathIntegrator path.

Names, argument order and error behaviour follow what a `.pine` script sees (registered in
src/pine/core/program_context.cpp:23-125 and the *_context functions it calls), e.g.

    scene = Scene()
    scene.add("floor", Diffuse([0.9, 0.9, 0.9]))
    scene.add(Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], True), "floor")
    scene.set(ThinLenCamera(Film([640, 640], Uncharted2()), [0, 0, 0], [0, 0, 1], 0.4))
    PathIntegrator(BlueSampler(256), 8).render(scene)
    scene.camera.film().save("images/cbox.png")

Everything here is plumbing over the C ABI (include/pine_gpu.h); all arithmetic that feeds the
render (shape constructors, matrices, camera, BVH) happens in libpine_gpu.so.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib, check, PineError, f3, f16


def _v3(v):
    v = list(v)
    if len(v) != 3:
        raise PineError("expected a vec3")
    return f3(*[float(x) for x in v])


# ---- mat4 (PRL builtins translate/rotate_*/scale/look_at, vecmath.h:1102-1180) -----------------
class mat4:
    """Column-vector 4x4 float matrix in the reference's storage order (m[c*4 + r])."""

    def __init__(self, storage=None):
        self.s = f16()
        if storage is None:
            lib.pine_gpu_mat4_identity(self.s)
        else:
            for i, x in enumerate(storage):
                self.s[i] = float(x)

    def __mul__(self, other):
        out = mat4()
        lib.pine_gpu_mat4_mul(self.s, other.s, out.s)
        return out

    def numpy(self):
        """4x4 array indexed [row, col]."""
        return np.array(list(self.s), dtype=np.float32).reshape(4, 4).T.copy()


def translate(v):
    out = mat4()
    lib.pine_gpu_mat4_translate(_v3(v), out.s)
    return out


def scale(v):
    out = mat4()
    lib.pine_gpu_mat4_scale(_v3(v), out.s)
    return out


def rotate_x(rad):
    out = mat4()
    lib.pine_gpu_mat4_rotate_x(float(rad), out.s)
    return out


def rotate_y(rad):
    out = mat4()
    lib.pine_gpu_mat4_rotate_y(float(rad), out.s)
    return out


def rotate_z(rad):
    out = mat4()
    lib.pine_gpu_mat4_rotate_z(float(rad), out.s)
    return out


def inverse(m):
    out = mat4()
    lib.pine_gpu_mat4_inverse(m.s, out.s)
    return out


def look_at(frm, to):
    out = mat4()
    lib.pine_gpu_mat4_look_at(_v3(frm), _v3(to), out.s)
    return out


# ---- materials (src/pine/core/material.cpp:46-62) ---------------------------------------------
# ---- shading nodes (src/pine/core/node.h:13-297, node.cpp:29-116) --------------------------------
class Node:
    """A Nodef (is_vec3 False) or Node3f (True) expression; built lazily, instantiated in a scene's node
    table when a material using it is added.  Operators compose nodes the way node.cpp:70-102 does."""
    is_vec3 = False

    def __init__(self, kind, *args, is_vec3=False):
        self.kind, self.args, self.is_vec3 = kind, args, is_vec3

    @staticmethod
    def of(x, want_vec3=None):
        if isinstance(x, Node):
            n = x
        elif isinstance(x, (int, float, np.floating)):
            n = Node("constf", float(np.float32(x)))
        else:
            n = Node("const3", [float(np.float32(v)) for v in x], is_vec3=True)
        if want_vec3 is True and not n.is_vec3:
            n = Node("splat", n, is_vec3=True)     # Node3f(Nodef): vec3{x.eval} (node.h:78,291-293)
        if want_vec3 is False and n.is_vec3:
            raise PineError("a Nodef is required here")
        return n

    def _bin(self, op, other, swap=False):
        o = Node.of(other)
        a, b = (o, self) if swap else (self, o)
        v = a.is_vec3 or b.is_vec3
        return Node("bin", op, Node.of(a, v), Node.of(b, v), is_vec3=v)

    def __add__(self, o): return self._bin("+", o)
    def __radd__(self, o): return self._bin("+", o, True)
    def __sub__(self, o): return self._bin("-", o)
    def __rsub__(self, o): return self._bin("-", o, True)
    def __mul__(self, o): return self._bin("*", o)
    def __rmul__(self, o): return self._bin("*", o, True)
    def __truediv__(self, o): return self._bin("/", o)
    def __rtruediv__(self, o): return self._bin("/", o, True)
    def __pow__(self, o): return self._bin("^", o)
    def __neg__(self): return Node("un", "-", self, is_vec3=self.is_vec3)
    def __getitem__(self, n):
        if not 0 <= int(n) <= 2:  # node.h:181-182 (and what ends an iteration over a node, which would never stop)
            raise PineError(f"NodeComponent's second parameter should be 0, 1, or 2, but get {int(n)}")
        if not self.is_vec3:
            raise PineError("a Node3f is required here")
        return Node("comp", self, int(n))

    def _instantiate(self, scene, memo):
        if id(self) in memo:
            return memo[id(self)][1]
        h, k, a = scene._h, self.kind, self.args
        sub = lambda x: x._instantiate(scene, memo)  # noqa: E731
        if k == "constf":
            r = lib.pine_gpu_scene_node_constf(h, float(a[0]))
        elif k == "const3":
            r = lib.pine_gpu_scene_node_const3(h, _v3(a[0]))
        elif k in ("position", "normal", "uv"):
            r = lib.pine_gpu_scene_node_input(h, {"position": 0, "normal": 1, "uv": 2}[k])
        elif k == "bin":
            r = lib.pine_gpu_scene_node_binary(h, ord(a[0]), sub(a[1]), sub(a[2]))
        elif k == "un":
            r = lib.pine_gpu_scene_node_unary(h, ord(a[0]), sub(a[1]))
        elif k == "comp":
            r = lib.pine_gpu_scene_node_component(h, sub(a[0]), a[1])
        elif k == "tovec3":
            ids = [sub(x) for x in a]
            r = lib.pine_gpu_scene_node_to_vec3(h, ids[0], ids[1] if len(ids) == 3 else -1, ids[2] if len(ids) == 3 else -1)
        elif k == "checker":
            r = lib.pine_gpu_scene_node_checkerboard(h, sub(a[0]), float(a[1]))
        elif k == "splat":
            r = lib.pine_gpu_scene_node_splat(h, sub(a[0]))
        elif k in ("image", "imagef"):
            p = sub(a[0])
            fn = lib.pine_gpu_scene_node_image if k == "image" else lib.pine_gpu_scene_node_imagef
            r = fn(h, p, a[1]._instantiate(scene))
        elif k in ("noisef", "noise3f"):
            p = sub(a[0])
            fn = lib.pine_gpu_scene_node_noisef if k == "noisef" else lib.pine_gpu_scene_node_noise3f
            r = fn(h, p, sub(a[1]))
        else:
            raise PineError("unknown node kind " + k)
        memo[id(self)] = (self, check(r, "node"))  # (keeps the node alive: ids of dead temporaries get reused)
        return memo[id(self)][1]


class Image:
    """An image for Texture / Texturef (image.h:11-25), rows as loaded: an (h, w, 3) float32 array (kept as it is), an
    (h, w, 3) or (h, w, 4) uint8 array (a texel reads as pow(value / 255, 2.2); alpha never reaches a result), or the path of
    a Radiance .hdr or a .png file (pine_amd/png.py: expanded to 3 channels, as the reference's image_from loads it).  One
    Image object is one image of a scene however many nodes look it up."""
    def __init__(self, array_or_path):
        a = array_or_path
        if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__"):
            path = os.fsdecode(a)
            with open(path, "rb") as f:
                head = f.read(8)
            if head == b"\x89PNG\r\n\x1a\n":
                from .png import read_png
                a = read_png(path, 3)
            elif head[:2] == b"#?":
                from .hdr import read_hdr
                a = read_hdr(path)
            elif head[:3] == b"\xff\xd8\xff":
                raise PineError(f"{path}: JPEG images are not supported (a lossy format; use PNG or Radiance .hdr)")
            else:
                raise PineError(f"{path}: neither a PNG nor a Radiance .hdr file")
        a = np.asarray(a)
        if a.dtype != np.uint8:
            a = a.astype(np.float32, copy=False)
        if a.ndim != 3 or a.shape[2] not in ((3, 4) if a.dtype == np.uint8 else (3,)):
            raise PineError("Image: expected (h, w, 3) float32 or (h, w, 3 | 4) uint8 texels")
        self.texels = np.ascontiguousarray(a)

    @staticmethod
    def of(x):
        return x if isinstance(x, Image) else Image(x)

    def _instantiate(self, scene):
        if id(self) not in scene._images:  # (the scene keeps the object alive: ids of dead temporaries get reused)
            t = self.texels
            h, w, ch = t.shape
            if t.dtype == np.uint8:
                r = lib.pine_gpu_scene_add_image_u8(scene._h, t.ctypes.data_as(C.POINTER(C.c_uint8)), ch, w, h)
            else:
                r = lib.pine_gpu_scene_add_image(scene._h, t.ctypes.data_as(_lib.c_f_p), w, h)
            scene._images[id(self)] = (self, check(r, "Image"))
        return scene._images[id(self)][1]


def Texture(p, image):
    """NodeImage (node.h:236-243, node.cpp:20-23): the rgb of the texel at min(vec2i(size * fract(vec2(p))), size - 1)."""
    return Node("image", Node.of(p, True), Image.of(image), is_vec3=True)


def Texturef(p, image):
    """NodeImagef (node.h:244-251, node.cpp:24-27): the same texel's first component."""
    return Node("imagef", Node.of(p, True), Image.of(image))


def Noisef(p, octaves):
    """NodeNoisef (node.h:209-216, node.cpp:7-9): fbm(p, int(octaves)), the reference's Perlin fbm; the first component of Noise3f."""
    return Node("noisef", Node.of(p, True), Node.of(octaves, False))


def Noise3f(p, octaves):
    """NodeNoise3f (node.h:218-225, node.cpp:11-13): fbm3d(p, int(octaves)), three channels of the same noise."""
    return Node("noise3f", Node.of(p, True), Node.of(octaves, False), is_vec3=True)


def Position(): return Node("position", is_vec3=True)
def Normal(): return Node("normal", is_vec3=True)
def UV(): return Node("uv", is_vec3=True)
def Checkerboard(p, ratio=0.5): return Node("checker", Node.of(p, True), float(np.float32(ratio)))
def Vec3(x, y=None, z=None):
    if y is None:
        return Node("tovec3", Node.of(x, False), is_vec3=True)
    return Node("tovec3", Node.of(x, False), Node.of(y, False), Node.of(z, False), is_vec3=True)
def node_abs(x): return Node("un", "a", Node.of(x), is_vec3=Node.of(x).is_vec3)
def node_sqr(x): return Node("un", "s", Node.of(x), is_vec3=Node.of(x).is_vec3)
def node_sqrt(x): return Node("un", "r", Node.of(x), is_vec3=Node.of(x).is_vec3)
def node_fract(x): return Node("un", "f", Node.of(x), is_vec3=Node.of(x).is_vec3)


def lerp(t, a, b):
    """lerp over nodes exactly as node.cpp:88-102 composes it (plain numbers lerp numerically)."""
    if not any(isinstance(x, Node) for x in (t, a, b)):
        raise PineError("lerp: at least one argument must be a node (use numpy for plain numbers)")
    t, a, b = Node.of(t), Node.of(a), Node.of(b)
    one = Node("constf", 1.0)
    if not t.is_vec3 and not a.is_vec3 and not b.is_vec3:      # (Nodef, Nodef, Nodef)
        return (t * b) + ((one - t) * a)
    if not t.is_vec3:                                           # (Nodef, Node3f, Node3f)
        return (Vec3(t) * Node.of(b, True)) + (Vec3(one - t) * Node.of(a, True))
    one3 = Node("const3", [1.0, 1.0, 1.0], is_vec3=True)        # (Node3f, Node3f, Node3f)
    return (t * Node.of(b, True)) + ((one3 - t) * Node.of(a, True))


class Material:
    pass


class Emissive(Material):
    def __init__(self, color):
        self.color = color


class Diffuse(Material):
    def __init__(self, albedo):
        self.albedo = albedo


class Uber(Material):
    def __init__(self, albedo, roughness, metallic=0.0, transmission=0.0, ior=1.45):
        self.albedo, self.roughness, self.metallic, self.transmission, self.ior = albedo, roughness, metallic, transmission, ior


class Subsurface(Material):
    def __init__(self, albedo, roughness, sigma_s):
        self.albedo, self.roughness, self.sigma_s = albedo, roughness, sigma_s


class Metal(Material):       # material.h:39-50
    def __init__(self, albedo, roughness):
        self.albedo, self.roughness = albedo, roughness


class Glossy(Material):      # material.h:52-64
    def __init__(self, albedo, roughness, ior=1.4):
        self.albedo, self.roughness, self.ior = albedo, roughness, ior


class Glass(Material):       # material.h:66-78
    def __init__(self, albedo, roughness, ior=1.4):
        self.albedo, self.roughness, self.ior = albedo, roughness, ior


# ---- lights other than emissive geometry (src/pine/core/light.h:21-67, light.cpp:173-186) ---------
class Light:
    pass


class PointLight(Light):
    def __init__(self, position, color):
        self.position, self.color = position, color


class SpotLight(Light):
    def __init__(self, position, direction, color, falloff_radian, cutoff_additional_radian=0.0):
        self.position, self.direction, self.color = position, direction, color
        self.falloff, self.cutoff_additional = falloff_radian, cutoff_additional_radian


class DirectionalLight(Light):
    def __init__(self, direction, color):
        self.direction, self.color = direction, color


class Sky:
    """EnvironmentLight Sky(sun_color): scene.set(Sky(...))."""
    def __init__(self, sun_color):
        self.sun_color = sun_color


class ImageSky:
    """EnvironmentLight ImageSky(image, tint, elevation, rotation) (light.h:81-94): scene.set(ImageSky(...)).  `image` is an
    (h, w, 3) float32 array (a Radiance HDR image as the reference loads it), an (h, w, 3) uint8 array (the reference's 8-bit
    images: each texel is pow(value / 255, 2.2)), rows top first, or the path of a Radiance .hdr file."""
    def __init__(self, image, tint=(1.0, 1.0, 1.0), elevation=0.0, rotation=0.0):
        if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
            from .hdr import read_hdr
            image = read_hdr(image)
        image = np.asarray(image)
        if image.dtype != np.uint8:
            image = image.astype(np.float32, copy=False)
        if image.ndim != 3 or image.shape[2] != 3:
            raise PineError("ImageSky: expected an (h, w, 3) image")
        self.image = np.ascontiguousarray(image)
        self.tint, self.elevation, self.rotation = tint, elevation, rotation


class Atmosphere:
    """EnvironmentLight Atmosphere(sun_direction, sun_color) (light.h:69-79): scene.set(Atmosphere(...)).  A single-scattering
    Rayleigh / Mie sky with a sun disc.  image_size is the grid its importance sampling is tabulated on -- the reference's is
    1024 x 1024, and its scripts cannot change it.  device: the HIP device that computes the light's tables when it is set
    (None: host threads; the same bytes either way)."""
    def __init__(self, sun_direction, sun_color, image_size=(1024, 1024), device=None):
        self.sun_direction, self.sun_color = sun_direction, sun_color
        self.image_size = (int(image_size[0]), int(image_size[1]))
        self.device = device


# ---- shapes (src/pine/core/geometry.cpp:901-946) ------------------------------------------------
class Shape:
    pass


class Rect(Shape):
    def __init__(self, position, ex, ey, flip_normal=False):
        self.position, self.ex, self.ey, self.flip_normal = position, ex, ey, flip_normal


class AABB(Shape):
    def __init__(self, lower, upper):
        self.lower, self.upper = lower, upper


class OBB(Shape):
    def __init__(self, aabb, m):
        self.aabb, self.m = aabb, m


def Box(*args):
    """Box(lower, upper) | Box(AABB, mat4) | Box(lower, upper, mat4) -- geometry.cpp:913-918."""
    if len(args) == 2 and isinstance(args[0], AABB):
        return OBB(args[0], args[1])
    if len(args) == 2:
        return AABB(args[0], args[1])
    if len(args) == 3:
        return OBB(AABB(args[0], args[1]), args[2])
    raise PineError("Box: no matching overload")


class Sphere(Shape):
    def __init__(self, center, radius):
        self.center, self.radius = center, radius


class Disk(Shape):
    def __init__(self, position, normal, radius):
        self.position, self.normal, self.radius = position, normal, radius


class Cone(Shape):
    def __init__(self, position, normal, radius, height):
        self.position, self.normal, self.radius, self.height = position, normal, radius, height


class Plane(Shape):
    """Plane(position, normal) geometry.cpp:31-34 (its bounding box is position +-100, geometry.cpp:52)"""
    def __init__(self, position, normal):
        self.position, self.normal = position, normal


class Line(Shape):
    """Line(p0, p1, thickness) geometry.cpp:171-179"""
    def __init__(self, p0, p1, thickness):
        self.p0, self.p1, self.thickness = p0, p1, thickness


class Cylinder(Shape):
    """Cylinder(p0, p1, r) geometry.h:139-157: side surface only, never a light"""
    def __init__(self, p0, p1, radius):
        self.p0, self.p1, self.radius = p0, p1, radius


class Triangle(Shape):
    """Triangle(v0, v1, v2) geometry.cpp:528-531"""
    def __init__(self, v0, v1, v2):
        self.v0, self.v1, self.v2 = v0, v1, v2


class Mesh(Shape):
    """Mesh(vertices, indices[, texcoords, normals]) geometry.cpp:596-604: per-vertex normals give the interpolated shading
    normal, per-vertex texcoords replace the barycentric uv (geometry.h:199-210)."""
    def __init__(self, vertices, indices, texcoords=None, normals=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        self.normals = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        self.texcoords = None if texcoords is None else np.ascontiguousarray(texcoords, dtype=np.float32).reshape(-1, 2)
        for name, a in (("normals", self.normals), ("texcoords", self.texcoords)):
            if a is not None and len(a) != len(self.vertices):
                raise PineError(f"Mesh: {len(self.vertices)} vertices but {len(a)} {name}")  # CHECK_EQ geometry.cpp:602-603


# ---- film / camera / sampler -------------------------------------------------------------------
class Uncharted2:
    code = 0


class ACES:
    code = 1


class Film:
    """Film(size[, tonemapper]) -- src/pine/core/film.h:24-27.  pixels: H x W x 4 float32, row 0 first."""

    def __init__(self, size, tone_mapper=None):
        self.size = (int(size[0]), int(size[1]))
        self.tone_mapper = tone_mapper or Uncharted2()
        self.pixels = np.zeros((self.size[1], self.size[0], 4), dtype=np.float32)

    def width(self):
        return self.size[0]

    def height(self):
        return self.size[1]

    def finalize_u8(self):
        """film.finalize() + gamma + y-flip as save() does (film.cpp:12-27, fileio.cpp:42-54)."""
        w, h = self.size
        out = np.zeros((h, w, 4), dtype=np.uint8)
        src = np.ascontiguousarray(self.pixels, dtype=np.float32)
        check(lib.pine_gpu_film_finalize_u8(src.ctypes.data_as(_lib.c_f_p), w, h, self.tone_mapper.code,
                                            out.ctypes.data_as(C.POINTER(C.c_uint8))), "film.finalize")
        return out

    def save(self, filename):
        """scene.camera.film().save(path): 8-bit PNG of the tone-mapped film."""
        from . import png
        png.write_png(filename, self.finalize_u8())


class ThinLenCamera:
    def __init__(self, film, frm, to, fov, len_radius=0.0, focus_distance=1.0):
        self._film, self.frm, self.to, self.fov = film, frm, to, fov
        self.len_radius, self.focus_distance = len_radius, focus_distance

    def film(self):
        return self._film


class BlueSampler:
    """BlueSobolSampler: spp rounded up to a power of two and clamped to 256 (sampler.cpp:115-121)."""
    kind = 0  # PINE_GPU_SAMPLER_BLUE

    def __init__(self, samples_per_pixel):
        if samples_per_pixel <= 0:
            raise PineError("`BlueSampler` should have positive samples per pixel")
        self.requested = int(samples_per_pixel)

    def spp(self):
        n = min(self.requested, 256)
        p = 1
        while p < n:
            p *= 2
        return p


class SobolSampler:
    """SobolSampler(spp) (sampler.h:83-164): spp is used as given -- no rounding, no clamp to 256.  On the
    device any count up to 4096."""
    kind = 1  # PINE_GPU_SAMPLER_SOBOL

    def __init__(self, samples_per_pixel):
        self.requested = int(samples_per_pixel)

    def spp(self):
        return self.requested


class HaltonSampler:
    """HaltonSampler(spp) (sampler.h:40-81): scrambled radical inverses over the first primes, the pixel's place in the
    sequence from its coordinates modulo 128; spp as given (on the device up to 4096)."""
    kind = 2  # PINE_GPU_SAMPLER_HALTON

    def __init__(self, samples_per_pixel):
        if samples_per_pixel <= 0:
            raise PineError("`HaltonSampler` should have positive samples per pixel")
        self.requested = int(samples_per_pixel)

    def spp(self):
        return self.requested


# ---- Scene (src/pine/core/scene.cpp:64-79) -----------------------------------------------------
class Scene:
    def __init__(self):
        self._h = C.c_void_p(check(lib.pine_gpu_scene_create(), "Scene()"))
        self.camera = None
        self._anon = 0
        self._images = {}  # id(Image) -> (Image, its id in this scene): one Image object is stored once

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.pine_gpu_scene_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # scene.add(name, material) | scene.add(shape, material | name)
    def add(self, a, b=None):
        if isinstance(a, str) and isinstance(b, Material):
            return self._add_material(a, b)
        if isinstance(a, Light) and b is None:
            h = self._h
            if isinstance(a, PointLight):
                return check(lib.pine_gpu_scene_add_light_point(h, _v3(a.position), _v3(a.color)), "PointLight")
            if isinstance(a, SpotLight):
                return check(lib.pine_gpu_scene_add_light_spot(h, _v3(a.position), _v3(a.direction), _v3(a.color),
                                                               float(a.falloff), float(a.cutoff_additional)), "SpotLight")
            return check(lib.pine_gpu_scene_add_light_directional(h, _v3(a.direction), _v3(a.color)), "DirectionalLight")
        if isinstance(a, Shape):
            if isinstance(b, str):
                mid = check(lib.pine_gpu_scene_find_material(self._h, b.encode()), "scene.add")
            elif isinstance(b, Material):
                mid = self._add_material("", b)
            else:
                raise PineError("scene.add: second argument must be a material or a material name")
            return self._add_shape(a, mid)
        raise PineError("scene.add: no matching overload")

    def set(self, camera):
        if isinstance(camera, Sky):
            check(lib.pine_gpu_scene_set_env_sky(self._h, _v3(camera.sun_color)), "scene.set")
            return camera
        if isinstance(camera, ImageSky):
            img = camera.image
            h, w = img.shape[:2]
            args = (w, h, _v3(camera.tint), float(camera.elevation), float(camera.rotation))
            if img.dtype == np.uint8:
                check(lib.pine_gpu_scene_set_env_image_u8(self._h, img.ctypes.data_as(C.POINTER(C.c_uint8)), *args), "scene.set")
            else:
                check(lib.pine_gpu_scene_set_env_image(self._h, img.ctypes.data_as(C.POINTER(C.c_float)), *args), "scene.set")
            return camera
        if isinstance(camera, Atmosphere):
            device = -1 if camera.device is None else int(camera.device)
            check(lib.pine_gpu_scene_set_env_atmosphere(self._h, _v3(camera.sun_direction), _v3(camera.sun_color), camera.image_size[0],
                                                        camera.image_size[1], device), "scene.set")
            return camera
        if not isinstance(camera, ThinLenCamera):
            raise PineError("scene.set: expected a camera")
        f = camera.film()
        check(lib.pine_gpu_scene_set_camera_thinlens(self._h, f.size[0], f.size[1], f.tone_mapper.code,
                                                     _v3(camera.frm), _v3(camera.to), float(camera.fov),
                                                     float(camera.len_radius), float(camera.focus_distance)),
              "scene.set")
        self.camera = camera
        return camera

    def _add_material(self, name, m):
        n = name.encode()
        if isinstance(m, (Emissive, Subsurface)) and any(isinstance(x, Node) for x in vars(m).values()):
            raise PineError(type(m).__name__ + ": a constant colour / albedo / roughness is required (no node-driven entry point)")
        if isinstance(m, Emissive):
            return check(lib.pine_gpu_scene_add_material_emissive(self._h, n, _v3(m.color)), "Emissive")
        memo = {}
        nid = lambda x, v: Node.of(x, v)._instantiate(self, memo)  # noqa: E731
        if isinstance(m, Diffuse) and isinstance(m.albedo, Node):
            return check(lib.pine_gpu_scene_add_material_diffuse_n(self._h, n, nid(m.albedo, True)), "Diffuse")
        if isinstance(m, Uber) and any(isinstance(x, Node) for x in (m.albedo, m.roughness, m.metallic, m.transmission)):
            return check(lib.pine_gpu_scene_add_material_uber_n(self._h, n, nid(m.albedo, True), nid(m.roughness, False),
                                                                nid(m.metallic, False), nid(m.transmission, False), float(m.ior)), "Uber")
        if isinstance(m, Metal):
            return check(lib.pine_gpu_scene_add_material_metal(self._h, n, nid(m.albedo, True), nid(m.roughness, False)), "Metal")
        if isinstance(m, Glossy):
            return check(lib.pine_gpu_scene_add_material_glossy(self._h, n, nid(m.albedo, True), nid(m.roughness, False),
                                                                nid(m.ior, False)), "Glossy")
        if isinstance(m, Glass):
            return check(lib.pine_gpu_scene_add_material_glass(self._h, n, nid(m.albedo, True), nid(m.roughness, False),
                                                               nid(m.ior, False)), "Glass")
        if isinstance(m, Diffuse):
            return check(lib.pine_gpu_scene_add_material_diffuse(self._h, n, _v3(m.albedo)), "Diffuse")
        if isinstance(m, Uber):
            return check(lib.pine_gpu_scene_add_material_uber(self._h, n, _v3(m.albedo), float(m.roughness),
                                                              float(m.metallic), float(m.transmission), float(m.ior)), "Uber")
        if isinstance(m, Subsurface):
            return check(lib.pine_gpu_scene_add_material_subsurface(self._h, n, _v3(m.albedo), float(m.roughness),
                                                                    _v3(m.sigma_s)), "Subsurface")
        raise PineError("unsupported material")

    def _add_shape(self, s, mid):
        h = self._h
        if isinstance(s, Rect):
            return check(lib.pine_gpu_scene_add_rect(h, _v3(s.position), _v3(s.ex), _v3(s.ey), int(bool(s.flip_normal)), mid), "Rect")
        if isinstance(s, AABB):
            return check(lib.pine_gpu_scene_add_aabb(h, _v3(s.lower), _v3(s.upper), mid), "Box")
        if isinstance(s, OBB):
            return check(lib.pine_gpu_scene_add_obb(h, _v3(s.aabb.lower), _v3(s.aabb.upper), s.m.s, mid), "Box")
        if isinstance(s, Sphere):
            return check(lib.pine_gpu_scene_add_sphere(h, _v3(s.center), float(s.radius), mid), "Sphere")
        if isinstance(s, Disk):
            return check(lib.pine_gpu_scene_add_disk(h, _v3(s.position), _v3(s.normal), float(s.radius), mid), "Disk")
        if isinstance(s, Cone):
            return check(lib.pine_gpu_scene_add_cone(h, _v3(s.position), _v3(s.normal), float(s.radius), float(s.height), mid), "Cone")
        if isinstance(s, Plane):
            return check(lib.pine_gpu_scene_add_plane(h, _v3(s.position), _v3(s.normal), mid), "Plane")
        if isinstance(s, Line):
            return check(lib.pine_gpu_scene_add_line(h, _v3(s.p0), _v3(s.p1), float(s.thickness), mid), "Line")
        if isinstance(s, Cylinder):
            return check(lib.pine_gpu_scene_add_cylinder(h, _v3(s.p0), _v3(s.p1), float(s.radius), mid), "Cylinder")
        if isinstance(s, Triangle):
            return check(lib.pine_gpu_scene_add_triangle(h, _v3(s.v0), _v3(s.v1), _v3(s.v2), mid), "Triangle")
        if isinstance(s, Mesh):
            if s.normals is not None or s.texcoords is not None:
                return check(lib.pine_gpu_scene_add_mesh_full(
                    h, s.vertices.ctypes.data_as(_lib.c_f_p), len(s.vertices), s.indices.ctypes.data_as(C.POINTER(C.c_uint32)), len(s.indices),
                    s.normals.ctypes.data_as(_lib.c_f_p) if s.normals is not None else None,
                    s.texcoords.ctypes.data_as(_lib.c_f_p) if s.texcoords is not None else None, mid), "Mesh")
            return check(lib.pine_gpu_scene_add_mesh(h, s.vertices.ctypes.data_as(_lib.c_f_p), len(s.vertices),
                                                     s.indices.ctypes.data_as(C.POINTER(C.c_uint32)), len(s.indices), mid), "Mesh")
        raise PineError("unsupported shape")

    def describe(self) -> str:
        """The scene as .pscene text (exchange format shared with the oracle and the reference driver)."""
        n = check(lib.pine_gpu_scene_describe(self._h, None, 0), "describe")
        buf = C.create_string_buffer(n + 1)
        lib.pine_gpu_scene_describe(self._h, buf, n + 1)
        return buf.value.decode()


# ---- PathIntegrator (program_context.cpp:76-81) -------------------------------------------------
def _specialize_flags(specialize):
    if specialize is None:
        return 0
    return _lib.FLAG_SPECIALIZE if specialize else _lib.FLAG_NO_SPECIALIZE


def _order_flags(order):
    if order in (None, "pine", "bvh"):
        return 0
    if order in ("embree", "nearest"):  # ("nearest": this order's former name)
        return _lib.FLAG_ORDER_EMBREE
    raise PineError(f"unknown traversal order {order!r} (pine | embree)")


class Plan:
    """A PathIntegrator bound to a scene with all device state resident (bench / multi-GPU)."""

    def __init__(self, scene, spp, max_path_length, device=0, shard_rank=0, shard_world=1,
                 samples_per_item=0, timing=False, sampler="blue", flags=0, specialize=None, order="pine", pass_samples=None,
                 integrator="path"):
        """integrator: "path" -- PathIntegrator; "ao" -- AOIntegrator(BVH(), sampler) (pine_gpu_ao_plan_create: max_path_length,
        samples_per_item, specialize and pass_samples do not apply; launch / stats / check work, the packed launch and
        read_samples raise).
        spp: an int (BlueSampler(spp), or SobolSampler(spp) with sampler="sobol") or a sampler object.
        specialize: None -- the library's default: the scene's own kernel from the cache, else compiled in the background
        while the precompiled kernel renders; True -- PINE_GPU_FLAG_SPECIALIZE: wait for the compiler at plan creation, fail if
        the kernel cannot be built; False -- PINE_GPU_FLAG_NO_SPECIALIZE: precompiled kernels only (stats().specialized tells).
        order: "pine" -- closest hits in pine-BVH order, Accel(BVH()) (the default and the parity gate); "embree" --
        PINE_GPU_FLAG_ORDER_EMBREE: the order of the reference's default accel, EmbreeAccel (order-dependent shapes appear as under it).
        pass_samples: render in passes of about this many samples per pixel (pine_gpu_plan_create_passes): launch_pass(j, ...)
        for j = 0 .. pass_count - 1 folds each pass into a running film; the last one leaves the film launch() of an ordinary
        plan writes, bit for bit, with sample and checkpoint buffers sized for one pass.  None: an ordinary plan."""
        flags = int(flags) | _specialize_flags(specialize) | _order_flags(order)
        if scene.camera is None:
            raise PineError("scene has no camera")
        self.scene = scene
        kind = {"sobol": 1, "halton": 2}.get(sampler, 0)
        if hasattr(spp, "requested"):
            kind, spp = getattr(spp, "kind", 0), spp.requested
        self.params = _lib.RenderParams(int(spp), int(max_path_length), int(device), int(shard_rank),
                                        int(shard_world), int(samples_per_item),
                                        (_lib.FLAG_TIMING if timing else 0) | int(flags), kind)
        if integrator not in ("path", "ao"):
            raise PineError(f"unknown integrator {integrator!r} (path | ao)")
        if integrator == "ao":
            if pass_samples is not None:
                raise PineError("AOIntegrator: a plan with passes is not available")
            h = lib.pine_gpu_ao_plan_create(scene._h, C.byref(self.params))
            if not h:
                raise PineError("AOIntegrator: " + _lib.last_error())
        elif pass_samples is None:
            h = lib.pine_gpu_plan_create(scene._h, C.byref(self.params))
        else:
            h = lib.pine_gpu_plan_create_passes(scene._h, C.byref(self.params), int(pass_samples))
        if not h:
            raise PineError("PathIntegrator: " + _lib.last_error())
        self._h = C.c_void_p(h)

    def launch(self, film_dev_ptr, stream_ptr=0):
        """One whole render (a plan with passes: all of them, in order)."""
        check(lib.pine_gpu_plan_launch(self._h, C.c_void_p(film_dev_ptr), C.c_void_p(stream_ptr)), "render")

    @property
    def pass_count(self):
        return check(lib.pine_gpu_plan_pass_count(self._h), "pass_count")

    def pass_info(self, j):
        """(first sample, samples, first whole-pixel tile, tiles) of pass j."""
        out = (C.c_int32 * 4)()
        check(lib.pine_gpu_plan_pass_info(self._h, int(j), out), "pass_info")
        return tuple(out)

    def launch_pass(self, j, film_dev_ptr, stream_ptr=0):
        """Pass j (in order 0 .. pass_count - 1): the film holds the running result afterwards."""
        check(lib.pine_gpu_plan_launch_pass(self._h, int(j), C.c_void_p(film_dev_ptr), C.c_void_p(stream_ptr)), "render")

    def tile_order(self):
        """Film tile of every local tile, in the plan's order (pass_info's tile numbers index it)."""
        n = check(lib.pine_gpu_plan_tile_order(self._h, None, 0), "tile_order")
        out = (C.c_int32 * max(n, 1))()
        check(lib.pine_gpu_plan_tile_order(self._h, out, n), "tile_order")
        return list(out[:n])

    def device_bytes(self):
        """Bytes asked of the device: (sample rows, RNG checkpoints, running sum + carried RNG states, all plan buffers)."""
        out = (C.c_int64 * 4)()
        check(lib.pine_gpu_plan_device_bytes(self._h, out), "device_bytes")
        return tuple(out)

    def launch_packed(self, slab_dev_ptr, stream_ptr=0):
        """Multi-GPU form: write only this rank's tiles, tile-major, into a slab of slab_floats() floats."""
        check(lib.pine_gpu_plan_launch_packed(self._h, C.c_void_p(slab_dev_ptr), C.c_void_p(stream_ptr)), "render")

    def slab_floats(self):
        w, h = self.scene.camera.film().size
        return int(lib.pine_gpu_packed_slab_floats(w, h, self.params.shard_world))

    def check(self):
        """Wait for the last launch; raises PineError if its path kernel bailed out (incomplete film)."""
        check(lib.pine_gpu_plan_check(self._h), "render")

    def stats(self):
        st = _lib.PlanStats()
        check(lib.pine_gpu_plan_stats_get(self._h, C.byref(st)), "stats")
        return st

    def read_samples(self):
        w, h = self.scene.camera.film().size
        spp = self.stats().spp_effective
        out = np.zeros((h, w, spp, 4), dtype=np.float32)
        check(lib.pine_gpu_plan_read_samples(self._h, out.ctypes.data_as(_lib.c_f_p), out.size), "read_samples")
        return out

    def denoise(self, film, **params):
        """Denoise a film this plan rendered, on the device: `film` is a float32 CUDA tensor of shape (H, W, 4); the guide images
        are rendered into device memory and the filter runs in place (pine_gpu_guides_render_device, pine_gpu_denoise_device).
        Returns `film`."""
        import torch
        w, h = self.scene.camera.film().size
        if tuple(film.shape) != (h, w, 4) or film.dtype != torch.float32 or not film.is_cuda or not film.is_contiguous():
            raise PineError("Plan.denoise: a contiguous float32 CUDA tensor of shape (H, W, 4) is expected")
        params.setdefault("device", self.params.device)
        prm = denoise_params(**params)
        stream = C.c_void_p(torch.cuda.current_stream(film.device).cuda_stream)
        albedo = torch.empty((h, w, 3), dtype=torch.float32, device=film.device)
        normal = torch.empty((h, w, 3), dtype=torch.float32, device=film.device)
        rp = _lib.RenderParams(1, 1, int(prm.device), 0, 1, 0, 0, 0)
        check(lib.pine_gpu_guides_render_device(self.scene._h, C.byref(rp), C.c_void_p(albedo.data_ptr()), C.c_void_p(normal.data_ptr()), stream), "guides")
        check(lib.pine_gpu_denoise_device(C.byref(prm), w, h, C.c_void_p(film.data_ptr()), C.c_void_p(albedo.data_ptr()), C.c_void_p(normal.data_ptr()),
                                          C.c_void_p(film.data_ptr()), stream), "denoise")
        return film

    def close(self):
        if getattr(self, "_h", None):
            lib.pine_gpu_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def film_unpack(size, world, slabs_dev_ptr, film_dev_ptr, device=0, stream_ptr=0):
    """Scatter gathered per-rank slabs ([rank][slab]) into the row-major film (device pointers)."""
    check(lib.pine_gpu_film_unpack(int(size[0]), int(size[1]), int(world), int(device), C.c_void_p(slabs_dev_ptr),
                                   C.c_void_p(film_dev_ptr), C.c_void_p(stream_ptr)), "film_unpack")


def packed_offset(size, world, x, y):
    """(rank, float4 index inside that rank's slab) of pixel (x, y): host statement of the slab layout."""
    r, o = C.c_int(0), C.c_int64(0)
    check(lib.pine_gpu_packed_offset(int(size[0]), int(size[1]), int(world), int(x), int(y), C.byref(r), C.byref(o)), "packed_offset")
    return r.value, o.value


class PathIntegrator:
    """PathIntegrator(sampler, max_path_length).render(scene) -- the convenience overload a .pine
    script uses (program_context.cpp:79-81); pine-BVH traversal order, UniformLightSampler."""

    def __init__(self, sampler, max_path_length, device=0, flags=0, devices=None, specialize=None, order="pine"):
        """devices: a list of HIP device ordinals -- the film is rendered by all of them from this one process
        (pine_gpu_path_render_devices); default: the single `device`.
        specialize: None / True / False as for Plan (the scene's own kernel: automatic / required / never; same film).
        order: "pine" (Accel(BVH()), the default) or "embree" (PINE_GPU_FLAG_ORDER_EMBREE: what the reference's EmbreeAccel does)."""
        flags = int(flags) | _specialize_flags(specialize) | _order_flags(order)
        if max_path_length <= 0:  # path.cpp:12-13
            raise PineError(f"`PathIntegrator` expect `max_path_length` to be positive, get {max_path_length}")
        self.sampler, self.max_path_length, self.device, self.flags = sampler, int(max_path_length), device, int(flags)
        self.devices = list(devices) if devices else None

    def render(self, scene, pass_samples=None, on_pass=None, denoise=False):
        """denoise: filter the finished film with the scene's guide images (guides + denoise with default parameters, or with
        the parameters of a dict), as DenoiseIntegrator(...).render(scene) afterwards would.
        pass_samples: render in passes of about that many samples per pixel (one device); on_pass(j, n, film) is called
        with the running film (an (H, W, 4) array, valid during the call) after every pass and stops the render by
        returning something true -- the film returned is then the last one delivered.  The finished film is the same, bit
        for bit, with or without passes."""
        if denoise:
            film = self.render(scene, pass_samples, on_pass)
            if getattr(self, "stopped", False) and (pass_samples is not None or on_pass is not None):
                return film
            params = dict(denoise) if isinstance(denoise, dict) else {}
            params.setdefault("device", self.device)
            return DenoiseIntegrator(**params).render(scene)
        if scene.camera is None:
            raise PineError("scene has no camera")
        film = scene.camera.film()
        prm = _lib.RenderParams(self.sampler.requested, self.max_path_length, self.device, 0, 1, 0, self.flags,
                                getattr(self.sampler, "kind", 0))
        out = np.zeros((film.size[1], film.size[0], 4), dtype=np.float32)
        if pass_samples is not None or on_pass is not None:
            if self.devices:
                raise PineError("PathIntegrator.render: passes render on one device")
            self.stopped = False

            def _cb(_user, j, n, _film):
                return 1 if (on_pass is not None and on_pass(j, n, out)) else 0
            rc = check(lib.pine_gpu_path_render_passes(scene._h, C.byref(prm), int(pass_samples or 0), out.ctypes.data_as(_lib.c_f_p),
                                                       _lib.PASS_CALLBACK(_cb), None), "PathIntegrator.render")
            self.stopped = rc == _lib.RENDER_STOPPED
            film.pixels = out
            return film
        if self.devices:
            arr = (C.c_int * len(self.devices))(*self.devices)
            check(lib.pine_gpu_path_render_devices(scene._h, C.byref(prm), arr, len(self.devices), out.ctypes.data_as(_lib.c_f_p)),
                  "PathIntegrator.render")
            film.pixels = out
            return film
        check(lib.pine_gpu_path_render(scene._h, C.byref(prm), out.ctypes.data_as(_lib.c_f_p)), "PathIntegrator.render")
        film.pixels = out
        return film


# ---- AOIntegrator (program_context.cpp:58-61, src/pine/impl/integrator/ao.h, ao.cpp) ---------------
def ao_constants(scene):
    """(radius, directions[8]) of an AOIntegrator render of `scene`, computed on the host (pine_gpu_ao_constants)."""
    out = np.zeros(25, dtype=np.float32)
    check(lib.pine_gpu_ao_constants(scene._h, out.ctypes.data_as(_lib.c_f_p)), "AOIntegrator")
    return out[0], out[1:].reshape(8, 3)


class AOIntegrator:
    """AOIntegrator(BVH(), sampler).render(scene): ambient occlusion -- per camera sample the fraction of eight rays of
    length min_value(scene.get_aabb().diagonal()) / 2 around the hit point that meet nothing.  The integrator renders
    max(sampler.spp() / 8, 1) samples per pixel (ao.cpp:13); the sampler keeps its own count.  Materials and lights play no
    part.  pine-BVH order only: the reference's EmbreeAccel answers the eight rays with Embree's packet traversal, which is
    not restated."""

    def __init__(self, sampler, device=0, flags=0, order="pine"):
        if _order_flags(order):
            raise PineError("AOIntegrator renders in pine-BVH order only: AOIntegrator(BVH(), sampler) "
                            "(EmbreeAccel's hit8 is Embree's packet traversal, not restated)")
        self.sampler, self.device, self.flags = sampler, device, int(flags)

    @property
    def spp(self):
        """The AO sample count: max(sampler.spp() / 8, 1)."""
        return max(self.sampler.spp() // 8, 1)

    def render(self, scene):
        if scene.camera is None:
            raise PineError("scene has no camera")
        film = scene.camera.film()
        prm = _lib.RenderParams(self.sampler.requested, 1, self.device, 0, 1, 0, self.flags, getattr(self.sampler, "kind", 0))
        out = np.zeros((film.size[1], film.size[0], 4), dtype=np.float32)
        check(lib.pine_gpu_ao_render(scene._h, C.byref(prm), out.ctypes.data_as(_lib.c_f_p)), "AOIntegrator.render")
        film.pixels = out
        return film


# ---- DenoiseIntegrator (src/pine/impl/integrator/denoiser.cpp, src/pine/core/denoise.h) -----------
def guides(scene, device=0, flags=0, order="pine"):
    """(albedo, normal) of DenoiseIntegrator's guide pass (denoiser.cpp:13-23): per pixel the albedo and the normal of the
    closest hit through the pixel centre, zeros on a miss; two (H, W, 3) arrays, bit for bit the reference's with
    Accel = BVH().  EmbreeAccel's order, sharded films and PINE_GPU_FLAG_FAST are refused."""
    if scene.camera is None:
        raise PineError("scene has no camera")
    w, h = scene.camera.film().size
    prm = _lib.RenderParams(1, 1, int(device), 0, 1, 0, int(flags) | _order_flags(order), 0)
    albedo = np.zeros((h, w, 3), dtype=np.float32)
    normal = np.zeros((h, w, 3), dtype=np.float32)
    check(lib.pine_gpu_guides_render(scene._h, C.byref(prm), albedo.ctypes.data_as(_lib.c_f_p), normal.ctypes.data_as(_lib.c_f_p)), "guides")
    return albedo, normal


def guides_variants():
    """Feature words (F_* bits) of the precompiled guide kernels, in the order of the first-fit search."""
    out = (C.c_uint32 * 16)()
    n = check(lib.pine_gpu_guides_variants(out, 16), "guides_variants")
    return list(out[:n])


def denoise_params(**params):
    """pine_gpu_denoise_params: the defaults (pine_gpu_denoise_params_default) with `params` over them -- iterations (0 ... 8),
    normal_power_log2, sigma_color, sigma_albedo, eps_albedo, device (-1: the host-thread build)."""
    prm = _lib.DenoiseParams()
    lib.pine_gpu_denoise_params_default(C.byref(prm))
    names = [f[0] for f in _lib.DenoiseParams._fields_]
    for k, v in params.items():
        if k not in names:
            raise PineError(f"denoise: unknown parameter {k!r} ({', '.join(names)})")
        setattr(prm, k, v)
    return prm


def denoise(film, albedo, normal, **params):
    """The edge-avoiding a-trous filter (pine_amd/csrc/pine_denoise.h) of an (H, W, 4) film guided by the
    (H, W, 3) albedo and normal images; returns the filtered film (alpha kept, misses -- a zero normal -- copied through).
    device=-1: the host-thread build of the same functions, the same bytes."""
    pixels = film.pixels if isinstance(film, Film) else film
    pixels = np.ascontiguousarray(pixels, dtype=np.float32)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    if pixels.ndim != 3 or pixels.shape[2] != 4 or albedo.shape != pixels.shape[:2] + (3,) or normal.shape != albedo.shape:
        raise PineError("denoise: film is (H, W, 4), albedo and normal are (H, W, 3)")
    prm = denoise_params(**params)
    out = np.empty_like(pixels)
    fp = lambda a: a.ctypes.data_as(_lib.c_f_p)  # noqa: E731
    check(lib.pine_gpu_denoise(C.byref(prm), pixels.shape[1], pixels.shape[0], fp(pixels), fp(albedo), fp(normal), fp(out)), "denoise")
    return out


class DenoiseIntegrator:
    """DenoiseIntegrator(...).render(scene) (denoiser.cpp:9-27): computes the guide images and denoises, in place, the film the
    scene's camera already holds.  The reference hands the three images to Open Image Denoise; here the filter is
    pine_denoise.h's.  params: those of denoise(); device also selects where the guide pass runs."""

    def __init__(self, **params):
        self.params = dict(params)
        denoise_params(**self.params)  # (an unknown name raises here)

    def render(self, scene):
        if scene.camera is None:
            raise PineError("scene has no camera")
        film = scene.camera.film()
        albedo, normal = guides(scene, device=max(int(self.params.get("device", 0)), 0))
        film.pixels = denoise(film.pixels, albedo, normal, **self.params)
        return film


# ---- Accel: batched ray queries (src/pine/core/accel.h:10-25, core/integrator.h:31-38, :61-74) ----
HIT_DTYPE = np.dtype([("t", "<f4"), ("geometry", "<i4"), ("triangle", "<i4"), ("material", "<i4"), ("p", "<f4", 3), ("n", "<f4", 3),
                      ("uv", "<f4", 2)])
assert HIT_DTYPE.itemsize == 48


class AccelHits:
    """What Accel.intersect returns for a torch tensor of rays: `records`, an (N, 12) float32 tensor on the rays' device
    (include/pine_gpu.h has the layout), and views of its columns -- t, geometry, triangle, material (int32, -1 on a miss), p, n, uv."""

    def __init__(self, records):
        import torch
        self.records = records
        self.t = records[:, 0]
        self.geometry = records[:, 1].view(torch.int32)
        self.triangle = records[:, 2].view(torch.int32)
        self.material = records[:, 3].view(torch.int32)
        self.p = records[:, 4:7]
        self.n = records[:, 7:10]
        self.uv = records[:, 10:12]

    def __len__(self):
        return int(self.records.shape[0])


def _is_torch_tensor(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _check_rays(rays, device=None):
    """The (N, 8) float32 rays of an Accel query: a C-contiguous numpy array, or a contiguous CUDA torch tensor on the accel's
    device.  Anything else raises ValueError before anything is launched.  -> True for a torch tensor."""
    if _is_torch_tensor(rays):
        import torch
        if rays.dtype != torch.float32:
            raise ValueError(f"Accel: rays must be float32, not {rays.dtype}")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"Accel: rays must have shape (N, 8), not {tuple(rays.shape)}")
        if not rays.is_cuda:
            raise ValueError("Accel: a torch tensor of rays must live on the GPU (pass a numpy array for host rays)")
        if device is not None and rays.device.index != int(device):
            raise ValueError(f"Accel: the rays are on {rays.device}, the accel on device {int(device)}")
        if not rays.is_contiguous():
            raise ValueError("Accel: rays must be contiguous")
        return True
    if not isinstance(rays, np.ndarray):
        raise ValueError("Accel: rays must be a numpy array or a torch tensor")
    if rays.dtype != np.float32:
        raise ValueError(f"Accel: rays must be float32, not {rays.dtype}")
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError(f"Accel: rays must have shape (N, 8), not {rays.shape}")
    if not rays.flags["C_CONTIGUOUS"]:
        raise ValueError("Accel: rays must be C-contiguous")
    return False


def _check_tensor(t, what, dtype, shape, device=None):
    """A contiguous CUDA torch tensor of `dtype` and `shape` (None in a place: any size) on `device`, or ValueError -- before
    anything is launched."""
    if not _is_torch_tensor(t):
        raise ValueError(f"{what} must be a torch tensor, not {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, not {t.dtype}")
    if t.dim() != len(shape) or any(want is not None and int(have) != int(want) for have, want in zip(t.shape, shape)):
        raise ValueError(f"{what} must have shape {tuple('N' if d is None else int(d) for d in shape)}, not {tuple(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{what} must live on the GPU")
    if device is not None and t.device.index != int(device):
        raise ValueError(f"{what} are on {t.device}, not on device {int(device)}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    return t


class _SceneQuery:
    """What Accel and Shader share: the library's handle of the scene's records on the device (self._h), freed by close();
    a context manager.  A subclass names itself (_NAME) and the function that destroys its handle (_DESTROY)."""
    _NAME, _DESTROY = "", None

    def _handle(self):
        if not self._h:
            raise PineError(f"{self._NAME}: closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._DESTROY(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accel(_SceneQuery):
    """Accel(scene): the scene's BVH on the device, answering batches of rays -- what a CustomRayIntegrator's radiance() gets as
    intersect(ray, it) and hit(ray) (core/integrator.h:61-74).  One ray is a row of 8 float32: o, d, tmin, tmax; d is used as
    given (t is in units of d).  order: "pine" -- Accel(BVH()); "embree" -- Accel(EmbreeAccel()).  The answers are the
    reference's, bit for bit.  The accel is a snapshot of the scene at creation.  A context manager; close() frees the device
    memory."""
    _NAME, _DESTROY = "Accel", lib.pine_gpu_accel_destroy

    def __init__(self, scene, order="pine", device=0):
        self._h = None
        self.device = int(device)
        h = lib.pine_gpu_accel_create(scene._h, self.device, _order_flags(order))
        if not h:
            raise PineError("Accel: " + _lib.last_error())
        self._h = C.c_void_p(h)
        info = (C.c_int32 * 4)()
        check(lib.pine_gpu_accel_info(self._h, info), "Accel")
        self.kernel_features, self.lds_bytes, self.film_size = int(info[0]) & 0xFFFFFFFF, int(info[1]), (int(info[2]), int(info[3]))

    def intersect(self, rays, out=None):
        """Closest hits.  A numpy array in: a structured array of HIT_DTYPE out.  A CUDA tensor in: an AccelHits over a new
        (N, 12) tensor on its device (or over `out`, such a tensor of the caller's), enqueued on its current stream, nothing
        copied and nothing waited for."""
        if _check_rays(rays, self.device):
            import torch
            if out is None:
                out = torch.empty((rays.shape[0], 12), dtype=torch.float32, device=rays.device)
            else:
                _check_tensor(out, "Accel: the hit records", torch.float32, (rays.shape[0], 12), self.device)
            stream = C.c_void_p(torch.cuda.current_stream(rays.device).cuda_stream)
            check(lib.pine_gpu_accel_intersect_device(self._handle(), C.c_void_p(rays.data_ptr()), rays.shape[0], C.c_void_p(out.data_ptr()), stream),
                  "Accel.intersect")
            return AccelHits(out)
        out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        check(lib.pine_gpu_accel_intersect(self._handle(), rays.ctypes.data_as(_lib.c_f_p), rays.shape[0], out.ctypes.data_as(C.c_void_p)), "Accel.intersect")
        return out

    def hit(self, rays, out=None):
        """Any hit within [tmin, tmax): an (N,) bool array for a numpy array, an (N,) uint8 tensor (0 or 1) for a CUDA tensor
        (a new one, or `out`, such a tensor of the caller's)."""
        if _check_rays(rays, self.device):
            import torch
            if out is None:
                out = torch.empty((rays.shape[0],), dtype=torch.uint8, device=rays.device)
            else:
                _check_tensor(out, "Accel: the occlusion bytes", torch.uint8, (rays.shape[0],), self.device)
            stream = C.c_void_p(torch.cuda.current_stream(rays.device).cuda_stream)
            check(lib.pine_gpu_accel_hit_device(self._handle(), C.c_void_p(rays.data_ptr()), rays.shape[0], C.c_void_p(out.data_ptr()), stream), "Accel.hit")
            return out
        out = np.zeros(rays.shape[0], dtype=np.uint8)
        check(lib.pine_gpu_accel_hit(self._handle(), rays.ctypes.data_as(_lib.c_f_p), rays.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint8))), "Accel.hit")
        return out.view(np.bool_)

    def camera_rays(self, tensor=False):
        """The (H * W, 8) pixel-centre rays of the scene's camera, row-major: camera.gen_ray((p + 0.5) / film_size, (0.5, 0.5)),
        DenoiseIntegrator's guide rays (denoiser.cpp:13-23).  tensor=True: a CUDA tensor on the accel's device (written on the
        current stream); else a numpy array."""
        import torch
        w, h = self.film_size
        if w * h == 0:
            raise PineError("Accel.camera_rays: scene has no camera")
        dev = torch.device("cuda", self.device)
        rays = torch.empty((w * h, 8), dtype=torch.float32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        check(lib.pine_gpu_accel_camera_rays_device(self._handle(), C.c_void_p(rays.data_ptr()), stream), "Accel.camera_rays")
        return rays if tensor else rays.cpu().numpy()


# ---- Shader: batched path-vertex shading queries (core/integrator.h:27-74, impl/integrator/path.cpp:42-123) ----
# (pine_gpu_shader_layout reports the same: tests/test_shader.py)
SHADER_STATE_WORDS, SHADER_RECORD_WORDS, SHADER_RAY_FLOATS, SHADER_LOG_FLOATS = 8, 16, 8, 16
KIND_NONE, KIND_MISS, KIND_EMISSIVE, KIND_LIMIT, KIND_SHADED = -1, 0, 1, 2, 3
RECORD_DTYPE = np.dtype([("kind", "<i4"), ("length", "<i4"), ("flags", "<u4"), ("light_pdf", "<f4"), ("lo", "<f4", 3), ("cosine", "<f4"),
                         ("direct", "<f4", 3), ("pdf", "<f4"), ("f", "<f4", 3), ("is_delta", "<f4")])
assert RECORD_DTYPE.itemsize == 4 * SHADER_RECORD_WORDS


class ShaderRecords:
    """What Shader.vertex writes: `records`, an (N, 16) float32 tensor (include/pine_gpu.h has the layout), and views of its
    columns -- kind (int32: KIND_NONE / _MISS / _EMISSIVE / _LIMIT / _SHADED), length, flags (int32: 1 has_shadow_ray, 2
    has_next_ray, 4 the light pdf is there), light_pdf, lo, cosine, direct (unshadowed), pdf, f, is_delta."""

    def __init__(self, records):
        import torch
        self.records = records
        self.kind = records[:, 0].view(torch.int32)
        self.length = records[:, 1].view(torch.int32)
        self.flags = records[:, 2].view(torch.int32)
        self.light_pdf = records[:, 3]
        self.lo = records[:, 4:7]
        self.cosine = records[:, 7]
        self.direct = records[:, 8:11]
        self.pdf = records[:, 11]
        self.f = records[:, 12:15]
        self.is_delta = records[:, 15]

    @property
    def has_shadow_ray(self):
        return (self.flags & 1) != 0

    @property
    def has_next_ray(self):
        return (self.flags & 2) != 0

    def __len__(self):
        return int(self.records.shape[0])


class Shader(_SceneQuery):
    """Shader(scene, sampler, max_path_length): one vertex of PathIntegrator's radiance() for N paths at a time, on contiguous
    CUDA torch tensors of the caller's -- on their device and the current stream, nothing copied and nothing waited for.  With an
    Accel: begin -> intersect -> vertex -> hit -> intersect -> vertex ... -> fold -> resolve (WavefrontPathIntegrator is that
    loop).  A pixel's samples are rendered in order: its RNG travels in the states.  A tensor of the wrong dtype, shape, device
    or layout raises ValueError before anything is launched.  A snapshot of the scene at creation; a context manager."""
    _NAME, _DESTROY = "Shader", lib.pine_gpu_shader_destroy

    def __init__(self, scene, sampler, max_path_length, device=0, flags=0):
        self._h = None
        self.device = int(device)
        prm = _lib.RenderParams(int(sampler.requested), int(max_path_length), self.device, 0, 1, 0, int(flags), getattr(sampler, "kind", 0))
        h = lib.pine_gpu_shader_create(scene._h, C.byref(prm))
        if not h:
            raise PineError("Shader: " + _lib.last_error())
        self._h = C.c_void_p(h)
        info = (C.c_int32 * 8)()
        check(lib.pine_gpu_shader_info(self._h, info), "Shader")
        self.film_size, self.spp, self.max_path_length = (int(info[0]), int(info[1])), int(info[2]), int(info[3])
        self.variant, self.kernel_features, self.lds_bytes = int(info[4]), int(info[5]) & 0xFFFFFFFF, int(info[6])

    def _stream(self, t):
        import torch
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def _new(self, shape, like=None, dtype=None):
        import torch
        return torch.empty(shape, dtype=dtype or torch.float32, device=like.device if like is not None else torch.device("cuda", self.device))

    def begin(self, sample, states=None, rays=None):
        """Sample `sample` of every pixel starts: -> (states (W*H, 8) int32, rays (W*H, 8) float32), new tensors or the ones
        given.  A sample after the first needs the states sample - 1 left."""
        import torch
        n = self.film_size[0] * self.film_size[1]
        if n == 0:
            raise PineError("Shader.begin: scene has no camera")
        if states is None:
            if int(sample) != 0:
                raise ValueError("Shader.begin: a sample after the first goes on from the states of the sample before")
            states = self._new((n, SHADER_STATE_WORDS), dtype=torch.int32)
        _check_tensor(states, "Shader: the states", torch.int32, (n, SHADER_STATE_WORDS), self.device)
        if rays is None:
            rays = self._new((n, 8), states)
        _check_tensor(rays, "Shader: the rays", torch.float32, (n, 8), self.device)
        check(lib.pine_gpu_shader_begin_device(self._handle(), int(sample), C.c_void_p(states.data_ptr()), C.c_void_p(rays.data_ptr()), self._stream(states)),
              "Shader.begin")
        return states, rays

    def vertex(self, rays, hits, states, records=None, shadow_rays=None, next_rays=None):
        """One radiance() invocation per path: rays (N, 8), hits (an AccelHits or its (N, 12) records) and states (N, 8) in;
        -> (ShaderRecords, shadow_rays (N, 8), next_rays (N, 8)), new tensors or the ones given.  The states advance in place."""
        import torch
        hits = getattr(hits, "records", hits)
        _check_tensor(rays, "Shader: the rays", torch.float32, (None, 8), self.device)
        n = int(rays.shape[0])
        _check_tensor(hits, "Shader: the hit records", torch.float32, (n, 12), self.device)
        _check_tensor(states, "Shader: the states", torch.int32, (n, SHADER_STATE_WORDS), self.device)
        records = getattr(records, "records", records)
        if records is None:
            records = self._new((n, SHADER_RECORD_WORDS), rays)
        if shadow_rays is None:
            shadow_rays = self._new((n, 8), rays)
        if next_rays is None:
            next_rays = self._new((n, 8), rays)
        _check_tensor(records, "Shader: the vertex records", torch.float32, (n, SHADER_RECORD_WORDS), self.device)
        _check_tensor(shadow_rays, "Shader: the shadow rays", torch.float32, (n, 8), self.device)
        _check_tensor(next_rays, "Shader: the next rays", torch.float32, (n, 8), self.device)
        if next_rays.data_ptr() == rays.data_ptr() and n:
            raise ValueError("Shader: the next rays must not be written over the rays")
        check(lib.pine_gpu_shader_vertex_device(self._handle(), C.c_void_p(rays.data_ptr()), C.c_void_p(hits.data_ptr()), n, C.c_void_p(states.data_ptr()),
                                                C.c_void_p(records.data_ptr()), C.c_void_p(shadow_rays.data_ptr()), C.c_void_p(next_rays.data_ptr()),
                                                self._stream(rays)), "Shader.vertex")
        return ShaderRecords(records), shadow_rays, next_rays

    def fold(self, records, occluded, sample, sum, log=None):
        """The backward fold of one sample: records (levels, N, 16) float32 and occluded (levels, N) uint8 (Accel.hit's answers
        for the shadow rays), level-major; path i adds its radiance to sum[i] ((N, 4) float32: xyz the running sum, w the sample
        count; sample 0 overwrites).  log: None, or a (levels, N, 16) float32 tensor for the per-vertex terms.  -> sum."""
        import torch
        _check_tensor(records, "Shader: the vertex records", torch.float32, (None, None, SHADER_RECORD_WORDS), self.device)
        levels, n = int(records.shape[0]), int(records.shape[1])
        _check_tensor(occluded, "Shader: the occlusion bytes", torch.uint8, (levels, n), self.device)
        _check_tensor(sum, "Shader: the sums", torch.float32, (n, 4), self.device)
        if log is not None:
            _check_tensor(log, "Shader: the log", torch.float32, (levels, n, SHADER_LOG_FLOATS), self.device)
        check(lib.pine_gpu_shader_fold_device(self._handle(), C.c_void_p(records.data_ptr()), C.c_void_p(occluded.data_ptr()), levels, n, int(sample),
                                              C.c_void_p(sum.data_ptr()), C.c_void_p(log.data_ptr() if log is not None else 0), self._stream(records)),
              "Shader.fold")
        return sum

    def resolve(self, sum, film=None):
        """film[i] = (sum[i].xyz / spp, 1): -> film, an (N, 4) float32 tensor (a new one, or the one given)."""
        import torch
        _check_tensor(sum, "Shader: the sums", torch.float32, (None, 4), self.device)
        n = int(sum.shape[0])
        if film is None:
            film = self._new((n, 4), sum)
        _check_tensor(film, "Shader: the film", torch.float32, (n, 4), self.device)
        check(lib.pine_gpu_shader_resolve_device(self._handle(), C.c_void_p(sum.data_ptr()), n, C.c_void_p(film.data_ptr()), self._stream(sum)),
              "Shader.resolve")
        return film


class WavefrontPathIntegrator:
    """PathIntegrator's film, bit for bit, from a loop written in Python over Accel's and Shader's batched calls: every level
    of every sample is an intersect, a vertex and a hit over all W * H paths (no compaction: a finished path costs a null ray).
    on_vertex(level, rays, hits, records) sees every level's tensors (valid during the call, on the current stream) -- AOVs,
    light baking, path filters.  Several times slower than PathIntegrator (profiles/shade_speed.txt): every vertex goes
    through device memory."""

    def __init__(self, sampler, max_path_length, order="pine", device=0):
        if max_path_length <= 0:  # path.cpp:12-13
            raise PineError(f"`PathIntegrator` expect `max_path_length` to be positive, get {max_path_length}")
        self.sampler, self.max_path_length, self.order, self.device = sampler, int(max_path_length), order, int(device)
        self.vertex_log = None

    def render(self, scene, on_vertex=None, vertex_log=False):
        """-> the scene's Film, its `pixels` the (H, W, 4) float32 film.  vertex_log: keep the fold's log of every sample in
        self.vertex_log, an (H, W, spp, max_path_length, 16) array -- the layout of pine_gpu_plan_vertex_log."""
        import torch
        if scene.camera is None:
            raise PineError("scene has no camera")
        film = scene.camera.film()
        with Accel(scene, order=self.order, device=self.device) as accel, Shader(scene, self.sampler, self.max_path_length, self.device) as shader:
            (w, h), depth, dev = shader.film_size, shader.max_path_length, torch.device("cuda", self.device)
            n = w * h
            records = torch.empty((depth, n, SHADER_RECORD_WORDS), dtype=torch.float32, device=dev)
            occluded = torch.empty((depth, n), dtype=torch.uint8, device=dev)
            hits = torch.empty((n, 12), dtype=torch.float32, device=dev)
            rays, shadow_rays, next_rays = (torch.empty((n, 8), dtype=torch.float32, device=dev) for _ in range(3))
            states = torch.empty((n, SHADER_STATE_WORDS), dtype=torch.int32, device=dev)
            sums = torch.empty((n, 4), dtype=torch.float32, device=dev)
            logs = torch.empty((shader.spp, depth, n, SHADER_LOG_FLOATS), dtype=torch.float32, device=dev) if vertex_log else None
            for s in range(shader.spp):
                shader.begin(s, states, rays)
                for level in range(depth):
                    found = accel.intersect(rays, out=hits)
                    rec, _, _ = shader.vertex(rays, found, states, records[level], shadow_rays, next_rays)
                    accel.hit(shadow_rays, out=occluded[level])
                    if on_vertex is not None:
                        on_vertex(level, rays, found, rec)
                    rays, next_rays = next_rays, rays
                shader.fold(records, occluded, s, sums, logs[s] if vertex_log else None)
            pixels = shader.resolve(sums).cpu().numpy()  # (waits for the stream)
            if vertex_log:
                self.vertex_log = np.ascontiguousarray(logs.cpu().numpy().reshape(shader.spp, depth, h, w, SHADER_LOG_FLOATS).transpose(2, 3, 0, 1, 4))
        film.pixels = pixels.reshape(h, w, 4)
        return film
