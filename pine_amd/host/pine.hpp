// pine_amd/host/pine.hpp -- C++ host facade over the C ABI (include/pine_gpu.h).
//
// Keeps the names a pine user writes (src/pine/core/program_context.cpp:23-125 and the *_context
// functions): Scene / add / set, Diffuse, Emissive, Uber, Subsurface, Rect, Box, Sphere, Disk, Cone,
// Mesh, Film, Uncharted2, ThinLenCamera, BlueSampler, PathIntegrator(sampler, depth).render(scene), AOIntegrator(sampler).render(scene),
// scene.camera.film().save(...).  Header-only; link with -lpine_gpu.  Errors throw pine::Error where
// the reference would SEVERE()/abort (src/pine/core/log.h:45-51).
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pine_gpu.h"
#include "gltf_import.hpp"
#include "hdr_read.hpp"
#include "png_read.hpp"

namespace pine {

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};
inline int check(int rc, const char* what) {
  if (rc < 0) throw Error(std::string(what) + ": " + pine_gpu_last_error());
  return rc;
}

struct vec3 {
  float x = 0, y = 0, z = 0;
  vec3() = default;
  vec3(float x, float y, float z) : x(x), y(y), z(z) {}
  const float* data() const { return &x; }
};
inline vec3 operator*(float s, vec3 v) { return {s * v.x, s * v.y, s * v.z}; }
struct vec2i {
  int x = 0, y = 0;
};

struct mat4 {  // storage order of the reference: m[c*4 + r]
  float m[16];
  mat4() { pine_gpu_mat4_identity(m); }
  friend mat4 operator*(const mat4& a, const mat4& b) {
    mat4 r;
    pine_gpu_mat4_mul(a.m, b.m, r.m);
    return r;
  }
};
inline mat4 translate(vec3 v) { mat4 r; pine_gpu_mat4_translate(v.data(), r.m); return r; }
inline mat4 scale(vec3 v) { mat4 r; pine_gpu_mat4_scale(v.data(), r.m); return r; }
inline mat4 rotate_x(float a) { mat4 r; pine_gpu_mat4_rotate_x(a, r.m); return r; }
inline mat4 rotate_y(float a) { mat4 r; pine_gpu_mat4_rotate_y(a, r.m); return r; }
inline mat4 rotate_z(float a) { mat4 r; pine_gpu_mat4_rotate_z(a, r.m); return r; }
inline mat4 inverse(const mat4& a) { mat4 r; pine_gpu_mat4_inverse(a.m, r.m); return r; }
inline mat4 look_at(vec3 from, vec3 to) { mat4 r; pine_gpu_mat4_look_at(from.data(), to.data(), r.m); return r; }

// ---- materials ----
struct Emissive { vec3 color; };
struct Diffuse { vec3 albedo; };
struct Uber { vec3 albedo; float roughness; float metallic = 0.0f; float transmission = 0.0f; float ior = 1.45f; };
struct Subsurface { vec3 albedo; float roughness; vec3 sigma_s; };
// constant-parameter forms of material.h:39-78 (node-graph parameters: use the C ABI's node calls)
struct Metal { vec3 albedo; float roughness; };
struct Glossy { vec3 albedo; float roughness; float ior = 1.4f; };
struct Glass { vec3 albedo; float roughness; float ior = 1.4f; };

// ---- lights other than emissive geometry (light.h:21-67) ----
struct PointLight { vec3 position, color; };
struct SpotLight { vec3 position, direction, color; float falloff_radian, cutoff_additional_radian = 0.0f; };
struct DirectionalLight { vec3 direction, color; };
struct Sky { vec3 sun_color; };

// ---- shapes ----
struct Rect { vec3 position, ex, ey; bool flip_normal = false; };
struct AABB { vec3 lower, upper; };
struct OBB { AABB base; mat4 m; };
inline AABB Box(vec3 lower, vec3 upper) { return {lower, upper}; }
inline OBB Box(AABB aabb, mat4 m) { return {aabb, m}; }
struct Sphere { vec3 center; float radius; };
struct Disk { vec3 position, normal; float radius; };
struct Cone { vec3 position, normal; float radius, height; };
struct Plane { vec3 position, normal; };
struct Line { vec3 p0, p1; float thickness; };
struct Cylinder { vec3 p0, p1; float radius; };
struct Triangle { vec3 v0, v1, v2; };
struct Mesh { std::vector<vec3> vertices; std::vector<std::array<uint32_t, 3>> indices; };

template <class T> struct is_shape : std::false_type {};
template <> struct is_shape<Rect> : std::true_type {};
template <> struct is_shape<AABB> : std::true_type {};
template <> struct is_shape<OBB> : std::true_type {};
template <> struct is_shape<Sphere> : std::true_type {};
template <> struct is_shape<Disk> : std::true_type {};
template <> struct is_shape<Cone> : std::true_type {};
template <> struct is_shape<Plane> : std::true_type {};
template <> struct is_shape<Line> : std::true_type {};
template <> struct is_shape<Cylinder> : std::true_type {};
template <> struct is_shape<Triangle> : std::true_type {};
template <> struct is_shape<Mesh> : std::true_type {};

struct Uncharted2 { static constexpr int code = 0; };
struct ACES { static constexpr int code = 1; };

struct Film {
  vec2i size_;
  int tone_mapper = 0;
  std::vector<float> pixels;  // W*H*4, row 0 first (Array2d<vec4>)
  Film() = default;
  Film(vec2i size, Uncharted2 = {}) : size_(size), tone_mapper(0), pixels(size_t(size.x) * size.y * 4, 0.0f) {}
  Film(vec2i size, ACES) : size_(size), tone_mapper(1), pixels(size_t(size.x) * size.y * 4, 0.0f) {}
  vec2i size() const { return size_; }
  // tone-mapped, gamma 2.2, y-flipped RGBA8 exactly as save() produces it
  std::vector<uint8_t> finalize_u8() const {
    std::vector<uint8_t> out(size_t(size_.x) * size_.y * 4);
    check(pine_gpu_film_finalize_u8(pixels.data(), size_.x, size_.y, tone_mapper, out.data()), "film.finalize");
    return out;
  }
  void save_raw(const std::string& path) const;  // raw float32 dump (PNG encoding lives in the Python layer)
};

struct ThinLenCamera {
  Film film_;
  vec3 from, to;
  float fov, len_radius = 0.0f, focus_distance = 1.0f;
  ThinLenCamera() = default;
  ThinLenCamera(Film film, vec3 from, vec3 to, float fov, float len_radius = 0.0f, float focus_distance = 1.0f)
      : film_(std::move(film)), from(from), to(to), fov(fov), len_radius(len_radius), focus_distance(focus_distance) {}
  Film& film() { return film_; }
};

struct BlueSampler {  // sampler.h:166-201
  int requested;
  explicit BlueSampler(int spp) : requested(spp) {
    if (spp <= 0) throw Error("`BlueSampler` should have positive samples per pixel");
  }
};
struct SobolSampler {  // sampler.h:83-164: spp as given (on the device any count up to 4096)
  int requested;
  explicit SobolSampler(int spp) : requested(spp) {}
};
struct HaltonSampler {  // sampler.h:40-81: spp as given (on the device any count up to 4096)
  int requested;
  explicit HaltonSampler(int spp) : requested(spp) {
    if (spp <= 0) throw Error("`HaltonSampler` should have positive samples per pixel");
  }
};
struct Sampler {  // the variant PathIntegrator takes (sampler.h:275-; UniformSampler is not reproducible)
  int requested, kind;
  Sampler(BlueSampler s) : requested(s.requested), kind(PINE_GPU_SAMPLER_BLUE) {}
  Sampler(SobolSampler s) : requested(s.requested), kind(PINE_GPU_SAMPLER_SOBOL) {}
  Sampler(HaltonSampler s) : requested(s.requested), kind(PINE_GPU_SAMPLER_HALTON) {}
};

// An image as ImageSky takes it (image.h:11-30): float texels (a Radiance HDR file, or an array), or 8-bit texels (a PNG file
// expanded to 3 channels as the reference's image_from loads it -- png_read.hpp -- or an array) that the library converts as
// the reference's vec3u8 images are read (pow(value / 255, 2.2)).  Rows top first, 3 values per texel.
struct Image {
  vec2i size;
  std::vector<float> rgb;
  std::vector<uint8_t> u8;
  Image(vec2i size, std::vector<float> texels) : size(size), rgb(std::move(texels)) { expect(rgb.size()); }
  Image(vec2i size, std::vector<uint8_t> texels) : size(size), u8(std::move(texels)) { expect(u8.size()); }
  explicit Image(vec3 color) : size{1, 1}, rgb{color.x, color.y, color.z} {}  // ImagePtr(vec3): the reference's 1 x 1 image
  explicit Image(const std::string& file) {  // a Radiance .hdr or a .png file, told apart by the file's first bytes
    try {
      unsigned char head[4] = {0, 0, 0, 0};
      if (FILE* f = fopen(file.c_str(), "rb")) {
        if (fread(head, 1, 4, f) != 4) head[0] = 0;
        fclose(f);
      }
      if (head[0] == 0x89 && head[1] == 'P' && head[2] == 'N' && head[3] == 'G') {
        PngImage p = read_png(file, 3);
        size = vec2i{p.w, p.h};
        u8 = std::move(p.texels);
        return;
      }
      HdrImage f = read_hdr(file);
      size = vec2i{f.w, f.h};
      rgb = std::move(f.rgb);
    } catch (const std::runtime_error& e) {
      throw Error(e.what());
    }
  }

 private:
  void expect(size_t values) const {
    if (size.x < 0 || size.y < 0 || values != size_t(size.x) * size_t(size.y) * 3) throw Error("Image: size and texel count disagree");
  }
};
using ImagePtr = std::shared_ptr<Image>;
struct ImageSky {  // light.h:81-94
  ImagePtr image;
  vec3 tint{1, 1, 1};
  float elevation = 0.0f, rotation = 0.0f;
  ImageSky(ImagePtr image, vec3 tint = vec3{1, 1, 1}, float elevation = 0.0f, float rotation = 0.0f)
      : image(std::move(image)), tint(tint), elevation(elevation), rotation(rotation) {
    if (!this->image) throw Error("ImageSky: no image");
  }
};
struct Atmosphere {  // light.h:69-79; image_size: the grid of its importance sampling (the reference's scripts always get 1024 x 1024)
  vec3 sun_direction, sun_color;
  vec2i image_size{1024, 1024};
  int device = -1;  // the HIP device that computes the light's tables when it is set; -1: host threads (the same bytes)
  Atmosphere(vec3 sun_direction, vec3 sun_color, vec2i image_size = vec2i{1024, 1024}, int device = -1)
      : sun_direction(sun_direction), sun_color(sun_color), image_size(image_size), device(device) {}
};

class Scene {
 public:
  Scene() : h_(pine_gpu_scene_create()) {}
  ~Scene() { pine_gpu_scene_destroy(h_); }
  Scene(const Scene&) = delete;
  Scene& operator=(const Scene&) = delete;

  int add(const std::string& name, Emissive m) { return check(pine_gpu_scene_add_material_emissive(h_, name.c_str(), m.color.data()), "Emissive"); }
  int add(const std::string& name, Diffuse m) { return check(pine_gpu_scene_add_material_diffuse(h_, name.c_str(), m.albedo.data()), "Diffuse"); }
  int add(const std::string& name, Uber m) {
    return check(pine_gpu_scene_add_material_uber(h_, name.c_str(), m.albedo.data(), m.roughness, m.metallic, m.transmission, m.ior), "Uber");
  }
  int add(const std::string& name, Subsurface m) {
    return check(pine_gpu_scene_add_material_subsurface(h_, name.c_str(), m.albedo.data(), m.roughness, m.sigma_s.data()), "Subsurface");
  }
  int add(const std::string& name, Metal m) {
    return check(pine_gpu_scene_add_material_metal(h_, name.c_str(), node(m.albedo), node(m.roughness)), "Metal");
  }
  int add(const std::string& name, Glossy m) {
    return check(pine_gpu_scene_add_material_glossy(h_, name.c_str(), node(m.albedo), node(m.roughness), node(m.ior)), "Glossy");
  }
  int add(const std::string& name, Glass m) {
    return check(pine_gpu_scene_add_material_glass(h_, name.c_str(), node(m.albedo), node(m.roughness), node(m.ior)), "Glass");
  }
  int add(PointLight l) { return check(pine_gpu_scene_add_light_point(h_, l.position.data(), l.color.data()), "PointLight"); }
  int add(SpotLight l) {
    return check(pine_gpu_scene_add_light_spot(h_, l.position.data(), l.direction.data(), l.color.data(), l.falloff_radian,
                                               l.cutoff_additional_radian), "SpotLight");
  }
  int add(DirectionalLight l) { return check(pine_gpu_scene_add_light_directional(h_, l.direction.data(), l.color.data()), "DirectionalLight"); }
  void set(Sky sky) { check(pine_gpu_scene_set_env_sky(h_, sky.sun_color.data()), "scene.set(Sky)"); }
  // the scene as .pscene text (the exchange format of the tests and the reference driver)
  std::string describe() const {
    const long long n = pine_gpu_scene_describe(h_, nullptr, 0);
    if (n < 0) throw Error(std::string("describe: ") + pine_gpu_last_error());
    std::string text(size_t(n) + 1, '\0');
    pine_gpu_scene_describe(h_, &text[0], n + 1);
    text.resize(size_t(n));
    return text;
  }
  void set(const Atmosphere& sky) {
    check(pine_gpu_scene_set_env_atmosphere(h_, sky.sun_direction.data(), sky.sun_color.data(), sky.image_size.x, sky.image_size.y, sky.device),
          "scene.set(Atmosphere)");
  }
  void set(const ImageSky& sky) {
    const Image& im = *sky.image;
    if (!im.u8.empty())
      check(pine_gpu_scene_set_env_image_u8(h_, im.u8.data(), im.size.x, im.size.y, sky.tint.data(), sky.elevation, sky.rotation), "scene.set(ImageSky)");
    else
      check(pine_gpu_scene_set_env_image(h_, im.rgb.data(), im.size.x, im.size.y, sky.tint.data(), sky.elevation, sky.rotation), "scene.set(ImageSky)");
  }
  // scene.add(shape, "material name") and scene.add(shape, Material)
  template <class S, class = std::enable_if_t<is_shape<S>::value>>
  int add(const S& shape, const std::string& material) {
    return add_shape(shape, check(pine_gpu_scene_find_material(h_, material.c_str()), "scene.add"));
  }
  template <class S, class M, class = std::enable_if_t<is_shape<S>::value && !std::is_convertible<M, std::string>::value>>
  int add(const S& shape, M material) {
    return add_shape(shape, add(std::string(), material));
  }
  ThinLenCamera& set(ThinLenCamera cam) {
    camera = std::move(cam);
    check(pine_gpu_scene_set_camera_thinlens(h_, camera.film_.size_.x, camera.film_.size_.y, camera.film_.tone_mapper,
                                             camera.from.data(), camera.to.data(), camera.fov, camera.len_radius,
                                             camera.focus_distance), "scene.set");
    return camera;
  }
  pine_gpu_scene* handle() const { return h_; }
  ThinLenCamera camera;

 private:
  int add_shape(const Rect& s, int m) { return check(pine_gpu_scene_add_rect(h_, s.position.data(), s.ex.data(), s.ey.data(), s.flip_normal, m), "Rect"); }
  int add_shape(const AABB& s, int m) { return check(pine_gpu_scene_add_aabb(h_, s.lower.data(), s.upper.data(), m), "Box"); }
  int add_shape(const OBB& s, int m) { return check(pine_gpu_scene_add_obb(h_, s.base.lower.data(), s.base.upper.data(), s.m.m, m), "Box"); }
  int add_shape(const Sphere& s, int m) { return check(pine_gpu_scene_add_sphere(h_, s.center.data(), s.radius, m), "Sphere"); }
  int add_shape(const Disk& s, int m) { return check(pine_gpu_scene_add_disk(h_, s.position.data(), s.normal.data(), s.radius, m), "Disk"); }
  int add_shape(const Cone& s, int m) { return check(pine_gpu_scene_add_cone(h_, s.position.data(), s.normal.data(), s.radius, s.height, m), "Cone"); }
  int add_shape(const Plane& s, int m) { return check(pine_gpu_scene_add_plane(h_, s.position.data(), s.normal.data(), m), "Plane"); }
  int add_shape(const Line& s, int m) { return check(pine_gpu_scene_add_line(h_, s.p0.data(), s.p1.data(), s.thickness, m), "Line"); }
  int add_shape(const Cylinder& s, int m) { return check(pine_gpu_scene_add_cylinder(h_, s.p0.data(), s.p1.data(), s.radius, m), "Cylinder"); }
  int add_shape(const Triangle& s, int m) { return check(pine_gpu_scene_add_triangle(h_, s.v0.data(), s.v1.data(), s.v2.data(), m), "Triangle"); }
  int add_shape(const Mesh& s, int m) {
    return check(pine_gpu_scene_add_mesh(h_, &s.vertices[0].x, int(s.vertices.size()), &s.indices[0][0], int(s.indices.size()), m), "Mesh");
  }
  int node(vec3 v) { return check(pine_gpu_scene_node_const3(h_, v.data()), "node"); }
  int node(float v) { return check(pine_gpu_scene_node_constf(h_, v), "node"); }
  pine_gpu_scene* h_;
};

class PathIntegrator {
 public:
  PathIntegrator(Sampler sampler, int max_path_length, int device = 0)
      : sampler_(sampler), max_path_length_(max_path_length), device_(device) {
    if (max_path_length <= 0) throw Error("`PathIntegrator` expect `max_path_length` to be positive");
  }
  // render on several devices of the node from this one process (tiles dealt round-robin, slabs gathered with peer copies)
  PathIntegrator& on_devices(std::vector<int> devices) {
    devices_ = std::move(devices);
    return *this;
  }
  // The scene's own path kernel (same film; pine_gpu.h): by default the library uses it when it is in its cache and compiles it
  // in the background otherwise.  specialize(true): wait for the compiler at render() and fail if the kernel cannot be built
  // (PINE_GPU_FLAG_SPECIALIZE); specialize(false): precompiled kernels only (PINE_GPU_FLAG_NO_SPECIALIZE).
  // closest hits in the order of the reference's default accel, EmbreeAccel (PINE_GPU_FLAG_ORDER_EMBREE), instead of pine-BVH
  // order (the default: Accel(BVH())); only scenes with order-dependent shapes -- a scaled Box(AABB, mat4), Plane, Line,
  // Cylinder -- show the difference
  PathIntegrator& order_embree(bool on = true) {
    flags_ = on ? (flags_ | PINE_GPU_FLAG_ORDER_EMBREE) : (flags_ & ~PINE_GPU_FLAG_ORDER_EMBREE);
    return *this;
  }
  PathIntegrator& order_nearest(bool on = true) { return order_embree(on); }  // (former name)
  PathIntegrator& specialize(bool on = true) {
    flags_ &= ~(PINE_GPU_FLAG_SPECIALIZE | PINE_GPU_FLAG_NO_SPECIALIZE);
    flags_ |= on ? PINE_GPU_FLAG_SPECIALIZE : PINE_GPU_FLAG_NO_SPECIALIZE;
    return *this;
  }
  // pass_samples > 0 or on_pass: render in passes of about that many samples per pixel on one device
  // (pine_gpu_path_render_passes): the same film, bit for bit, from sample and checkpoint buffers sized for one pass;
  // on_pass(pass, pass_count, film) sees the running film after every pass and stops the render by returning non-zero --
  // render() then returns false and the film holds the last one delivered.
  bool render(Scene& scene, int pass_samples = 0, std::function<int(int, int, const float*)> on_pass = nullptr) {
    pine_gpu_render_params p{};
    p.flags = flags_;
    p.spp = sampler_.requested;
    p.max_path_length = max_path_length_;
    p.device = device_;
    p.shard_rank = 0;
    p.shard_world = 1;
    p.sampler = sampler_.kind;
    if (pass_samples > 0 || on_pass) {
      if (devices_.size() > 1) throw Error("PathIntegrator::render: passes render on one device");
      const pine_gpu_pass_callback cb = [](void* user, int pass, int count, const float* film) -> int {
        auto& fn = *static_cast<std::function<int(int, int, const float*)>*>(user);
        return fn ? fn(pass, count, film) : 0;
      };
      const int rc = pine_gpu_path_render_passes(scene.handle(), &p, pass_samples, scene.camera.film_.pixels.data(), cb, &on_pass);
      check(rc, "PathIntegrator::render");
      return rc != PINE_GPU_RENDER_STOPPED;
    }
    if (devices_.size() > 1)
      check(pine_gpu_path_render_devices(scene.handle(), &p, devices_.data(), int(devices_.size()), scene.camera.film_.pixels.data()),
            "PathIntegrator::render");
    else
      check(pine_gpu_path_render(scene.handle(), &p, scene.camera.film_.pixels.data()), "PathIntegrator::render");
    return true;
  }

 private:
  Sampler sampler_;
  int max_path_length_, device_;
  int flags_ = 0;
  std::vector<int> devices_;
};

// AOIntegrator(sampler).render(scene): ambient occlusion (src/pine/impl/integrator/ao.h, ao.cpp) -- what the reference's
// AOIntegrator(BVH(), sampler) renders, bit for bit: max(sampler.spp() / 8, 1) samples per pixel, each the fraction of eight rays
// of length min_value(scene.get_aabb().diagonal()) / 2 around the hit point that meet nothing.  Materials and lights play no
// part.  (pine-BVH order only: EmbreeAccel's hit8 is Embree's packet traversal, which is not reproduced.)
class AOIntegrator {
 public:
  explicit AOIntegrator(Sampler sampler, int device = 0) : sampler_(sampler), device_(device) {}
  void render(Scene& scene) {
    pine_gpu_render_params p{};
    p.spp = sampler_.requested;
    p.max_path_length = 1;
    p.device = device_;
    p.shard_rank = 0;
    p.shard_world = 1;
    p.sampler = sampler_.kind;
    check(pine_gpu_ao_render(scene.handle(), &p, scene.camera.film_.pixels.data()), "AOIntegrator::render");
  }

 private:
  Sampler sampler_;
  int device_;
};

// guides(scene, albedo, normal): the guide images of the reference's DenoiseIntegrator (src/pine/impl/integrator/denoiser.cpp:13-23)
// -- per pixel the albedo and the normal of the closest hit through the pixel centre, zeros on a miss -- as W*H*3 floats each, film
// row order; bit for bit the reference's with Accel = BVH().
inline void guides(Scene& scene, std::vector<float>& albedo, std::vector<float>& normal, int device = 0) {
  const vec2i size = scene.camera.film_.size();
  albedo.assign(size_t(size.x) * size.y * 3, 0.0f);
  normal.assign(size_t(size.x) * size.y * 3, 0.0f);
  pine_gpu_render_params p{};
  p.spp = 1;
  p.max_path_length = 1;
  p.device = device;
  p.shard_world = 1;
  check(pine_gpu_guides_render(scene.handle(), &p, albedo.data(), normal.data()), "guides");
}

// The filter's parameters (pine_gpu_denoise_params) with the library's defaults; device = -1: the host-thread build.
struct DenoiseParams : pine_gpu_denoise_params {
  DenoiseParams() { pine_gpu_denoise_params_default(this); }
};

// DenoiseIntegrator(params).render(scene) (denoiser.cpp:9-27): computes the guide images and denoises, in place, the film the
// scene's camera already holds.  The reference hands the three images to Open Image Denoise; the filter here is the edge-avoiding
// a-trous filter of pine_amd/csrc/pine_denoise.h.
class DenoiseIntegrator {
 public:
  explicit DenoiseIntegrator(DenoiseParams params = DenoiseParams()) : params_(params) {}
  void render(Scene& scene) {
    std::vector<float> albedo, normal;
    guides(scene, albedo, normal, params_.device < 0 ? 0 : params_.device);
    Film& film = scene.camera.film_;
    check(pine_gpu_denoise(&params_, film.size_.x, film.size_.y, film.pixels.data(), albedo.data(), normal.data(), film.pixels.data()),
          "DenoiseIntegrator::render");
  }

 private:
  DenoiseParams params_;
};

// Accel accel(scene, BVH{} | Embree{}): the scene's accel answering batches of rays (src/pine/core/accel.h:10-25) -- what
// RTIntegrator::intersect / hit hand to a CustomRayIntegrator's radiance() (core/integrator.h:31-38, :61-74).  A snapshot of
// the scene at construction.  BVH{}: Accel(BVH()); Embree{}: Accel(EmbreeAccel()), the reference's default.
struct BVH {};
struct Embree {};
struct Ray {  // ray.h:8-23; d is used as given: t is in units of d
  vec3 o, d;
  float tmin = 0.0f, tmax = 3.402823466e+38f;
};
struct Interaction {  // one hit record (include/pine_gpu.h): on a miss t is the ray's tmax as it came, the indices are -1, the rest 0
  float t;
  int32_t geometry, triangle, material;
  float p[3], n[3], uv[2];
  bool hit() const { return geometry >= 0; }
};
static_assert(sizeof(Ray) == 32 && sizeof(Interaction) == 48, "the layouts of pine_gpu_accel_intersect");
class Accel {
 public:
  Accel(Scene& scene, BVH = BVH{}, int device = 0) : h_(pine_gpu_accel_create(scene.handle(), device, 0)) { created(); }
  Accel(Scene& scene, Embree, int device = 0) : h_(pine_gpu_accel_create(scene.handle(), device, PINE_GPU_FLAG_ORDER_EMBREE)) { created(); }
  ~Accel() { pine_gpu_accel_destroy(h_); }
  Accel(const Accel&) = delete;
  Accel& operator=(const Accel&) = delete;
  // host arrays: upload, query, wait, download
  void intersect(const Ray* rays, int64_t n, Interaction* out) const {
    check(pine_gpu_accel_intersect(h_, reinterpret_cast<const float*>(rays), n, out), "Accel::intersect");
  }
  void hit(const Ray* rays, int64_t n, uint8_t* occluded) const { check(pine_gpu_accel_hit(h_, reinterpret_cast<const float*>(rays), n, occluded), "Accel::hit"); }
  // 16-byte aligned device pointers, enqueued on `stream` (a hipStream_t), nothing waited for
  void intersect_device(const void* rays_dev, int64_t n, void* hits_dev, void* stream = nullptr) const {
    check(pine_gpu_accel_intersect_device(h_, rays_dev, n, hits_dev, stream), "Accel::intersect_device");
  }
  void hit_device(const void* rays_dev, int64_t n, void* occluded_dev, void* stream = nullptr) const {
    check(pine_gpu_accel_hit_device(h_, rays_dev, n, occluded_dev, stream), "Accel::hit_device");
  }
  // W * H pixel-centre rays of the scene's camera, row-major (denoiser.cpp:13-23), to device memory
  void camera_rays_device(void* rays_dev, void* stream = nullptr) const { check(pine_gpu_accel_camera_rays_device(h_, rays_dev, stream), "Accel::camera_rays_device"); }
  pine_gpu_accel* handle() const { return h_; }

 private:
  void created() const {
    if (!h_) throw Error(std::string("Accel: ") + pine_gpu_last_error());
  }
  pine_gpu_accel* h_;
};

// Shader(scene, sampler, max_path_length): one vertex of PathIntegrator::radiance() for n paths at a time in the caller's device
// buffers (include/pine_gpu.h has the layouts of the state, the vertex record and the log).  With an Accel:
// begin -> intersect -> vertex -> hit -> intersect -> vertex -> ... -> fold -> resolve.  Every call takes 16-byte aligned device
// pointers, is enqueued on `stream` (a hipStream_t) and waits for nothing.
struct VertexRecord {
  int32_t kind, length;  // kind: -1 none, 0 miss, 1 emissive, 2 the path-length limit, 3 shaded
  uint32_t flags;        // 1 has_shadow_ray, 2 has_next_ray, 4 the light pdf is there
  float light_pdf, lo[3], cosine, direct[3], pdf, f[3], is_delta;
  bool has_shadow_ray() const { return (flags & 1u) != 0; }
  bool has_next_ray() const { return (flags & 2u) != 0; }
};
static_assert(sizeof(VertexRecord) == 64, "the layout of pine_gpu_shader_vertex_device");
class Shader {
 public:
  Shader(Scene& scene, Sampler sampler, int max_path_length, int device = 0) {
    pine_gpu_render_params p{};
    p.spp = sampler.requested;
    p.max_path_length = max_path_length;
    p.device = device;
    p.shard_rank = 0;
    p.shard_world = 1;
    p.sampler = sampler.kind;
    h_ = pine_gpu_shader_create(scene.handle(), &p);
    if (!h_) throw Error(std::string("Shader: ") + pine_gpu_last_error());
    check(pine_gpu_shader_info(h_, info_), "Shader");
  }
  ~Shader() { pine_gpu_shader_destroy(h_); }
  Shader(const Shader&) = delete;
  Shader& operator=(const Shader&) = delete;
  int film_width() const { return info_[0]; }
  int film_height() const { return info_[1]; }
  int spp() const { return info_[2]; }  // effective
  int max_path_length() const { return info_[3]; }
  static constexpr int state_bytes = 32, record_bytes = 64, ray_floats = 8, log_floats = 16;
  // sample `sample` of every pixel starts: W * H states and camera rays, row-major
  void begin_device(int sample, void* states_dev, void* rays_dev, void* stream = nullptr) const {
    check(pine_gpu_shader_begin_device(h_, sample, states_dev, rays_dev, stream), "Shader::begin_device");
  }
  void vertex_device(const void* rays_dev, const void* hits_dev, int64_t n, void* states_dev, void* records_dev, void* shadow_rays_dev,
                     void* next_rays_dev, void* stream = nullptr) const {
    check(pine_gpu_shader_vertex_device(h_, rays_dev, hits_dev, n, states_dev, records_dev, shadow_rays_dev, next_rays_dev, stream), "Shader::vertex_device");
  }
  void fold_device(const void* records_dev, const void* occluded_dev, int levels, int64_t n, int sample, void* sum_dev, void* log_dev = nullptr,
                   void* stream = nullptr) const {
    check(pine_gpu_shader_fold_device(h_, records_dev, occluded_dev, levels, n, sample, sum_dev, log_dev, stream), "Shader::fold_device");
  }
  void resolve_device(const void* sum_dev, int64_t n, void* film_dev, void* stream = nullptr) const {
    check(pine_gpu_shader_resolve_device(h_, sum_dev, n, film_dev, stream), "Shader::resolve_device");
  }
  pine_gpu_shader* handle() const { return h_; }

 private:
  pine_gpu_shader* h_ = nullptr;
  int32_t info_[8] = {};
};

inline float get_progress() { return pine_gpu_progress(); }

// load(scene, "file.glb" [, mat4]) (fileio.cpp:584-589): glTF import -- every mesh primitive with its material, and the
// camera when a node carries one (gltf_import.hpp)
inline void load(Scene& scene, const std::string& filename, const mat4& m = mat4()) {
  pine_gltf::ImportedCamera cam;
  try {
    cam = pine_gltf::import_scene(scene.handle(), filename, m.m);
  } catch (const pine_gltf::Error& e) {
    throw Error(std::string("load: ") + e.what());
  }
  if (cam.present)
    scene.set(ThinLenCamera(Film(vec2i{cam.film_w, cam.film_h}), vec3(cam.from[0], cam.from[1], cam.from[2]),
                            vec3(cam.to[0], cam.to[1], cam.to[2]), cam.fov));
}

}  // namespace pine
