// tools/ref_atmosphere_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_atmosphere.py; no test runs it).
//
// Our own driver around the REAL reference's Atmosphere light and atmosphere_color.  It is compiled where the reference's
// sources lie and linked with oracle/_ref/libpine_ref.a; the binary goes to a scratch directory.  Only the reference's public
// API is called: atmosphere_color (color.h), Atmosphere's constructor, color, sample and pdf (light.h), Distribution2D
// (distribution.h), and for films the scene built from a .pscene exactly as oracle/ref_driver.cpp builds it (that file -- this
// repository's own -- is included for its loader; the generator takes the `envlight atmosphere` line out before it gets there).
//
//   LIGHT = <sun.x> <sun.y> <sun.z> <color.x> <color.y> <color.z> <w> <h>                        (floats as hexfloat text)
//   ref_atmosphere_driver color   <queries.bin> <out.f32>
//       per query of 7 floats (direction, sun direction, flag) 3 floats: atmosphere_color(direction, sun, 8, flag != 0)
//   ref_atmosphere_driver density LIGHT <out.f32>
//       the density Atmosphere's constructor computes (light.cpp:97-103), w * h floats in for_2d order
//   ref_atmosphere_driver tree    LIGHT <out.stream>
//       Distribution2D(density, 15) in pre-order, 7 words per node: weight bits, split_x, lower, upper, leaf
//   ref_atmosphere_driver calls   LIGHT <queries.bin> <out.records>
//       per query of 5 floats (u2, wo) 13 floats: ds.p, sample's pdf, wo, le, color(wo), pdf(wo); ds.p from a Distribution2D built
//       from the same density as Atmosphere builds its own (its own is private)
//   ref_atmosphere_driver search  LIGHT <count> <out.f32>
//       hashed u2 number 0 .. count - 1: those whose ds.p.x == w or ds.p.y == h, at most 8, 2 floats each
//   ref_atmosphere_driver film    LIGHT <scene.pscene> <spp> <blue|sobol> <depth> <out.film> <out.miss>
//       PathIntegrator(BVH(), sampler, UniformLightSampler(), depth).render; out.film raw vec4, W * H * 16 bytes; out.miss one
//       byte per pixel: 1 where the camera ray through the pixel's centre (lens sample 0.5, 0.5) meets nothing
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/color.h>
#include <pine/core/distribution.h>
#include <pine/core/light.h>
#include <pine/core/sampling.h>

struct SkyArgs {
  vec3 sun, color;
  int w, h;
};
static SkyArgs load_light_args(char** a) {
  SkyArgs s;
  s.sun = vec3(strtof(a[0], nullptr), strtof(a[1], nullptr), strtof(a[2], nullptr));
  s.color = vec3(strtof(a[3], nullptr), strtof(a[4], nullptr), strtof(a[5], nullptr));
  s.w = atoi(a[6]), s.h = atoi(a[7]);
  return s;
}

// The density of every texel as Atmosphere computes it for its private Distribution2D: the length of atmosphere_color, sun
// disc included, at the texel's direction -- texel / size through uniform_sphere, y and z exchanged.
static Array2d<float> density_of(const SkyArgs& S) {
  const vec3 sun = normalize(S.sun);
  Array2d<float> density(vec2i(S.w, S.h));
  for (int y = 0; y < S.h; y++)
    for (int x = 0; x < S.w; x++) {
      const vec3 d = uniform_sphere(vec2(float(x), float(y)) / vec2(float(S.w), float(S.h)));
      density[vec2i(x, y)] = length(atmosphere_color(vec3(d.x, d.z, d.y), sun, 8, true));
    }
  return density;
}

static void tree_stream(const Distribution2D::Node* n, std::vector<uint32_t>& out) {
  uint32_t wb;
  memcpy(&wb, &n->weight, 4);
  out.push_back(wb), out.push_back(n->split_x ? 1u : 0u);
  out.push_back(uint32_t(n->lower.x)), out.push_back(uint32_t(n->lower.y)), out.push_back(uint32_t(n->upper.x)), out.push_back(uint32_t(n->upper.y));
  out.push_back(n->left ? 0u : 1u);
  if (n->left) tree_stream(n->left.get(), out), tree_stream(n->right.get(), out);
}

static uint32_t hash32(uint32_t x) {
  x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
  return x;
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "color" && argc == 4) {
    const std::vector<float> q = read_floats(argv[2]);
    const size_t n = q.size() / 7;
    std::vector<float> out(n * 3);
    for (size_t i = 0; i < n; i++) {
      const float* a = &q[i * 7];
      const vec3 c = atmosphere_color(vec3(a[0], a[1], a[2]), vec3(a[3], a[4], a[5]), 8, a[6] != 0.0f);
      out[i * 3] = c.x, out[i * 3 + 1] = c.y, out[i * 3 + 2] = c.z;
    }
    write_file(argv[3], out.data(), out.size() * 4);
    return 0;
  }
  if (argc < 10) return fprintf(stderr, "usage: see the head of tools/ref_atmosphere_driver.cpp\n"), 2;
  const SkyArgs S = load_light_args(argv + 2);
  char** rest = argv + 10;
  const int nrest = argc - 10;
  if (cmd == "density" && nrest == 1) {
    const auto density = density_of(S);
    std::vector<float> out;
    for_2d(vec2i(S.w, S.h), [&](vec2i p) { out.push_back(density[p]); });
    write_file(rest[0], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "tree" && nrest == 1) {
    const auto distr = Distribution2D(density_of(S), 15);
    std::vector<uint32_t> out;
    tree_stream(distr.root.get(), out);
    write_file(rest[0], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "search" && nrest == 2) {
    const auto distr = Distribution2D(density_of(S), 15);
    const uint32_t count = uint32_t(strtoul(rest[0], nullptr, 10));
    std::vector<float> out;
    for (uint32_t i = 0; i < count && out.size() < 16; i++) {
      const vec2 u2(float(hash32(2 * i + 1) >> 8) / float(1 << 24), float(hash32(2 * i + 2) >> 8) / float(1 << 24));
      const auto ds = distr.sample(u2);
      if (ds.p.x == S.w || ds.p.y == S.h) out.push_back(u2.x), out.push_back(u2.y);
    }
    write_file(rest[1], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "calls" && nrest == 2) {
    const auto sky = Atmosphere(S.sun, S.color, vec2i(S.w, S.h));
    const auto distr = Distribution2D(density_of(S), 15);
    const std::vector<float> q = read_floats(rest[0]);
    const size_t n = q.size() / 5;
    std::vector<float> out(n * 13, 0.0f);
    for (size_t i = 0; i < n; i++) {
      float* o = &out[i * 13];
      const vec2 u2(q[i * 5], q[i * 5 + 1]);
      const auto ds = distr.sample(u2);
      o[0] = float(ds.p.x), o[1] = float(ds.p.y);
      const auto ls = sky.sample(vec3(0), u2);
      o[2] = ls->pdf;
      o[3] = ls->wo.x, o[4] = ls->wo.y, o[5] = ls->wo.z;
      o[6] = ls->le.x, o[7] = ls->le.y, o[8] = ls->le.z;
      if (ls->distance != float_max) return fprintf(stderr, "sample(): distance is not float_max\n"), 3;
      const vec3 wo(q[i * 5 + 2], q[i * 5 + 3], q[i * 5 + 4]);
      const vec3 c = sky.color(wo);
      o[9] = c.x, o[10] = c.y, o[11] = c.z;
      o[12] = sky.pdf(wo);
    }
    write_file(rest[1], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "film" && nrest == 6) {
    Loaded L;
    load_pscene(rest[0], L);
    L.scene.set_env_light(EnvironmentLight(Atmosphere(S.sun, S.color, vec2i(S.w, S.h))));
    const int spp = atoi(rest[1]), depth = atoi(rest[3]);
    const bool sobol = std::string(rest[2]) == "sobol";
    auto integ = PathIntegrator(Accel(BVH()), sobol ? Sampler(SobolSampler(spp)) : Sampler(BlueSobolSampler(spp)), UniformLightSampler(), depth);
    integ.render(L.scene);
    auto& film = L.scene.camera.film();
    write_file(rest[4], film.data(), size_t(16) * L.W * L.H);
    Accel accel = Accel(BVH());
    accel.build(&L.scene);
    std::vector<unsigned char> miss(size_t(L.W) * L.H);
    for (int y = 0; y < L.H; y++)
      for (int x = 0; x < L.W; x++) {
        const Ray ray = L.scene.camera.gen_ray((vec2(x, y) + vec2(0.5f)) / film.size(), vec2(0.5f));
        miss[size_t(y) * L.W + x] = accel.hit(ray) ? 0 : 1;
      }
    write_file(rest[5], miss.data(), miss.size());
    return 0;
  }
  return fprintf(stderr, "usage: see the head of tools/ref_atmosphere_driver.cpp\n"), 2;
}
