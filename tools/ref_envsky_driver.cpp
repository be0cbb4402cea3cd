// tools/ref_envsky_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_envsky.py; no test runs it).
//
// Our own driver around the REAL reference's ImageSky.  It is compiled where the reference's sources lie and linked with
// oracle/_ref/libpine_ref.a; the binary goes to a scratch directory.  Only the reference's public API is called: the scene is
// built from a .pscene exactly as oracle/ref_driver.cpp builds it (that file -- this repository's own -- is included for its
// loader; the generator takes the `envlight image` line out before it gets there), the image through Array2d / Image from a raw
// texel file, the light through ImageSky's constructor and Scene::set_env_light.
//
//   IMAGE = <texels.bin> <w> <h> <f32|u8> <tint.x> <tint.y> <tint.z> <elevation> <rotation>     (floats as hexfloat text)
//   ref_envsky_driver film   IMAGE <scene.pscene> <spp> <blue|sobol> <depth> <out.film> <out.miss>
//       PathIntegrator(BVH(), sampler, UniformLightSampler(), depth).render; out.film raw vec4, W * H * 16 bytes; out.miss one
//       byte per pixel: 1 where the camera ray through the pixel's centre (lens sample 0.5, 0.5) meets nothing
//   ref_envsky_driver calls  IMAGE <queries.bin> <out.records> <out.flags>
//       per query of 5 floats (u2, wo) 13 floats: ds.p, sample's pdf, wo, le, color(wo), pdf(wo); ds.p from a Distribution2D built
//       from the same density as ImageSky builds its own.  out.flags one byte per query: 1 where the linear index of ds.p
//       (a coordinate may equal `upper`) lies outside the image's array: the reference would read outside it, so
//       ImageSky::sample is then not called and the record's words 2-8 stay zero
//   ref_envsky_driver tree   IMAGE <out.stream>
//       Distribution2D(density, 20) in pre-order, 7 words per node: weight bits, split_x, lower, upper, leaf
//   ref_envsky_driver texels IMAGE <out.f32>          Image::operator[] of every texel, 3 floats each
//   ref_envsky_driver hdr    <file.hdr> <out.bin>     image_from: width, height (int32), then operator[] of every texel
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/distribution.h>
#include <pine/core/image.h>
#include <pine/core/light.h>

struct SkyImage {
  psl::shared_ptr<Image> image;
  vec3 tint;
  float elevation, rotation;
  int w, h;
};

static SkyImage load_image_args(char** a) {
  SkyImage s;
  s.w = atoi(a[1]), s.h = atoi(a[2]);
  std::ifstream f(a[0], std::ios::binary);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", a[0]);
    exit(2);
  }
  const size_t n = size_t(s.w) * s.h;
  if (std::string(a[3]) == "u8") {
    std::vector<vec3u8> px(n);
    f.read((char*)px.data(), std::streamsize(n * 3));
    s.image = psl::make_shared<Image>(Array2d<vec3u8>(vec2i(s.w, s.h), px.data()));
  } else {
    std::vector<vec3> px(n);
    f.read((char*)px.data(), std::streamsize(n * 12));
    s.image = psl::make_shared<Image>(Array2d<vec3>(vec2i(s.w, s.h), px.data()));
  }
  s.tint = vec3(strtof(a[4], nullptr), strtof(a[5], nullptr), strtof(a[6], nullptr));
  s.elevation = strtof(a[7], nullptr), s.rotation = strtof(a[8], nullptr);
  return s;
}

static Array2d<float> density_of(const Image& image) {  // as ImageSky's constructor computes it (light.cpp:130-131)
  auto density = Array2d<float>{image.size()};
  for_2d(image.size(), [&](auto p) { density[p] = length((vec3)image[p]); });
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

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "hdr" && argc == 4) {
    std::ifstream f(argv[2], std::ios::binary);
    std::vector<char> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    auto image = image_from(bytes.data(), bytes.size());
    if (!image) return fprintf(stderr, "image_from refused %s\n", argv[2]), 2;
    std::vector<float> out;
    const vec2i size = image->size();
    const int wh[2] = {size.x, size.y};
    out.resize(2);
    memcpy(out.data(), wh, 8);
    for_2d(size, [&](vec2i p) {
      const vec4 c = (*image)[p];
      out.push_back(c.x), out.push_back(c.y), out.push_back(c.z);
    });
    write_file(argv[3], out.data(), out.size() * 4);
    return 0;
  }
  if (argc < 11) return fprintf(stderr, "usage: see the head of tools/ref_envsky_driver.cpp\n"), 2;
  SkyImage S = load_image_args(argv + 2);
  char** rest = argv + 11;
  const int nrest = argc - 11;
  if (cmd == "texels" && nrest == 1) {
    std::vector<float> out;
    for_2d(S.image->size(), [&](vec2i p) {
      const vec4 c = (*S.image)[p];
      out.push_back(c.x), out.push_back(c.y), out.push_back(c.z);
    });
    write_file(rest[0], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "tree" && nrest == 1) {
    const auto distr = Distribution2D(density_of(*S.image), 20);
    std::vector<uint32_t> out;
    tree_stream(distr.root.get(), out);
    write_file(rest[0], out.data(), out.size() * 4);
    return 0;
  }
  if (cmd == "calls" && nrest == 3) {
    const auto sky = ImageSky(S.image, S.tint, S.elevation, S.rotation);
    const auto distr = Distribution2D(density_of(*S.image), 20);
    const std::vector<float> q = read_floats(rest[0]);
    const size_t n = q.size() / 5;
    std::vector<float> out(n * 13, 0.0f);
    std::vector<unsigned char> flags(n, 0);
    for (size_t i = 0; i < n; i++) {
      float* o = &out[i * 13];
      const vec2 u2(q[i * 5], q[i * 5 + 1]);
      const auto ds = distr.sample(u2);
      o[0] = float(ds.p.x), o[1] = float(ds.p.y);
      const long long lin = (long long)ds.p.x + (long long)ds.p.y * S.w;  // what Array2d::operator[] reads, unchecked
      if (lin < 0 || lin >= (long long)S.w * S.h) {
        flags[i] = 1;
      } else {
        const auto ls = sky.sample(vec3(0), u2);
        o[2] = ls->pdf;
        o[3] = ls->wo.x, o[4] = ls->wo.y, o[5] = ls->wo.z;
        o[6] = ls->le.x, o[7] = ls->le.y, o[8] = ls->le.z;
      }
      const vec3 wo(q[i * 5 + 2], q[i * 5 + 3], q[i * 5 + 4]);
      const vec3 c = sky.color(wo);
      o[9] = c.x, o[10] = c.y, o[11] = c.z;
      o[12] = sky.pdf(wo);
    }
    write_file(rest[1], out.data(), out.size() * 4);
    write_file(rest[2], flags.data(), flags.size());
    return 0;
  }
  if (cmd == "film" && nrest == 6) {
    Loaded L;
    load_pscene(rest[0], L);
    L.scene.set_env_light(EnvironmentLight(ImageSky(S.image, S.tint, S.elevation, S.rotation)));
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
  return fprintf(stderr, "usage: see the head of tools/ref_envsky_driver.cpp\n"), 2;
}
