// tools/ref_noise_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_noise.py; no test runs it).
//
// Our own driver around the REAL reference's NodeNoisef / NodeNoise3f.  It is compiled where the reference's sources lie,
// together with the reference's impl/integrator/denoiser.cpp read from its own place, and linked with
// oracle/_ref/libpine_ref.a; the binary goes to a scratch directory.  Only the reference's public API is called.  A scene
// arrives in two files: the `node` and `material` lines of its .pscene (FRONT), read here -- oracle/ref_driver.cpp's loader
// knows no noise node -- and the remaining lines (REST: shapes, lights, camera), read by that loader (that file -- this
// repository's own -- is included for it) into the scene that already holds the materials.
//
//   ref_noise_driver calls  <front> <queries.bin> <out.records>
//       per material (description order) and query (8 floats: p, n, uv) 10 floats, the layout of pine_gpu_test_material_params:
//       albedo, albedo / Pi, roughness, metallic, transmission, ior -- each the material's own member evaluated at
//       NodeEvalCtx{p, n, uv}; a member the material does not have is 0
//   ref_noise_driver sense  <queries.bin> <max octaves>
//       sensitivity of the queries to perlin_interp's binary64 step: fbm(p, o) of the reference beside the same sum over a
//       perlin_interp written here with `1.0f` literals, for every query's p and o = 1 .. max; prints both counts
//   ref_noise_driver film   <front> <rest> <spp> <depth> <out.film> <out.first>
//       PathIntegrator(BVH(), BlueSampler(spp), UniformLightSampler(), depth).render; out.film raw vec4; out.first one byte per
//       pixel: 1 + the index (description order) of the material the camera ray through the pixel's centre meets first, 0: none
//   ref_noise_driver guides <front> <rest> <out.albedo> <out.normal>
//       DenoiseIntegrator(BVH(), SobolSampler(1), UniformLightSampler()).render with this driver's denoise() (as
//       tools/ref_guides_driver.cpp): the guide images it is handed, raw vec3
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/denoise.h>
#include <pine/core/noise.h>
#include <pine/core/rng.h>
#include <pine/impl/integrator/denoiser.h>

static const char* g_albedo_path = nullptr;
static const char* g_normal_path = nullptr;
static int g_denoise_calls = 0;

namespace pine {
void denoise(DenoiseQuality, Array2d<vec3>& output, const Array2d<vec3>& color, const Array2d<vec3>* albedo, const Array2d<vec3>* normal) {
  if (!albedo || !normal) {
    fprintf(stderr, "denoise() was called without guide images\n");
    exit(3);
  }
  write_file(g_albedo_path, albedo->data(), size_t(12) * albedo->width() * albedo->height());
  write_file(g_normal_path, normal->data(), size_t(12) * normal->width() * normal->height());
  if (&output != &color) output = color;
  g_denoise_calls++;
}
}  // namespace pine

struct Front {
  std::vector<psl::optional<Nodef>> nf;
  std::vector<psl::optional<Node3f>> n3;
};

template <char Op>
static void binary(Front& T, int id, bool vec, int a, int b) {
  if (vec) T.n3[id] = Node3f(NodeBinary<vec3, Op>(*T.n3[a], *T.n3[b]));
  else T.nf[id] = Nodef(NodeBinary<float, Op>(*T.nf[a], *T.nf[b]));
}
template <char Op>
static void unary(Front& T, int id, bool vec, int a) {
  if (vec) T.n3[id] = Node3f(NodeUnary<vec3, Op>(*T.n3[a]));
  else T.nf[id] = Nodef(NodeUnary<float, Op>(*T.nf[a]));
}

static void load_front(const char* path, Front& T, Loaded& out) {
  std::ifstream f(path);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    std::string kw;
    in >> kw;
    if (kw == "node") {
      int id, a = -1, b = -1, c = -1;
      std::string kind, op;
      in >> id >> kind;
      T.nf.emplace_back();
      T.n3.emplace_back();
      if (kind == "constf") T.nf[id] = Nodef(rdf(in));
      else if (kind == "const3") T.n3[id] = Node3f(rd3(in));
      else if (kind == "position") T.n3[id] = Node3f(NodePosition());
      else if (kind == "normal") T.n3[id] = Node3f(NodeNormal());
      else if (kind == "uv") T.n3[id] = Node3f(NodeUV());
      else if (kind == "binf" || kind == "bin3") {
        in >> op >> a >> b;
        const bool v = kind == "bin3";
        switch (op[0]) {
          case '+': binary<'+'>(T, id, v, a, b); break;
          case '-': binary<'-'>(T, id, v, a, b); break;
          case '*': binary<'*'>(T, id, v, a, b); break;
          case '/': binary<'/'>(T, id, v, a, b); break;
          default: binary<'^'>(T, id, v, a, b); break;
        }
      } else if (kind == "unf" || kind == "un3") {
        in >> op >> a;
        const bool v = kind == "un3";
        switch (op[0]) {
          case '-': unary<'-'>(T, id, v, a); break;
          case 'a': unary<'a'>(T, id, v, a); break;
          case 's': unary<'s'>(T, id, v, a); break;
          case 'r': unary<'r'>(T, id, v, a); break;
          default: unary<'f'>(T, id, v, a); break;
        }
      } else if (kind == "comp") {
        int n;
        in >> a >> n;
        T.nf[id] = Nodef(NodeComponent(*T.n3[a], n));
      } else if (kind == "tovec3") {
        in >> a;
        if (in >> b >> c) T.n3[id] = Node3f(NodeToVec3(*T.nf[a], *T.nf[b], *T.nf[c]));
        else T.n3[id] = Node3f(NodeToVec3(*T.nf[a]));
      } else if (kind == "checker") {
        in >> a;
        T.nf[id] = Nodef(NodeCheckerboard(*T.n3[a], rdf(in)));
      } else if (kind == "splat") {
        in >> a;
        T.n3[id] = Node3f(*T.nf[a]);
      } else if (kind == "noisef") {
        in >> a >> b;
        T.nf[id] = Nodef(NodeNoisef(*T.n3[a], *T.nf[b]));
      } else if (kind == "noise3f") {
        in >> a >> b;
        T.n3[id] = Node3f(NodeNoise3f(*T.n3[a], *T.nf[b]));
      } else {
        fprintf(stderr, "unknown node kind %s\n", kind.c_str());
        exit(2);
      }
    } else if (kw == "material") {
      std::string name, kind;
      in >> name >> kind;
      out.material_order.push_back(name);
      int a, r, m, t, i;
      auto& scene = out.scene;
      if (kind == "diffuse_n") {
        in >> a;
        scene.add_material(name.c_str(), Material(DiffuseMaterial(*T.n3[a])));
      } else if (kind == "uber_n") {
        in >> a >> r >> m >> t;
        scene.add_material(name.c_str(), Material(UberMaterial(*T.n3[a], *T.nf[r], *T.nf[m], *T.nf[t], rdf(in))));
      } else if (kind == "metal") {
        in >> a >> r;
        scene.add_material(name.c_str(), Material(MetalMaterial(*T.n3[a], *T.nf[r])));
      } else if (kind == "glossy") {
        in >> a >> r >> i;
        scene.add_material(name.c_str(), Material(GlossyMaterial(*T.n3[a], *T.nf[r], *T.nf[i])));
      } else if (kind == "glass") {
        in >> a >> r >> i;
        scene.add_material(name.c_str(), Material(GlassMaterial(*T.n3[a], *T.nf[r], *T.nf[i])));
      } else if (kind == "emissive") {
        scene.add_material(name.c_str(), Material(EmissiveMaterial(rd3(in))));
      } else if (kind == "diffuse") {
        scene.add_material(name.c_str(), Material(DiffuseMaterial(rd3(in))));
      } else {
        fprintf(stderr, "unknown material kind %s\n", kind.c_str());
        exit(2);
      }
    } else {
      fprintf(stderr, "the front file holds node and material lines only: %s\n", kw.c_str());
      exit(2);
    }
  }
}

// The sensitivity probe's own sum: the steps of fbm over a Perlin noise whose interpolation has `1.0f` where the
// reference's has `1.0` -- what a restatement in binary32 alone would compute.  Built from the reference's public functions.
static float noise_all_float(vec3 np, int seed) {
  const vec3 cell = floor(np);
  vec3 t = np - cell;
  t = t * t * (vec3(3) - 2 * t);
  float sum = 0;
  for (int k = 0; k < 8; k++) {  // x, y, z with z innermost, as perlin_interp visits them
    const vec3i corner(k >> 2, (k >> 1) & 1, k & 1);
    RNG rng(hash(vec3i(cell + corner), seed));
    const vec3 gradient = unit_square_to_cartesian(rng.next2f());
    const float wx = corner.x ? t.x : 1.0f - t.x, wy = corner.y ? t.y : 1.0f - t.y, wz = corner.z ? t.z : 1.0f - t.z;
    sum += wx * wy * wz * dot(gradient, t - vec3(corner));
  }
  return 0.5f * (1.0f + sum);
}
static float fbm_all_float(vec3 np, int octaves) {
  float accum = 0, weight = 1.0f;
  for (int i = 0; i < octaves; i++) {
    accum += weight * noise_all_float(np, 0);
    weight *= 0.5f;
    np *= 2.0f;
  }
  return psl::sqr(accum / (2.0f - weight * 2));
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "sense" && argc == 4) {
    const std::vector<float> qs = read_floats(argv[2]);
    const size_t nq = qs.size() / 8;
    const int top = atoi(argv[3]);
    size_t differ = 0, total = 0, same_check = 0;
    for (size_t i = 0; i < nq; i++)
      for (int o = 1; o <= top; o++) {
        const vec3 p(qs[i * 8], qs[i * 8 + 1], qs[i * 8 + 2]);
        const float a = fbm(p, o), b = fbm_all_float(p, o);
        total++;
        differ += memcmp(&a, &b, 4) != 0;
        // (the probe's loop itself is the reference's: with the reference's own noise it gives the reference's bits)
        float accum = 0, weight = 1.0f;
        vec3 np = p;
        for (int k = 0; k < o; k++) accum += weight * perlin_noise(np, 0), weight *= 0.5f, np *= 2.0f;
        const float c = psl::sqr(accum / (2.0f - weight * 2));
        same_check += memcmp(&a, &c, 4) == 0;
      }
    if (same_check != total) return fprintf(stderr, "the probe's fbm loop does not reproduce the reference's fbm\n"), 3;
    printf("{\"evaluations\": %zu, \"differ_with_float_interp\": %zu}\n", total, differ);
    return 0;
  }
  if (argc < 4) return fprintf(stderr, "usage: see the head of tools/ref_noise_driver.cpp\n"), 2;
  Front T;
  Loaded L;
  load_front(argv[2], T, L);
  if (cmd == "calls" && argc == 5) {
    const std::vector<float> qs = read_floats(argv[3]);
    const size_t nq = qs.size() / 8;
    std::vector<float> out;
    for (const std::string& name : L.material_order) {
      const Material& mat = *L.scene.materials[psl::string(name.c_str())];
      for (size_t i = 0; i < nq; i++) {
        const float* q = &qs[i * 8];
        const NodeEvalCtx c(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), vec2(q[6], q[7]));
        float rec[10] = {};
        mat.dispatch([&](const auto& x) {
          using M = std::decay_t<decltype(x)>;
          vec3 a;
          if constexpr (std::is_same_v<M, EmissiveMaterial>) a = x.color.eval(c);
          else a = x.albedo.eval(c);
          const vec3 ap = a / Pi;  // the Lambertian f (bxdf.cpp:21,27)
          rec[0] = a.x, rec[1] = a.y, rec[2] = a.z, rec[3] = ap.x, rec[4] = ap.y, rec[5] = ap.z;
          if constexpr (requires { x.roughness; }) rec[6] = x.roughness.eval(c);
          if constexpr (requires { x.metallic; }) rec[7] = x.metallic.eval(c);
          if constexpr (requires { x.transmission; }) rec[8] = x.transmission.eval(c);
          if constexpr (requires { x.ior; }) {
            if constexpr (std::is_same_v<std::decay_t<decltype(x.ior)>, float>) rec[9] = x.ior;
            else rec[9] = x.ior.eval(c);
          }
        });
        out.insert(out.end(), rec, rec + 10);
      }
    }
    write_file(argv[4], out.data(), out.size() * 4);
    printf("{\"queries\": %zu, \"materials\": %zu}\n", nq, L.material_order.size());
    return 0;
  }
  if (cmd == "film" && argc == 8) {
    load_pscene(argv[3], L);
    const int spp = atoi(argv[4]), depth = atoi(argv[5]);
    auto integ = PathIntegrator(Accel(BVH()), Sampler(BlueSobolSampler(spp)), UniformLightSampler(), depth);
    integ.render(L.scene);
    auto& film = L.scene.camera.film();
    write_file(argv[6], film.data(), size_t(16) * L.W * L.H);
    Accel accel = Accel(BVH());
    accel.build(&L.scene);
    std::vector<unsigned char> first(size_t(L.W) * L.H, 0);
    for (int y = 0; y < L.H; y++)
      for (int x = 0; x < L.W; x++) {
        Ray ray = L.scene.camera.gen_ray((vec2(x, y) + vec2(0.5f)) / film.size(), vec2(0.5f));
        SurfaceInteraction it;
        if (!accel.intersect(ray, it)) continue;
        const Material* m = &it.material();
        for (size_t k = 0; k < L.material_order.size(); k++)
          if (L.scene.materials[psl::string(L.material_order[k].c_str())].get() == m) first[size_t(y) * L.W + x] = (unsigned char)(k + 1);
      }
    write_file(argv[7], first.data(), first.size());
    return 0;
  }
  if (cmd == "guides" && argc == 6) {
    load_pscene(argv[3], L);
    g_albedo_path = argv[4], g_normal_path = argv[5];
    L.scene.camera.film().clear();
    auto integ = DenoiseIntegrator(Accel(BVH()), Sampler(SobolSampler(1)), LightSampler(UniformLightSampler()));
    integ.render(L.scene);
    if (g_denoise_calls != 1) return fprintf(stderr, "DenoiseIntegrator::render did not reach this driver's denoise()\n"), 3;
    return 0;
  }
  return fprintf(stderr, "usage: see the head of tools/ref_noise_driver.cpp\n"), 2;
}
