// tools/ref_texture_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_texture.py; no test runs it).
//
// Our own driver around the REAL reference's NodeImage / NodeImagef.  It is compiled where the reference's sources lie, together
// with the reference's impl/integrator/denoiser.cpp read from its own place, and linked with oracle/_ref/libpine_ref.a; the
// binary goes to a scratch directory.  Only the reference's public API is called.  A textured scene arrives in two files: the
// `image`, `node` and `material` lines of its .pscene (FRONT), read here -- oracle/ref_driver.cpp's loader knows no image --
// and the remaining lines (REST: shapes, lights, camera), read by that loader (that file -- this repository's own -- is
// included for it) into the scene that already holds the materials.  The texels of image <i> are <dir>/image_<i>.bin, as the
// caller handed them over: 3 floats, or 3 or 4 bytes, per texel.
//
//   ref_texture_driver calls  <dir> <front> <queries.bin> <out.records> <out.lookups>
//       per material (description order) and query (8 floats: p, n, uv) 10 floats, the layout of pine_gpu_test_material_params:
//       albedo, albedo / Pi, roughness, metallic, transmission, ior -- each the material's own member evaluated at
//       NodeEvalCtx{p, n, uv}; a member the material does not have is 0.  out.lookups: per image node (description order) and
//       query 4 int32: the image, vec2i(size * fract(vec2(p))) BEFORE the min -- p the reference's value of the node's coordinate
//       operand -- and 1 where the coordinate is not finite or the index after the min lies outside the image
//   ref_texture_driver film   <dir> <front> <rest> <spp> <depth> <out.film> <out.first>
//       PathIntegrator(BVH(), BlueSampler(spp), UniformLightSampler(), depth).render; out.film raw vec4; out.first one byte per
//       pixel: 1 + the index (description order) of the material the camera ray through the pixel's centre meets first, 0: none
//   ref_texture_driver glb    <file.glb> <w> <h> <spp> <depth> <out.film> <out.first>
//       the reference's OWN importer (load_scene -> scene_from_gltf, fileio.cpp:146-330 through tinygltf) builds the scene;
//       the camera it set keeps its position and orientation and gets a film of w x h (the importer's is 640 high) and the
//       fov2d the constructor derives from it (camera.cpp:14); then as `film`, out.first counting geometries
//   ref_texture_driver png    <file.png> <out.bin>
//       int32 width, height, then what image_from returns (fileio.cpp:78-95: stb, 3 channels), then what tinygltf's own
//       LoadImageData returns (4 channels); a loader that refuses the file ends the driver with status 4
//   ref_texture_driver guides <dir> <front> <rest> <out.albedo> <out.normal>
//       DenoiseIntegrator(BVH(), SobolSampler(1), UniformLightSampler()).render with this driver's denoise() (as
//       tools/ref_guides_driver.cpp): the guide images it is handed, raw vec3
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/denoise.h>
#include <pine/core/fileio.h>
#include <pine/core/image.h>
#include <tiny_gltf.h>
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

struct ImageNode {
  int coordinate, image;
};
struct Front {
  std::vector<psl::shared_ptr<Image>> images;
  std::vector<psl::optional<Nodef>> nf;
  std::vector<psl::optional<Node3f>> n3;
  std::vector<ImageNode> image_nodes;
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

static std::vector<char> read_bytes(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path.c_str());
    exit(2);
  }
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void load_front(const std::string& dir, const char* path, Front& T, Loaded& out) {
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
    if (kw == "image") {
      int id, w, h;
      std::string kind;
      in >> id >> w >> h >> kind;
      const std::vector<char> bytes = read_bytes(dir + "/image_" + std::to_string(id) + ".bin");
      const size_t n = size_t(w) * h, per = kind == "f32" ? 12 : kind == "u8x3" ? 3 : 4;
      if (bytes.size() != n * per) {
        fprintf(stderr, "image %d: %zu bytes for %d x %d %s\n", id, bytes.size(), w, h, kind.c_str());
        exit(2);
      }
      if (kind == "f32") T.images.push_back(psl::make_shared<Image>(Array2d<vec3>(vec2i(w, h), (const vec3*)bytes.data())));
      else if (kind == "u8x3") T.images.push_back(psl::make_shared<Image>(Array2d<vec3u8>(vec2i(w, h), (const vec3u8*)bytes.data())));
      else T.images.push_back(psl::make_shared<Image>(Array2d<vec4u8>(vec2i(w, h), (const vec4u8*)bytes.data())));
    } else if (kw == "node") {
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
      } else if (kind == "image" || kind == "imagef") {
        int image;
        in >> a >> image;
        if (kind == "image") T.n3[id] = Node3f(NodeImage(*T.n3[a], T.images[size_t(image)]));
        else T.nf[id] = Nodef(NodeImagef(*T.n3[a], T.images[size_t(image)]));
        T.image_nodes.push_back(ImageNode{a, image});
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
      fprintf(stderr, "the front file holds image, node and material lines only: %s\n", kw.c_str());
      exit(2);
    }
  }
}

int main(int argc, char** argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "png" && argc == 4) {
    std::vector<char> bytes = read_bytes(argv[2]);
    auto image = image_from(bytes.data(), bytes.size());
    tinygltf::Image gi;
    std::string err, warn;
    if (!image || !image->is<Array2d<vec3u8>>()) return fprintf(stderr, "image_from refused %s\n", argv[2]), 4;
    if (!tinygltf::LoadImageData(&gi, 0, &err, &warn, 0, 0, (const unsigned char*)bytes.data(), int(bytes.size()), nullptr))
      return fprintf(stderr, "tinygltf refused %s: %s\n", argv[2], err.c_str()), 4;
    const vec2i size = image->size();
    if (gi.width != size.x || gi.height != size.y || gi.component != 4 || gi.bits != 8) return fprintf(stderr, "tinygltf: unexpected layout\n"), 4;
    std::vector<unsigned char> out(8);
    const int wh[2] = {size.x, size.y};
    memcpy(out.data(), wh, 8);
    const auto& a = image->as<Array2d<vec3u8>>();
    out.insert(out.end(), (const unsigned char*)a.data(), (const unsigned char*)a.data() + size_t(3) * size.x * size.y);
    out.insert(out.end(), gi.image.begin(), gi.image.end());
    write_file(argv[3], out.data(), out.size());
    return 0;
  }
  if (cmd == "glb" && argc == 9) {
    Scene scene = load_scene(argv[2]);
    const int w = atoi(argv[3]), h = atoi(argv[4]), spp = atoi(argv[5]), depth = atoi(argv[6]);
    auto& cam = scene.camera.as<ThinLenCamera>();
    const float fov = cam.fov2d.y;
    cam.film_ = Film(vec2i(w, h));
    cam.fov2d = vec2(fov * cam.film_.aspect(), fov);
    auto integ = PathIntegrator(Accel(BVH()), Sampler(BlueSobolSampler(spp)), UniformLightSampler(), depth);
    integ.render(scene);
    auto& film = scene.camera.film();
    write_file(argv[7], film.data(), size_t(16) * w * h);
    Accel accel = Accel(BVH());
    accel.build(&scene);
    std::vector<unsigned char> first(size_t(w) * h, 0);
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        Ray ray = scene.camera.gen_ray((vec2(x, y) + vec2(0.5f)) / film.size(), vec2(0.5f));
        SurfaceInteraction it;
        if (!accel.intersect(ray, it)) continue;
        for (size_t k = 0; k < scene.geometries.size(); k++)
          if (scene.geometries[k]->material.get() == &it.material()) first[size_t(y) * w + x] = (unsigned char)(k + 1);
      }
    write_file(argv[8], first.data(), first.size());
    return 0;
  }
  if (argc < 4) return fprintf(stderr, "usage: see the head of tools/ref_texture_driver.cpp\n"), 2;
  Front T;
  Loaded L;
  load_front(argv[2], argv[3], T, L);
  if (cmd == "calls" && argc == 7) {
    const std::vector<float> qs = read_floats(argv[4]);
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
    write_file(argv[5], out.data(), out.size() * 4);
    std::vector<int32_t> look;
    for (const ImageNode& k : T.image_nodes)
      for (size_t i = 0; i < nq; i++) {
        const float* q = &qs[i * 8];
        const NodeEvalCtx c(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), vec2(q[6], q[7]));
        const vec3 p = T.n3[size_t(k.coordinate)]->eval(c);
        const vec2i size = T.images[size_t(k.image)]->size();
        const bool finite = std::isfinite(p.x) && std::isfinite(p.y);
        vec2i raw(0, 0), sc(0, 0);
        if (finite) {
          raw = vec2i(size * fract(vec2(p)));  // node.cpp:21, before the min
          sc = min(raw, size - vec2i(1));
        }
        const bool outside = !finite || sc.x < 0 || sc.y < 0 || sc.x >= size.x || sc.y >= size.y;
        look.insert(look.end(), {int32_t(k.image), int32_t(raw.x), int32_t(raw.y), int32_t(outside)});
      }
    write_file(argv[6], look.data(), look.size() * 4);
    printf("{\"queries\": %zu, \"materials\": %zu, \"image_nodes\": %zu}\n", nq, L.material_order.size(), T.image_nodes.size());
    return 0;
  }
  if (cmd == "film" && argc == 9) {
    load_pscene(argv[4], L);
    const int spp = atoi(argv[5]), depth = atoi(argv[6]);
    auto integ = PathIntegrator(Accel(BVH()), Sampler(BlueSobolSampler(spp)), UniformLightSampler(), depth);
    integ.render(L.scene);
    auto& film = L.scene.camera.film();
    write_file(argv[7], film.data(), size_t(16) * L.W * L.H);
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
    write_file(argv[8], first.data(), first.size());
    return 0;
  }
  if (cmd == "guides" && argc == 7) {
    load_pscene(argv[4], L);
    g_albedo_path = argv[5], g_normal_path = argv[6];
    L.scene.camera.film().clear();
    auto integ = DenoiseIntegrator(Accel(BVH()), Sampler(SobolSampler(1)), LightSampler(UniformLightSampler()));
    integ.render(L.scene);
    if (g_denoise_calls != 1) return fprintf(stderr, "DenoiseIntegrator::render did not reach this driver's denoise()\n"), 3;
    return 0;
  }
  return fprintf(stderr, "usage: see the head of tools/ref_texture_driver.cpp\n"), 2;
}
