// tools/ref_accel_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_accel.py; no test runs it).
//
// Our own driver around the REAL reference's Accel (src/pine/core/accel.h:10-25).  It is compiled where the reference's sources
// lie and linked with oracle/_ref/libpine_ref.a -- and, with -DPINE_REF_WITH_EMBREE, with the Embree that `make -C oracle embree`
// built from the reference's vendored copy; the binary goes to a scratch directory.  The scene is built from a .pscene exactly
// as oracle/ref_driver.cpp builds it (that file -- this repository's own -- is included for its loader), then per ray
// Accel::intersect(ray, it) and Accel::hit(ray) are called, for Accel(BVH()) or Accel(EmbreeAccel()).
//
//   ref_accel_driver <bvh|embree> <scene.pscene> <rays.bin> <out.records> <out.occluded>
//     rays.bin      8 floats per ray: o, d, tmin, tmax
//     out.records   12 words per ray (include/pine_gpu.h, pine_gpu_accel_intersect_device): ray.tmax after the query, geometry,
//                   triangle, material, it.p, it.n, it.uv; on a miss tmax as it came, -1 -1 -1, zeros
//     out.occluded  one byte per ray: Accel::hit
//
// Two of the words are not fields of the reference's interaction and are looked up from what it does hold.
//   geometry, material: the geometry whose shape `it.shape` points to, and the place of its material in the description.
//   triangle: Accel::intersect keeps the winning triangle in a local.  With BVH() the same query is run once more through the
//     BVH's own two levels with BVH::intersect's callbacks (bvh.cpp:513-548, as the `bvh` command of oracle/ref_driver.cpp does)
//     and must agree with Accel::intersect in hit, geometry and tmax bits: its triangle is the word.  With EmbreeAccel() the word
//     is the triangle of the hit mesh that lies nearest to it.p (in double precision); under BVH() that rule is evaluated too and
//     the count of rays where it names another triangle than the traversal is printed (it must be 0 for the fixture to be kept).
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/accel.h>

#include <cmath>

namespace {
struct D3 {
  double x, y, z;
};
D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 d3(vec3 v) { return {v.x, v.y, v.z}; }
// squared distance from p to triangle abc (closest point by regions)
double dist2_triangle(D3 p, D3 a, D3 b, D3 c) {
  const D3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
  auto len2 = [](D3 v) { return dot(v, v); };
  const double d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0 && d2 <= 0) return len2(ap);
  const D3 bp = sub(p, b);
  const double d3_ = dot(ab, bp), d4 = dot(ac, bp);
  if (d3_ >= 0 && d4 <= d3_) return len2(bp);
  const double vc = d1 * d4 - d3_ * d2;
  if (vc <= 0 && d1 >= 0 && d3_ <= 0) {
    const double v = d1 / (d1 - d3_);
    return len2(sub(ap, D3{ab.x * v, ab.y * v, ab.z * v}));
  }
  const D3 cp = sub(p, c);
  const double d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0 && d5 <= d6) return len2(cp);
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0 && d2 >= 0 && d6 <= 0) {
    const double w = d2 / (d2 - d6);
    return len2(sub(ap, D3{ac.x * w, ac.y * w, ac.z * w}));
  }
  const double va = d3_ * d6 - d5 * d4;
  if (va <= 0 && (d4 - d3_) >= 0 && (d5 - d6) >= 0) {
    const double w = (d4 - d3_) / ((d4 - d3_) + (d5 - d6));
    const D3 bc = sub(c, b);
    return len2(sub(bp, D3{bc.x * w, bc.y * w, bc.z * w}));
  }
  const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
  return len2(sub(ap, D3{ab.x * v + ac.x * w, ab.y * v + ac.y * w, ab.z * v + ac.z * w}));
}
int nearest_triangle(const Mesh& mesh, vec3 p) {
  int best = -1;
  double best_d = 0;
  for (size_t t = 0; t < mesh.num_triangles(); t++) {
    const auto face = mesh.indices[t];
    const double d = dist2_triangle(d3(p), d3(mesh.vertices[face[0]]), d3(mesh.vertices[face[1]]), d3(mesh.vertices[face[2]]));
    if (best < 0 || d < best_d) best = int(t), best_d = d;
  }
  return best;
}
uint32_t bits(float f) {
  uint32_t w;
  memcpy(&w, &f, 4);
  return w;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: ref_accel_driver <bvh|embree> <scene.pscene> <rays.bin> <out.records> <out.occluded>\n");
    return 2;
  }
  const bool embree = std::string(argv[1]) == "embree";
#ifndef PINE_REF_WITH_EMBREE
  if (embree) {
    fprintf(stderr, "this binary was built without Embree (make -C oracle embree)\n");
    return 2;
  }
#endif
  Loaded L;
  load_pscene(argv[2], L);
  auto& scene = L.scene;
  Accel accel =
#ifdef PINE_REF_WITH_EMBREE
      embree ? Accel(EmbreeAccel()) :
#endif
             Accel(BVH());
  accel.build(&scene);
  BVH two_level;  // (BVH() only: the same tree once more, for the triangle word)
  if (!embree) two_level.build(&scene);
  const BVHImpl& tbvh = two_level.*rob(TagTbvh{});
  const auto& lbvh = two_level.*rob(TagLbvh{});
  const auto& indices = two_level.*rob(TagIndices{});

  std::ifstream rf(argv[3], std::ios::binary);
  rf.seekg(0, std::ios::end);
  const size_t nbytes = rf.tellg();
  rf.seekg(0);
  std::vector<float> rays(nbytes / 4);
  rf.read((char*)rays.data(), nbytes);

  std::vector<uint32_t> records;
  std::vector<uint8_t> occluded;
  size_t hits = 0, mesh_hits = 0, nearest_differs = 0;
  for (size_t r = 0; r + 8 <= rays.size(); r += 8) {
    const float* q = &rays[r];
    Ray ray(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7]);
    SurfaceInteraction it;
    const bool hit = accel.intersect(ray, it);
    occluded.push_back(accel.hit(Ray(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7])) ? 1 : 0);
    int geom = -1, tri = -1, material = -1;
    if (hit) {
      hits++;
      for (size_t g = 0; g < scene.geometries.size(); g++)
        if (it.shape == &scene.geometries[g]->shape) geom = int(g);
      if (geom < 0) {
        fprintf(stderr, "ray %zu: the interaction's shape is no geometry of the scene\n", r / 8);
        return 1;
      }
      for (size_t m = 0; m < L.material_order.size(); m++)
        if (scene.materials[psl::string(L.material_order[m].c_str())].get() == scene.geometries[geom]->material.get()) material = int(m);
      if (material < 0 || &it.material() != scene.geometries[geom]->material.get()) {
        fprintf(stderr, "ray %zu: the interaction's material is not its geometry's\n", r / 8);
        return 1;
      }
      if (it.shape->is<Mesh>()) {
        mesh_hits++;
        const int nearest = nearest_triangle(it.shape->as<Mesh>(), it.p);
        tri = nearest;
        if (!embree) {
          Ray ray2(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7]);
          SurfaceInteraction it2;
          uint32_t geom_index = 0, prim_index = 0;
          const bool hit2 = tbvh.Intersect(ray2, [&](Ray& ray, int i_lbvh) {
            auto& geometry = scene.geometries[indices[i_lbvh]];
            if (i_lbvh < int(lbvh.size())) {
              auto& mesh = geometry->shape.as<Mesh>();
              auto h = lbvh[i_lbvh].Intersect(ray, [&](Ray& ray, int index) {
                auto hh = mesh.intersect(ray, index);
                if (hh) prim_index = index;
                return hh;
              });
              if (h) geom_index = indices[i_lbvh];
              return h;
            } else {
              auto h = geometry->intersect(ray, it2);
              if (h) geom_index = indices[i_lbvh];
              return h;
            }
          });
          if (!hit2 || int(geom_index) != geom || bits(ray2.tmax) != bits(ray.tmax)) {
            fprintf(stderr, "ray %zu: the two-level walk disagrees with Accel::intersect\n", r / 8);
            return 1;
          }
          tri = int(prim_index);
          if (nearest != tri) nearest_differs++;
        }
      }
    }
    records.push_back(bits(ray.tmax));
    records.push_back(uint32_t(geom)), records.push_back(uint32_t(tri)), records.push_back(uint32_t(material));
    const float f[8] = {it.p.x, it.p.y, it.p.z, it.n.x, it.n.y, it.n.z, it.uv.x, it.uv.y};
    for (float v : f) records.push_back(hit ? bits(v) : 0u);
  }
  write_file(argv[4], records.data(), records.size() * 4);
  write_file(argv[5], occluded.data(), occluded.size());
  printf("{\"rays\": %zu, \"accel\": \"%s\", \"hits\": %zu, \"mesh_hits\": %zu, \"nearest_differs\": %zu}\n", rays.size() / 8, embree ? "embree" : "bvh", hits,
         mesh_hits, nearest_differs);
  return 0;
}
