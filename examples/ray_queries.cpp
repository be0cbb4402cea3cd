// examples/ray_queries.cpp -- ray queries against the Cornell box through the C++ facade (pine_amd/host/pine.hpp): what a
// CustomRayIntegrator's radiance() calls as intersect(ray, it) and hit(ray) (core/integrator.h:61-74), for a batch of rays.
//   g++ -std=c++17 examples/ray_queries.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o ray_queries
//   ./ray_queries <bvh|embree> <out.bin> [<out.pscene>]
// 64 rays from the camera through an 8 x 8 grid of the view; out.bin: 64 rays (8 floats each), 64 hit records (12 words each),
// 64 occlusion bytes.  tests/test_accel_gpu.py compares them with what the Python interface answers for the same scene and rays.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../pine_amd/host/pine.hpp"

using namespace pine;

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <bvh|embree> <out.bin> [<out.pscene>]\n", argv[0]);
    return 2;
  }
  try {
    Scene scene;
    scene.add("floor", Diffuse{{0.9f, 0.9f, 0.9f}});
    scene.add("blue", Diffuse{{0.2f, 0.5f, 0.9f}});
    scene.add("red", Diffuse{{0.9f, 0.1f, 0.05f}});
    scene.add("green", Diffuse{{0.2f, 0.9f, 0.05f}});
    scene.add(Rect{{0, 0, 1}, {2, 0, 0}, {0, 0, 2}, true}, "floor");
    scene.add(Rect{{0, 2, 1}, {2, 0, 0}, {0, 0, 2}}, "floor");
    scene.add(Rect{{-1, 1, 1}, {0, 0, 2}, {0, 2, 0}, true}, "red");
    scene.add(Rect{{1, 1, 1}, {0, 0, 2}, {0, 2, 0}}, "green");
    scene.add(Rect{{0, 1, 2}, {2, 0, 0}, {0, 2, 0}, true}, "blue");
    scene.add(Box(AABB{{0, 0, 0}, {1, 1, 1}}, translate({0.0f, 0.0f, 0.6f}) * rotate_y(0.4f) * scale({0.6f, 0.6f, 0.6f})), "floor");
    scene.add(Box(AABB{{0, 0, 0}, {1, 1, 1}}, translate({-0.6f, 0.0f, 1.0f}) * rotate_y(-0.4f) * scale({0.6f, 1.3f, 0.6f})), "floor");
    scene.add(Rect{{0.0f, 1.9f, 1}, {0.1f, 0, 0}, {0, 0, 0.1f}}, Emissive{600.0f * vec3{1.0f, 0.64f, 0.185f}});
    scene.set(ThinLenCamera(Film({64, 64}, Uncharted2()), {0, 1, -4}, {0, 1, 0}, 0.25f));

    std::vector<Ray> rays;
    for (int y = 0; y < 8; y++)
      for (int x = 0; x < 8; x++) {
        Ray r;
        r.o = {0.0f, 1.0f, -4.0f};
        r.d = {(float(x) - 3.5f) * 0.08f, (float(y) - 3.5f) * 0.08f, 1.0f};  // (not normalised: t is in units of d)
        if ((x + y) % 3 == 0) r.tmax = 4.5f;                                  // (some stop short of the back wall)
        rays.push_back(r);
      }
    std::vector<Interaction> hits(rays.size());
    std::vector<uint8_t> occluded(rays.size());
    if (std::string(argv[1]) == "embree") {
      Accel accel(scene, Embree{});
      accel.intersect(rays.data(), int64_t(rays.size()), hits.data());
      accel.hit(rays.data(), int64_t(rays.size()), occluded.data());
    } else {
      Accel accel(scene, BVH{});
      accel.intersect(rays.data(), int64_t(rays.size()), hits.data());
      accel.hit(rays.data(), int64_t(rays.size()), occluded.data());
    }
    int nhit = 0;
    for (const Interaction& it : hits) nhit += it.hit() ? 1 : 0;
    printf("%d of %zu rays hit; the first: t %.6f geometry %d material %d p (%.4f %.4f %.4f) n (%.1f %.1f %.1f)\n", nhit, hits.size(), hits[0].t,
           hits[0].geometry, hits[0].material, hits[0].p[0], hits[0].p[1], hits[0].p[2], hits[0].n[0], hits[0].n[1], hits[0].n[2]);
    FILE* f = fopen(argv[2], "wb");
    if (!f) throw Error(std::string("cannot write ") + argv[2]);
    fwrite(rays.data(), sizeof(Ray), rays.size(), f);
    fwrite(hits.data(), sizeof(Interaction), hits.size(), f);
    fwrite(occluded.data(), 1, occluded.size(), f);
    fclose(f);
    if (argc > 3) {
      const std::string text = scene.describe();
      FILE* g = fopen(argv[3], "wb");
      if (!g) throw Error(std::string("cannot write ") + argv[3]);
      fwrite(text.data(), 1, text.size(), g);
      fclose(g);
    }
  } catch (const Error& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
