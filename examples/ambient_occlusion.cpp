// examples/ambient_occlusion.cpp -- an AOIntegrator render written against the C++ facade (pine_amd/host/pine.hpp).
//   g++ -std=c++17 examples/ambient_occlusion.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o ao
//   ./ao pine_amd/data/bluesobol_u8.bin 256 64 out.film
#include <cstdio>
#include <cstdlib>

#include "../pine_amd/host/pine.hpp"

using namespace pine;

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s <bluesobol_u8.bin> <size> <spp> <out.film>\n", argv[0]);
    return 2;
  }
  try {
    check(pine_gpu_set_table_path(argv[1]), "tables");
    const int size = atoi(argv[2]), spp = atoi(argv[3]);
    Scene scene;
    scene.add("grey", Diffuse{{0.75f, 0.75f, 0.75f}});
    scene.add(Rect{{0, 0, 1}, {4, 0, 0}, {0, 0, 4}, true}, "grey");
    scene.add(Sphere{{-0.5f, 0.5f, 1.0f}, 0.5f}, "grey");
    scene.add(Box(AABB{{0, 0, 0}, {1, 1, 1}}, translate({0.25f, 0.0f, 0.75f}) * rotate_y(0.5f) * scale({0.5f, 1.0f, 0.5f})), "grey");
    scene.set(ThinLenCamera(Film({size, size}), {0, 1, -4}, {0, 0.5f, 1}, 0.25f));
    AOIntegrator(BlueSampler(spp)).render(scene);  // (the sampler's count / 8 samples per pixel, ao.cpp:13)
    auto& film = scene.camera.film();
    FILE* f = fopen(argv[4], "wb");
    fwrite(film.pixels.data(), 4, film.pixels.size(), f);
    fclose(f);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
