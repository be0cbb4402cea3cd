// examples/denoise.cpp -- a few-samples render of the Cornell box and its denoised twin, written against the C++ facade
// (pine_amd/host/pine.hpp): PathIntegrator, then DenoiseIntegrator on the film the camera holds.
//   g++ -std=c++17 examples/denoise.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o denoise
//   ./denoise pine_amd/data/bluesobol_u8.bin 256 8 cbox      -> cbox_noisy.png, cbox_denoised.png
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../pine_amd/host/pine.hpp"
#include "../pine_amd/host/png_writer.hpp"

using namespace pine;

static void save(Film& film, const std::string& path) {
  const vec2i size = film.size();
  if (!png_writer::write_rgba8(path, size.x, size.y, film.finalize_u8().data())) throw Error("cannot write " + path);
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s <bluesobol_u8.bin> <size> <spp> <out prefix>\n", argv[0]);
    return 2;
  }
  try {
    check(pine_gpu_set_table_path(argv[1]), "tables");
    const int size = atoi(argv[2]), spp = atoi(argv[3]);
    const std::string prefix = argv[4];
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
    const AABB unit{{0, 0, 0}, {1, 1, 1}};
    scene.add(Box(unit, translate({0.0f, 0.0f, 0.6f}) * rotate_y(0.4f) * scale({0.6f, 0.6f, 0.6f})), "floor");
    scene.add(Box(unit, translate({-0.6f, 0.0f, 1.0f}) * rotate_y(-0.4f) * scale({0.6f, 1.3f, 0.6f})), "floor");
    scene.add(Rect{{0.0f, 1.9f, 1}, {0.1f, 0, 0}, {0, 0, 0.1f}}, Emissive{600.0f * vec3{1.0f, 0.64f, 0.185f}});
    scene.set(ThinLenCamera(Film({size, size}), {0, 1, -4}, {0, 1, 0}, 0.25f));
    PathIntegrator(BlueSampler(spp), 5).render(scene);
    save(scene.camera.film(), prefix + "_noisy.png");
    // The default sigma_color is cautious (profiles/denoise_quality.txt); 0.25 smooths a picture of so few samples well.
    DenoiseParams params;
    params.sigma_color = 0.25f;
    DenoiseIntegrator(params).render(scene);
    save(scene.camera.film(), prefix + "_denoised.png");
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
