// examples/atmosphere.cpp -- the physical sky through the C++ facade: the scene of examples/atmosphere.pine, its Atmosphere
// tabulated on a 64 x 32 grid (the reference's own grid, 1024 x 1024, is the default of pine::Atmosphere).
//   g++ -std=c++17 -O2 examples/atmosphere.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o build/atmosphere
//   build/atmosphere [--describe]
#include <cstdio>
#include <cstring>

#include "../pine_amd/host/pine.hpp"

int main(int argc, char** argv) {
  using namespace pine;
  try {
    const bool describe = argc > 1 && !strcmp(argv[1], "--describe");
    Scene scene;
    scene.add("floor", Diffuse{vec3(0.8f, 0.8f, 0.8f)});
    scene.add(Rect{{0, 0, 0}, {8, 0, 0}, {0, 0, 8}, true}, "floor");
    scene.add(Sphere{{-2.1f, 0.6f, 0.0f}, 0.6f}, Diffuse{vec3(0.9f, 0.4f, 0.3f)});
    scene.add(Sphere{{-0.7f, 0.6f, 0.0f}, 0.6f}, Glossy{vec3(0.3f, 0.8f, 0.4f), 0.2f});
    scene.add(Sphere{{0.7f, 0.6f, 0.0f}, 0.6f}, Metal{vec3(0.9f, 0.9f, 0.9f), 0.1f});
    scene.add(Sphere{{2.1f, 0.6f, 0.0f}, 0.6f}, Glass{vec3(1.0f, 1.0f, 1.0f), 0.0f});
    scene.set(ThinLenCamera(Film(vec2i{48, 32}, Uncharted2()), vec3(0, 1.2f, -6), vec3(0, 1.2f, 0), 0.5f));
    // (the tables on the host when the scene is only described, on the render device otherwise)
    scene.set(Atmosphere(vec3(0.3f, 1.0f, 0.2f), vec3(4.0f, 4.0f, 4.0f), vec2i{64, 32}, describe ? -1 : 0));
    if (describe) {
      printf("%s", scene.describe().c_str());
      return 0;
    }
    PathIntegrator(BlueSampler(16), 5).render(scene);
    const Film& film = scene.camera.film();
    FILE* out = fopen("atmosphere.f32", "wb");  // raw float32 RGBA, row 0 first
    if (!out || fwrite(film.pixels.data(), 4, film.pixels.size(), out) != film.pixels.size()) throw Error("cannot write atmosphere.f32");
    fclose(out);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
