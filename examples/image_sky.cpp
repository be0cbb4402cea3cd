// examples/image_sky.cpp -- an image environment light through the C++ facade: the scene of examples/image_sky.pine, lit
// by a Radiance HDR file when one is given and by the 1 x 1 image otherwise.
//   g++ -std=c++17 -O2 examples/image_sky.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o build/image_sky
//   build/image_sky [sky.hdr] [--describe]
#include <cstdio>
#include <cstring>

#include "../pine_amd/host/pine.hpp"

int main(int argc, char** argv) {
  using namespace pine;
  try {
    const char* file = nullptr;
    bool describe = false;
    for (int i = 1; i < argc; i++) {
      if (!strcmp(argv[i], "--describe")) describe = true;
      else file = argv[i];
    }
    Scene scene;
    scene.add(Rect{{0, 0, 0}, {4, 0, 0}, {0, 0, 4}, true}, Diffuse{vec3(0.8f, 0.8f, 0.8f)});
    scene.add(Sphere{{0.0f, 1.4f, 0.0f}, 0.3f}, Emissive{vec3(20.0f, 16.0f, 10.0f)});
    scene.add(Sphere{{0.6f, 0.4f, 0.2f}, 0.4f}, Diffuse{vec3(0.25f, 0.5f, 0.875f)});
    scene.set(ThinLenCamera(Film(vec2i{24, 24}, Uncharted2()), vec3(0, 1.0f, -4), vec3(0, 0.8f, 0), 0.4f));
    ImagePtr image = file ? std::make_shared<Image>(std::string(file)) : std::make_shared<Image>(vec3(0.75f, 1.0f, 1.5f));
    scene.set(file ? ImageSky(image, vec3(1, 1, 1), 0.0f, 0.25f) : ImageSky(image));
    if (describe) {
      printf("%s", scene.describe().c_str());
      if (file)
        for (float v : image->rgb) printf("%a\n", v);
      return 0;
    }
    PathIntegrator(BlueSampler(8), 3).render(scene);
    const Film& film = scene.camera.film();
    FILE* out = fopen("image_sky.f32", "wb");  // raw float32 RGBA, row 0 first
    if (!out || fwrite(film.pixels.data(), 4, film.pixels.size(), out) != film.pixels.size()) throw Error("cannot write image_sky.f32");
    fclose(out);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
