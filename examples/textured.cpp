// examples/textured.cpp -- image textures through the C++ facade.  The facade has no shading nodes, so a textured material
// reaches it the way most textured scenes do: inside a glTF asset.  pine::load imports the .glb -- its PNG images become 8-bit
// images of the scene, its baseColorTexture / metallicRoughnessTexture become Texture(UV(), image) nodes -- and pine::Image
// reads a .png file (3 channels, as the reference loads it), here as the texels of an ImageSky.
//   g++ -std=c++17 -O2 examples/textured.cpp -Lpine_amd/lib -lpine_gpu -Wl,-rpath,$PWD/pine_amd/lib -o build/textured
//   build/textured tests/golden/textured_quad.glb [sky.png] [--describe | --texels]
#include <cstdio>
#include <cstring>

#include "../pine_amd/host/pine.hpp"

int main(int argc, char** argv) {
  using namespace pine;
  try {
    const char* glb = nullptr;
    const char* png = nullptr;
    bool describe = false, texels = false;
    for (int i = 1; i < argc; i++) {
      if (!strcmp(argv[i], "--describe")) describe = true;
      else if (!strcmp(argv[i], "--texels")) texels = true;
      else if (!glb) glb = argv[i];
      else png = argv[i];
    }
    if (!glb) throw Error("usage: textured scene.glb [sky.png] [--describe | --texels]");
    Scene scene;
    load(scene, glb);
    ImagePtr sky;
    if (png) {
      sky = std::make_shared<Image>(std::string(png));
      scene.set(ImageSky(sky, vec3(0.5f, 0.5f, 0.5f)));
    }
    if (texels) {  // the bytes pine::Image read
      if (!sky) throw Error("--texels needs a .png file");
      printf("%d %d\n", sky->size.x, sky->size.y);
      for (uint8_t v : sky->u8) printf("%02x", unsigned(v));
      printf("\n");
      return 0;
    }
    if (describe) {
      printf("%s", scene.describe().c_str());
      return 0;
    }
    PathIntegrator(BlueSampler(4), 3).render(scene);
    const Film& film = scene.camera.film();
    FILE* out = fopen("textured.f32", "wb");  // raw float32 RGBA, row 0 first
    if (!out || fwrite(film.pixels.data(), 4, film.pixels.size(), out) != film.pixels.size()) throw Error("cannot write textured.f32");
    fclose(out);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
