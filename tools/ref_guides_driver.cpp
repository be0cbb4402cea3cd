// tools/ref_guides_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_denoise.py; no test runs it).
//
// Our own driver around the REAL reference's DenoiseIntegrator.  It is compiled where the reference's sources lie, together with
// the reference's impl/integrator/denoiser.cpp read from its own place, and linked with oracle/_ref/libpine_ref.a; the binary goes
// to a scratch directory.  The scene is built from a .pscene exactly as oracle/ref_driver.cpp builds it (that file -- this
// repository's own -- is included for its loader), then DenoiseIntegrator(BVH(), SobolSampler(1), LightSampler()).render(scene).
//
// The reference's denoise() (src/pine/core/denoise.h) was Open Image Denoise, a library this build of it does not have: the
// function is the reference's own hook for it, and this driver DEFINES it -- its definition writes the albedo and normal arrays
// DenoiseIntegrator::render hands over to files (the archive's member with the empty definition is then not linked: nothing
// else asks for it).  The guide images are therefore the real reference's, not a restatement.
//
//   ref_guides_driver <scene.pscene> <out.albedo> <out.normal>
//     out.albedo, out.normal   raw vec3 images, W * H * 12 bytes, film row order
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/denoise.h>
#include <pine/impl/integrator/denoiser.h>

static const char* g_albedo_path = nullptr;
static const char* g_normal_path = nullptr;
static int g_denoise_calls = 0;

namespace pine {
void denoise(DenoiseQuality, Array2d<vec3>& output, const Array2d<vec3>& color, const Array2d<vec3>* albedo, const Array2d<vec3>* normal) {
  static_assert(sizeof(vec3) == 12, "vec3 is three floats");
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

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: ref_guides_driver <scene.pscene> <out.albedo> <out.normal>\n");
    return 2;
  }
  Loaded L;
  load_pscene(argv[1], L);
  g_albedo_path = argv[2], g_normal_path = argv[3];
  L.scene.camera.film().clear();
  auto integ = DenoiseIntegrator(Accel(BVH()), Sampler(SobolSampler(1)), LightSampler(UniformLightSampler()));
  integ.render(L.scene);
  if (g_denoise_calls != 1) {
    fprintf(stderr, "DenoiseIntegrator::render did not reach this driver's denoise()\n");
    return 3;
  }
  return 0;
}
