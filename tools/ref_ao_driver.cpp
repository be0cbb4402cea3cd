// tools/ref_ao_driver.cpp -- FIXTURE GENERATION ONLY (tools/make_golden_ao.py; no test runs it).
//
// Our own driver around the REAL reference's AOIntegrator.  It is compiled where the reference's sources lie, together with
// the reference's impl/integrator/ao.cpp read from its own place, and linked with oracle/_ref/libpine_ref.a (which does not
// hold ao.cpp); the binary goes to a scratch directory.  Only the reference's public API is called: the scene is built from a
// .pscene exactly as oracle/ref_driver.cpp builds it (that file -- this repository's own -- is included for its loader),
// then AOIntegrator(BVH(), sampler).render, uniform_sphere, Scene::get_aabb, Sampler::spp.
//
//   ref_ao_driver <scene.pscene> <spp> <blue|sobol|halton> <out.film> <out.consts>
//     out.film    raw vec4 film, W * H * 16 bytes
//     out.consts  26 words: radius, directions[8] as xyz (floats), the integrator's sample count (int32)
#define main pine_ref_driver_main
#include "../oracle/ref_driver.cpp"
#undef main

#include <pine/core/sampling.h>
#include <pine/impl/integrator/ao.h>

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: ref_ao_driver <scene.pscene> <spp> <blue|sobol|halton> <out.film> <out.consts>\n");
    return 2;
  }
  Loaded L;
  load_pscene(argv[1], L);
  const int spp = atoi(argv[2]);
  const std::string kind = argv[3];
  auto make_sampler = [&]() {
    return kind == "sobol" ? Sampler(SobolSampler(spp)) : kind == "halton" ? Sampler(HaltonSampler(spp)) : Sampler(BlueSobolSampler(spp));
  };
  auto integ = AOIntegrator(Accel(BVH()), make_sampler());
  integ.render(L.scene);
  auto& film = L.scene.camera.film();
  write_file(argv[4], film.data(), size_t(16) * L.W * L.H);

  float consts[26];
  consts[0] = min_value(L.scene.get_aabb().diagonal()) / 2;
  const float pairs[8][2] = {{0.0f, 0.25f}, {0.25f, 0.25f}, {0.5f, 0.25f}, {0.75f, 0.25f}, {0.0f, 0.75f}, {0.25f, 0.75f}, {0.5f, 0.75f}, {0.75f, 0.75f}};
  for (int i = 0; i < 8; i++) {
    const vec3 d = uniform_sphere(vec2(pairs[i][0], pairs[i][1]));
    consts[1 + 3 * i] = d.x, consts[2 + 3 * i] = d.y, consts[3 + 3 * i] = d.z;
  }
  const int ao_spp = psl::max(make_sampler().spp() / 8, 1);
  memcpy(&consts[25], &ao_spp, 4);
  write_file(argv[5], consts, sizeof consts);
  return 0;
}
