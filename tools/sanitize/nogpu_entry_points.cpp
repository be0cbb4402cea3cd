// tools/sanitize/nogpu_entry_points.cpp -- SANITIZER BUILD ONLY (tools/sanitize/Makefile), never part of the product.
//
// The host side of libpine_gpu.so (pine_amd/csrc/pine_host.cpp: scene building, shape constructors, BVH build,
// node folding, .pscene dump, film finalize, the host-only test hooks) is plain C++ and is what parses caller-supplied
// data; the CPU leg of the test-suite exercises exactly that code.  GPU AddressSanitizer is not available on this pool,
// so the sanitizer build compiles pine_host.cpp with g++ -fsanitize=address,undefined and takes the device-side entry
// points (pine_amd/csrc/pine_kernels.hip, pine_test_hooks.hip) from here: every one of them fails the way the real
// library fails on a host without a HIP device.  Nothing is rendered by this build.
#include <cstdint>
#include <string>

#include "../../include/pine_gpu.h"
#include "../../pine_amd/csrc/pine_host.h"
#include "../../pine_amd/csrc/pine_math_check.h"
#include "../../pine_amd/csrc/pine_denoise_host.h"

#include "../../pine_amd/csrc/pine_specialize.h"

// (the structure sizes a run-time compiled kernel is checked against come from the device half of the library: none here --
//  a kernel compiled through this build's pine_gpu_test_specialize_compile fails its static_assert, as it should)
pine_gpu::AbiFingerprint pine_gpu::abi_fingerprint() { return pine_gpu::AbiFingerprint{}; }

using pine_gpu::set_error;
static const char* const kNoDevice =
    "no HIP device available: the PathIntegrator hot path requires an AMD GPU (no CPU fallback) [sanitizer build: host code only]";
static int fail() {
  set_error(kNoDevice);
  return -1;
}
// (the Atmosphere tables on a device: pine_kernels.hip; the host build of them, device = -1, is the real thing in pine_host.cpp)
int pine_gpu::atmosphere_table_device(int, const float*, int, int, float*, float*) { return fail(); }

extern "C" {
float pine_gpu_progress(void) { return 0.0f; }
void pine_gpu_release_cached_memory(void) {}
int pine_gpu_set_table_path(const char* path) { return path ? 0 : fail(); }
int pine_gpu_path_render(pine_gpu_scene*, const pine_gpu_render_params*, float*) { return fail(); }
int pine_gpu_path_render_multi(pine_gpu_scene*, const pine_gpu_render_params*, uint64_t, float*) { return fail(); }
int pine_gpu_path_render_devices(pine_gpu_scene*, const pine_gpu_render_params*, const int*, int, float*) { return fail(); }
int pine_gpu_ao_render(pine_gpu_scene*, const pine_gpu_render_params*, float*) { return fail(); }
pine_gpu_plan* pine_gpu_ao_plan_create(pine_gpu_scene*, const pine_gpu_render_params*) {
  fail();
  return nullptr;
}
pine_gpu_plan* pine_gpu_plan_create(pine_gpu_scene*, const pine_gpu_render_params*) {
  fail();
  return nullptr;
}
pine_gpu_plan* pine_gpu_plan_create_passes(pine_gpu_scene*, const pine_gpu_render_params*, int32_t) {
  fail();
  return nullptr;
}
int pine_gpu_guides_render(pine_gpu_scene*, const pine_gpu_render_params*, float*, float*) { return fail(); }
int pine_gpu_guides_render_device(pine_gpu_scene*, const pine_gpu_render_params*, void*, void*, void*) { return fail(); }
int pine_gpu_guides_variants(uint32_t*, int) { return fail(); }
pine_gpu_accel* pine_gpu_accel_create(pine_gpu_scene*, int, uint32_t) {
  fail();
  return nullptr;
}
void pine_gpu_accel_destroy(pine_gpu_accel*) {}
int pine_gpu_accel_intersect_device(pine_gpu_accel*, const void*, int64_t, void*, void*) { return fail(); }
int pine_gpu_accel_hit_device(pine_gpu_accel*, const void*, int64_t, void*, void*) { return fail(); }
int pine_gpu_accel_intersect(pine_gpu_accel*, const float*, int64_t, void*) { return fail(); }
int pine_gpu_accel_hit(pine_gpu_accel*, const float*, int64_t, uint8_t*) { return fail(); }
int pine_gpu_accel_camera_rays_device(pine_gpu_accel*, void*, void*) { return fail(); }
int pine_gpu_accel_info(pine_gpu_accel*, int32_t*) { return fail(); }
pine_gpu_shader* pine_gpu_shader_create(pine_gpu_scene*, const pine_gpu_render_params*) {
  fail();
  return nullptr;
}
void pine_gpu_shader_destroy(pine_gpu_shader*) {}
int pine_gpu_shader_layout(int32_t*) { return fail(); }
int pine_gpu_shader_info(pine_gpu_shader*, int32_t*) { return fail(); }
int pine_gpu_shader_begin_device(pine_gpu_shader*, int, void*, void*, void*) { return fail(); }
int pine_gpu_shader_vertex_device(pine_gpu_shader*, const void*, const void*, int64_t, void*, void*, void*, void*, void*) { return fail(); }
int pine_gpu_shader_fold_device(pine_gpu_shader*, const void*, const void*, int, int64_t, int, void*, void*, void*) { return fail(); }
int pine_gpu_shader_resolve_device(pine_gpu_shader*, const void*, int64_t, void*, void*) { return fail(); }
// (the filter's host-thread build, device = -1, is the real thing: pine_denoise_host.h)
void pine_gpu_denoise_params_default(pine_gpu_denoise_params* prm) {
  if (prm) *prm = pine_gpu_denoise_params{5, 7, PINE_GPU_DENOISE_SIGMA_COLOR, PINE_GPU_DENOISE_SIGMA_ALBEDO, PINE_GPU_DENOISE_EPS_ALBEDO, 0};
}
int pine_gpu_denoise(const pine_gpu_denoise_params* prm, int w, int h, const float* film, const float* albedo, const float* normal, float* out) {
  pine_gpu::DenoiseConsts C;
  if (pine_gpu::denoise_check(prm, w, h, C)) return -1;
  if (!film || !albedo || !normal || !out || prm->device >= 0) return fail();
  return pine_gpu::denoise_host(prm, C, film, albedo, normal, out);
}
int pine_gpu_denoise_device(const pine_gpu_denoise_params*, int, int, const void*, const void*, const void*, void*, void*) { return fail(); }
int pine_gpu_plan_pass_count(pine_gpu_plan*) { return fail(); }
int pine_gpu_plan_pass_info(pine_gpu_plan*, int, int32_t*) { return fail(); }
int pine_gpu_plan_launch_pass(pine_gpu_plan*, int, void*, void*) { return fail(); }
int pine_gpu_plan_tile_order(pine_gpu_plan*, int32_t*, int) { return fail(); }
int pine_gpu_plan_device_bytes(pine_gpu_plan*, int64_t*) { return fail(); }
int pine_gpu_path_render_passes(pine_gpu_scene*, const pine_gpu_render_params*, int32_t, float*, pine_gpu_pass_callback, void*) { return fail(); }
int pine_gpu_plan_launch(pine_gpu_plan*, void*, void*) { return fail(); }
int pine_gpu_plan_launch_packed(pine_gpu_plan*, void*, void*) { return fail(); }
void pine_gpu_plan_destroy(pine_gpu_plan*) {}
int pine_gpu_plan_stats_get(pine_gpu_plan*, pine_gpu_plan_stats*) { return fail(); }
int pine_gpu_plan_check(pine_gpu_plan*) { return fail(); }
int pine_gpu_plan_debug_sections(pine_gpu_plan*, uint64_t*) { return fail(); }
int pine_gpu_plan_read_samples(pine_gpu_plan*, float*, int64_t) { return fail(); }
int64_t pine_gpu_plan_vertex_log(pine_gpu_plan*, float*, int64_t) { return fail(); }
int pine_gpu_film_unpack(int, int, int, int, const void*, void*, void*) { return fail(); }
int pine_gpu_test_sampler(int, int, float*, int64_t) { return fail(); }
int pine_gpu_test_rng(int, uint64_t*, int64_t) { return fail(); }
int64_t pine_gpu_test_sampler_draws(int, int, int, int, int, int, const int32_t*, int64_t, float*, int64_t) { return fail(); }
int pine_gpu_test_halton_tables(uint32_t*, int64_t*) { return fail(); }
int pine_gpu_test_sincos(int, const float*, int64_t, float*, float*) { return fail(); }
int pine_gpu_test_powlog(int, const float*, const float*, int64_t, float*, float*) { return fail(); }
int pine_gpu_test_atan(int, const float*, const float*, int64_t, float*, float*) { return fail(); }
int pine_gpu_test_traverse(pine_gpu_scene*, int, const float*, int64_t, int, int, uint32_t*) { return fail(); }
// (the host halves are the real thing, pine_math_check.h: the comparison, the references, the host build of the functions)
int pine_gpu_test_math_eval(int device, int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n, uint32_t* got) {
  return device < 0 ? pine_gpu::math_check::eval_host_arrays(fn, a, b, c, n, got) : fail();
}
int pine_gpu_test_math_sweep(int device, int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count, uint32_t stride,
                             int64_t* stats, uint32_t* examples, int cap) {
  return device < 0 ? pine_gpu::math_check::sweep_host(fn, fixed_bits, swept_arg, first, count, stride, stats, examples, cap)
                    : fail();
}
int pine_gpu_test_shapes(pine_gpu_scene*, int, const float*, int64_t, float*, int64_t) { return fail(); }
int pine_gpu_test_bxdf(int, const float*, int64_t, float*) { return fail(); }
int pine_gpu_test_light_samples(pine_gpu_scene*, int, const float*, int64_t, float*) { return fail(); }
int pine_gpu_test_env_light(pine_gpu_scene*, int, const float*, int64_t, float*) { return fail(); }
int64_t pine_gpu_test_env_tree(pine_gpu_scene*, int32_t*, int64_t) { return fail(); }
int pine_gpu_test_atmosphere_color(int, const float*, int64_t, float*) { return fail(); }
int64_t pine_gpu_test_env_table(pine_gpu_scene*, float*, int64_t) { return fail(); }
int pine_gpu_test_env_light_sample(pine_gpu_scene*, int, const float*, int64_t, float*) { return fail(); }
int64_t pine_gpu_test_node_programs(pine_gpu_scene*, int32_t*, int64_t) { return fail(); }
int64_t pine_gpu_test_tex_words(pine_gpu_scene*) { return fail(); }
int pine_gpu_test_material_params(pine_gpu_scene*, int, const float*, int64_t, float*) { return fail(); }
int pine_gpu_test_choose_lobe(pine_gpu_scene*, int, const float*, int64_t, float*) { return fail(); }
int pine_gpu_plan_test_traverse_baked(pine_gpu_plan*, const float*, int64_t, uint32_t*) { return fail(); }
int pine_gpu_test_kernel_variants(int, uint32_t*, int32_t*, int32_t*, int) { return fail(); }
int pine_gpu_test_box_slabs(const float*, const float*, int64_t, uint32_t*) { return fail(); }
int pine_gpu_test_short_div(int, int, int, const uint32_t*, uint32_t, uint32_t, uint32_t, int64_t, int64_t*, uint32_t*, int) { return fail(); }
int pine_gpu_test_live_device_blocks(int64_t*) { return fail(); }
int pine_gpu_test_poison_stats(int64_t*) { return fail(); }
int pine_gpu_test_poison_probe(int, int, int64_t, uint32_t*) { return fail(); }
int64_t pine_gpu_test_frame_table(pine_gpu_scene*, pine_gpu_plan*, int, float*, float*, int64_t, int32_t*, int64_t, const float*, int64_t, int32_t*) {
  return fail();
}
}
