// pine_amd/csrc/pine_denoise.hip -- the denoising filter of pine_denoise.h as gfx950 kernels and as a host-thread build of the
// same per-pixel functions, and its entry points of the C ABI (include/pine_gpu.h: pine_gpu_denoise, pine_gpu_denoise_device).
// Built with the path kernels' flags (-ffp-contract=off): the two builds write the same bytes.
//
// Kernels: one launch packs the guides and demodulates, then one launch per iteration; the last one remodulates into the
// output.  A workgroup is 64 x 4 pixels, a wave one row segment of 64: every tap of a wave is a coalesced run of 16-byte
// words.  Direct global loads -- the 25 taps of neighbouring pixels overlap in L1 / L2; no LDS, no atomics, no waits.
#include <hip/hip_runtime.h>

#include <cstring>

#include "pine_plan.h"
#include "pine_denoise_host.h"

namespace pine_gpu {

constexpr int kDenoiseBlockX = 64, kDenoiseBlockY = 4;

__global__ void __launch_bounds__(kBlock) denoise_prepare_kernel(DenoiseConsts C, const float4* __restrict__ film, const float* __restrict__ albedo,
                                                                 const float* __restrict__ normal, float4* __restrict__ g, float4* __restrict__ I0) {
  const size_t i = blockIdx.x * size_t(kBlock) + threadIdx.x;
  if (i < size_t(C.w) * size_t(C.h)) denoise_prepare_pixel(C, i, film, albedo, normal, g, I0);
}

// (no __restrict__ on film / out: the last iteration may write the film it reads)
template <bool LAST>
__global__ void __launch_bounds__(kBlock) denoise_iterate_kernel(DenoiseConsts C, int step, float sigma_color_sq, const float4* __restrict__ g,
                                                                 const float4* __restrict__ in, const float4* film, float4* out) {
  const int x = int(blockIdx.x) * kDenoiseBlockX + int(threadIdx.x), y = int(blockIdx.y) * kDenoiseBlockY + int(threadIdx.y);
  if (x < C.w && y < C.h) denoise_iterate_pixel<LAST>(C, x, y, step, sigma_color_sq, g, in, film, out);
}

// The launches on `stream`: the guides packed and the colour demodulated, the iterations between the two colour buffers, the
// last one into `out` (which may be `film`).  The buffers are the caller's and must outlive the launches.
static int denoise_launch(const pine_gpu_denoise_params* prm, const DenoiseConsts& C, const float4* film, const float* albedo, const float* normal,
                          float4* out, float4* g, float4* a, float4* b, hipStream_t stream) {
  const size_t n = size_t(C.w) * size_t(C.h);
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, C, film, albedo, normal, g, a);
  const dim3 grid(unsigned((C.w + kDenoiseBlockX - 1) / kDenoiseBlockX), unsigned((C.h + kDenoiseBlockY - 1) / kDenoiseBlockY)),
      block(kDenoiseBlockX, kDenoiseBlockY);
  float4 *src = a, *dst = b;
  for (int it = 0; it < prm->iterations; it++) {
    const float sc = denoise_sigma_color_sq(prm->sigma_color, it);
    if (it + 1 == prm->iterations) {
      hipLaunchKernelGGL(denoise_iterate_kernel<true>, grid, block, 0, stream, C, 1 << it, sc, (const float4*)g, (const float4*)src, film, out);
    } else {
      hipLaunchKernelGGL(denoise_iterate_kernel<false>, grid, block, 0, stream, C, 1 << it, sc, (const float4*)g, (const float4*)src, film, dst);
    }
    std::swap(src, dst);
  }
  return hip_launch_check("denoise: kernel launch");
}

static int denoise_device(const pine_gpu_denoise_params* prm, const DenoiseConsts& C, const void* film, const void* albedo, const void* normal,
                          void* out, hipStream_t stream) {
  const size_t n = size_t(C.w) * size_t(C.h);
  if (prm->iterations == 0) {
    if (out != film) HIP_OK(hipMemcpyAsync(out, film, n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
    return 0;
  }
  const char* const what = "denoise: the work buffers";
  DeviceBuffer<float4> g(kFromPool), a(kFromPool), b(kFromPool);
  if (g.alloc(2 * n, what) || a.alloc(n, what) || (prm->iterations > 1 && b.alloc(n, what))) return -1;
  const int rc = denoise_launch(prm, C, static_cast<const float4*>(film), static_cast<const float*>(albedo), static_cast<const float*>(normal),
                                static_cast<float4*>(out), g, a, b, stream);
  // the work buffers go back to the pool when this returns: the launches that use them must have finished
  const hipError_t e = hipStreamSynchronize(stream);
  if (rc) return rc;
  return e == hipSuccess ? 0 : hip_error("denoise", e);
}

}  // namespace pine_gpu

extern "C" {

void pine_gpu_denoise_params_default(pine_gpu_denoise_params* prm) {
  if (!prm) return;
  prm->iterations = 5;
  prm->normal_power_log2 = 7;
  prm->sigma_color = PINE_GPU_DENOISE_SIGMA_COLOR;
  prm->sigma_albedo = PINE_GPU_DENOISE_SIGMA_ALBEDO;
  prm->eps_albedo = PINE_GPU_DENOISE_EPS_ALBEDO;
  prm->device = 0;
}

int pine_gpu_denoise(const pine_gpu_denoise_params* prm, int w, int h, const float* film, const float* albedo, const float* normal, float* out) {
  DenoiseConsts C;
  if (denoise_check(prm, w, h, C)) return -1;
  if (!film || !albedo || !normal || !out) {
    set_error("null argument");
    return -1;
  }
  if (prm->device < 0) return denoise_host(prm, C, film, albedo, normal, out);  // (pine_denoise_host.h)
  if (need_device(prm->device)) return -1;
  const size_t n = size_t(w) * size_t(h);
  const char* const what = "denoise: the film and the guides";
  DeviceBuffer<float> d_film(kFromPool), d_albedo(kFromPool), d_normal(kFromPool);
  if (d_film.upload(film, 4 * n, what) || d_albedo.upload(albedo, 3 * n, what) || d_normal.upload(normal, 3 * n, what)) return -1;
  if (denoise_device(prm, C, d_film, d_albedo, d_normal, d_film, nullptr)) return -1;
  return d_film.download(out, 4 * n, "denoise: film download");
}

int pine_gpu_denoise_device(const pine_gpu_denoise_params* prm, int w, int h, const void* film_dev, const void* albedo_dev, const void* normal_dev,
                            void* out_dev, void* stream) {
  DenoiseConsts C;
  if (denoise_check(prm, w, h, C)) return -1;
  if (!film_dev || !albedo_dev || !normal_dev || !out_dev) {
    set_error("null argument");
    return -1;
  }
  if (prm->device < 0) {
    set_error("pine_gpu_denoise_device: device memory needs a device (device >= 0); the host build is pine_gpu_denoise with device = -1");
    return -1;
  }
  if (need_device(prm->device)) return -1;
  return denoise_device(prm, C, film_dev, albedo_dev, normal_dev, out_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
