// pine_amd/csrc/pine_denoise_host.h -- the host side of the denoising filter that needs no device: the parameter check and the
// host-thread build of pine_denoise.h's per-pixel functions (pine_gpu_denoise with device = -1).  Plain C++: included by
// pine_denoise.hip, the product, and by the sanitizer build of the host code (tools/sanitize), which has no device half.
#pragma once
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/pine_gpu.h"
#include "pine_host.h"
#include "pine_math_check.h"
#include "pine_denoise.h"

namespace pine_gpu {

inline int denoise_check(const pine_gpu_denoise_params* prm, int w, int h, DenoiseConsts& C) {
  if (!prm) {
    set_error("null argument");
    return -1;
  }
  if (w < 1 || h < 1 || w > 65535 || h > 65535) {
    set_error("denoise: film sides are 1 ... 65535");
    return -1;
  }
  if (prm->iterations < 0 || prm->iterations > kDenoiseMaxIterations) {
    set_error("denoise: iterations are 0 ... 8");
    return -1;
  }
  if (prm->normal_power_log2 < 0 || prm->normal_power_log2 > 16) {
    set_error("denoise: normal_power_log2 is 0 ... 16");
    return -1;
  }
  // (the smallest colour sigma, sigma_color / 2^8, must still have a normal square)
  auto ok = [](float s) { return s >= 1e-12f && s <= 1e12f; };
  if (!ok(prm->sigma_color) || !ok(prm->sigma_albedo) || !ok(prm->eps_albedo)) {
    set_error("denoise: sigma_color, sigma_albedo and eps_albedo lie in [1e-12, 1e12]");
    return -1;
  }
  C.w = w, C.h = h;
  C.normal_power_log2 = prm->normal_power_log2;
  C.sigma_albedo_sq = prm->sigma_albedo * prm->sigma_albedo;
  C.eps_albedo = prm->eps_albedo;
  return 0;
}

// The host-thread build: rows dealt out in contiguous ranges, every pixel by the function the kernels run.
template <class F>
inline void denoise_host_rows(int h, F f) {
  const int nt = std::max(1, std::min(math_check::threads(), h));
  if (nt == 1) {
    f(0, h);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { f(int(int64_t(h) * t / nt), int(int64_t(h) * (t + 1) / nt)); });
  for (auto& t : th) t.join();
}

inline int denoise_host(const pine_gpu_denoise_params* prm, const DenoiseConsts& C, const float* film_, const float* albedo, const float* normal,
                        float* out_) {
  const size_t n = size_t(C.w) * size_t(C.h);
  const float4* film = reinterpret_cast<const float4*>(film_);
  float4* out = reinterpret_cast<float4*>(out_);
  if (prm->iterations == 0) {
    if (out_ != film_) memmove(out_, film_, n * sizeof(float4));
    return 0;
  }
  std::vector<float4> g(2 * n), a(n), b(prm->iterations > 1 ? n : 0);
  denoise_host_rows(C.h, [&](int y0, int y1) {
    for (size_t i = size_t(y0) * C.w; i < size_t(y1) * C.w; i++) denoise_prepare_pixel(C, i, film, albedo, normal, g.data(), a.data());
  });
  float4 *src = a.data(), *dst = b.data();
  for (int it = 0; it < prm->iterations; it++) {
    const bool last = it + 1 == prm->iterations;
    const float sc = denoise_sigma_color_sq(prm->sigma_color, it);
    denoise_host_rows(C.h, [&](int y0, int y1) {
      for (int y = y0; y < y1; y++)
        for (int x = 0; x < C.w; x++) {
          if (last) denoise_iterate_pixel<true>(C, x, y, 1 << it, sc, g.data(), src, film, out);
          else denoise_iterate_pixel<false>(C, x, y, 1 << it, sc, g.data(), src, film, dst);
        }
    });
    std::swap(src, dst);
  }
  return 0;
}

}  // namespace pine_gpu
