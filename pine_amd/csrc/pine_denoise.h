// pine_amd/csrc/pine_denoise.h -- the filter behind DenoiseIntegrator: an a-trous edge-avoiding wavelet filter (Dammertz,
// Sewtz, Hanika, Lensch 2010) on albedo-demodulated colour, guided by the albedo and normal images of pine_guides_kernel.h.
// The reference has the interface (src/pine/core/denoise.h) and the guide pass (impl/integrator/denoiser.cpp) but no filter
// of its own: its denoise() was Open Image Denoise.  So there is nothing to equal bit for bit but OURSELVES: the per-pixel
// functions below are PINE_HD, compiled without FP contraction, and run by the gfx950 kernels and by host threads
// (pine_denoise.hip) -- the same bytes either way.
//
// Definition.  Film F (rgba), albedo A, normal N; hit(p) = N(p) != (0, 0, 0).
//   D(p)      = max(A(p), eps_a) per component;  I_0(p) = F.rgb(p) / D(p)
//   I_{i+1}(p) = sum_q h(q) w(p, q) I_i(q) / sum_q h(q) w(p, q),  i = 0 .. n-1, step s = 2^i, over the 25 taps
//               q = p + s (dx, dy), dx, dy in -2 .. 2, that lie inside the film and have hit(q); dy outer, dx inner, the
//               sums sequential in fp32; h = the outer product of [1/16, 1/4, 3/8, 1/4, 1/16]
//   w         = (w_n * w_a) * w_c;  the centre tap's w is exactly 1
//   w_n       = max(0, N(p) . N(q)) squared k times (k = 7: the power 128; no powf)
//   w_a       = expf_glibc(-|A(p) - A(q)|^2 / sigma_a^2)
//   w_c       = expf_glibc(-|I_i(p) - I_i(q)|^2 / (sigma_c 2^-i)^2)
//   out.rgb   = I_n D, out.a = F.a;  a pixel with !hit(p) is copied through and contributes to no other pixel;
//               n = 0 is the identity.
// Storage: the guides packed once into two float4 per pixel -- (A, hit as 1 or 0) and (N, 0) -- and I_i as one float4 (w unused):
// a tap is three 16-byte loads.
#pragma once
#include "pine_math.h"

#if !defined(__HIPCC__)  // (a host-only build, tools/sanitize: HIP's float4 without HIP)
struct float4 {
  float x, y, z, w;
};
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
#endif

namespace pine_gpu {

constexpr int kDenoiseMaxIterations = 8;

struct DenoiseConsts {
  int w, h;
  int normal_power_log2;
  float sigma_albedo_sq;  // sigma_a * sigma_a
  float eps_albedo;
};

// (sigma_c 2^-i)^2: the halvings are exact, the square is one rounding
inline float denoise_sigma_color_sq(float sigma_color, int iteration) {
  float s = sigma_color;
  for (int j = 0; j < iteration; j++) s = s * 0.5f;
  return s * s;
}

PINE_HD float denoise_kernel_weight(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
PINE_HD float denoise_dist_sq(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}
PINE_HD float denoise_demod(float a, float eps) { return pmax(a, eps); }

// Pack the guides of pixel i and demodulate its colour: g[2 i], g[2 i + 1], I_0[i].
PINE_HD void denoise_prepare_pixel(const DenoiseConsts& C, size_t i, const float4* film, const float* albedo, const float* normal, float4* g, float4* I0) {
  const float ax = albedo[3 * i], ay = albedo[3 * i + 1], az = albedo[3 * i + 2];
  const float nx = normal[3 * i], ny = normal[3 * i + 1], nz = normal[3 * i + 2];
  const bool hit = nx != 0.0f || ny != 0.0f || nz != 0.0f;
  g[2 * i] = make_float4(ax, ay, az, hit ? 1.0f : 0.0f);
  g[2 * i + 1] = make_float4(nx, ny, nz, 0.0f);
  const float4 f = film[i];
  I0[i] = make_float4(f.x / denoise_demod(ax, C.eps_albedo), f.y / denoise_demod(ay, C.eps_albedo), f.z / denoise_demod(az, C.eps_albedo), 0.0f);
}

// One iteration at pixel (x, y): I_{i+1}(p) from I_i = `in`.  LAST: the result goes out remodulated, with the film's alpha -- and
// a pixel that is no hit as the film has it (`film` may be `out`: a pixel reads its own film value only, before it writes).
template <bool LAST>
PINE_HD void denoise_iterate_pixel(const DenoiseConsts& C, int x, int y, int step, float sigma_color_sq, const float4* g, const float4* in,
                                   const float4* film, float4* out) {
  const size_t p = size_t(y) * size_t(C.w) + size_t(x);
  const float4 ga = g[2 * p];
  if (ga.w == 0.0f) {
    if (LAST) out[p] = film[p];
    return;
  }
  const float4 gn = g[2 * p + 1];
  const float4 ip = in[p];
  float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + dy * step;
    if (qy < 0 || qy >= C.h) continue;
    const float hy = denoise_kernel_weight(dy);
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + dx * step;
      if (qx < 0 || qx >= C.w) continue;
      const size_t q = size_t(qy) * size_t(C.w) + size_t(qx);
      const float4 qa = g[2 * q];
      if (qa.w == 0.0f) continue;
      const float4 iq = in[q];
      float wgt = 1.0f;
      if (dx != 0 || dy != 0) {
        const float4 qn = g[2 * q + 1];
        float wn = pmax(0.0f, (gn.x * qn.x + gn.y * qn.y) + gn.z * qn.z);
        for (int k = 0; k < C.normal_power_log2; k++) wn = wn * wn;
        const float wa = pine_libm::expf_glibc(-denoise_dist_sq(ga.x, ga.y, ga.z, qa.x, qa.y, qa.z) / C.sigma_albedo_sq);
        const float wc = pine_libm::expf_glibc(-denoise_dist_sq(ip.x, ip.y, ip.z, iq.x, iq.y, iq.z) / sigma_color_sq);
        wgt = (wn * wa) * wc;
      }
      const float c = (denoise_kernel_weight(dx) * hy) * wgt;
      sr = sr + c * iq.x;
      sg = sg + c * iq.y;
      sb = sb + c * iq.z;
      sw = sw + c;
    }
  }
  const float r = sr / sw, gg = sg / sw, b = sb / sw;
  if (LAST) {
    out[p] = make_float4(r * denoise_demod(ga.x, C.eps_albedo), gg * denoise_demod(ga.y, C.eps_albedo), b * denoise_demod(ga.z, C.eps_albedo), film[p].w);
  } else {
    out[p] = make_float4(r, gg, b, 0.0f);
  }
}

}  // namespace pine_gpu
