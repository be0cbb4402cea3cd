// pine_amd/csrc/pine_atmosphere.h -- atmosphere_color (src/pine/core/color.cpp:41-98), the single-scattering Rayleigh / Mie
// sky of the reference's Atmosphere light (light.cpp:94-125), for the kernels and -- this header needs pine_math.h alone --
// for a plain C++ build of the host code.  Every operation in the reference's order, one rounding each; exp and pow are
// the glibc-exact pexp and ppow.  Its quirks are the reference's: the light step's "height" is a squared length minus a
// radius (so the planet never shadows the sun and a sun below the horizon still lights the sky), the view loop ends at
// height <= 0, and the sun-disc test takes dot(direction, sun_dir) as it is.
#pragma once
#include "pine_math.h"

namespace pine_gpu {

constexpr int kAtmosphereSamples = 8;  // Atmosphere passes kViewSteps = 8 everywhere (light.cpp:102, 107, 117)

// The integral is a function of its own in device code, not inlined: inlined into the path kernels' miss branch it raised the
// VGPR spills of every F_LIGHTS variant of the stage-queued kernel (profiles/atmosphere_regs.txt).
#if defined(__HIP_DEVICE_COMPILE__)
#define PINE_ATMOSPHERE_HD __host__ __device__ __noinline__ inline
#else
#define PINE_ATMOSPHERE_HD PINE_HD
#endif
PINE_ATMOSPHERE_HD f3 atmosphere_color_of(f3 direction, f3 sun_dir, bool real_sun) {
  const f3 beta_r{3.8e-6f, 13.5e-6f, 33.1e-6f}, beta_m{21e-6f, 21e-6f, 21e-6f};
  const float r_atmosphere = 6420e3f, r_planet = 6360e3f;
  const float inv_scale_r = 1.0f / 7995.0f, inv_scale_m = 1.0f / 1200.0f;
  constexpr int kViewSteps = kAtmosphereSamples, kSunSteps = kViewSteps / 2;
  const float mu = dot(direction, sun_dir);
  const float g = 0.76f;
  const float phase_r = 3.0f / (16.0f * kPi) * (1.0f + mu * mu);
  const float phase_m = 3.0f / (8.0f * kPi) * (1.0f - g * g) * (1.0f + mu * mu) / ((2.0f + g * g) * ppow(1.0f + g * g - 2.0f * g * mu, 1.5f));

  const f3 o{0.0f, r_planet, 0.0f};
  const float tmax = sphere_compute_t(o, direction, 0.0f, f3{0.0f, 0.0f, 0.0f}, r_atmosphere);
  const float step = tmax / float(kViewSteps);
  float t = 0.0f;
  float depth_r = 0.0f, depth_m = 0.0f;
  f3 sum_r{0.0f, 0.0f, 0.0f}, sum_m{0.0f, 0.0f, 0.0f};

  for (int i = 0; i < kViewSteps; i++) {
    const f3 pos = o + (t + step * 0.5f) * direction;
    const float height = length(pos) - r_planet;
    if (height <= 0) break;
    const float w_r = pexp(-height * inv_scale_r) * step, w_m = pexp(-height * inv_scale_m) * step;
    depth_r += w_r;
    depth_m += w_m;

    const float sun_tmax = sphere_compute_t(pos, sun_dir, 0.0f, f3{0.0f, 0.0f, 0.0f}, r_atmosphere);
    const float sun_step = sun_tmax / float(kSunSteps);
    float depth_r_sun = 0.0f, depth_m_sun = 0.0f;

    int j = 0;
    const float pos_pos = dot(pos, pos);
    const float sun_sun = dot(sun_dir, sun_dir);
    const float pos_sun = dot(pos, sun_dir);
    float s = sun_step * 0.5f;
    for (; j < kSunSteps; j++, s += sun_step) {
      const float sun_height = pos_pos + sqr(s) * sun_sun + 2 * s * pos_sun - r_planet;
      if (sun_height < 0) break;
      depth_r_sun += pexp(-sun_height * inv_scale_r) * sun_step;
      depth_m_sun += pexp(-sun_height * inv_scale_m) * sun_step;
    }
    if (j == kSunSteps) {
      const f3 tau = beta_r * (depth_r + depth_r_sun) + beta_m * (depth_m + depth_m_sun);
      const f3 transmittance{pexp(-tau.x), pexp(-tau.y), pexp(-tau.z)};
      sum_r = sum_r + transmittance * w_r;
      sum_m = sum_m + transmittance * w_m;
    }
    t += step;
  }

  const f3 color = sum_r * beta_r * phase_r + sum_m * beta_m * phase_m;
  f3 scale{5.0f, 5.0f, 5.0f};
  if (real_sun && dot(direction, sun_dir) > 0.998f) scale = scale * (1000.0f * f3{1.0f, 0.9f, 0.8f});
  return color * scale;
}

// The direction of grid point (x, y) of a w x h image: ic2sc (light.cpp:90-92), uniform_sphere, y and z swapped
// (Atmosphere's constructor and sample(), light.cpp:99-101, 112-114).  x = w and y = h are grid points too.
PINE_HD f3 atmosphere_texel_direction(int x, int y, int w, int h) {
  const f3 d = uniform_sphere(f2{float(x) / float(w), float(y) / float(h)});
  return f3{d.x, d.z, d.y};
}
// One entry of the Atmosphere tables: the colour with the sun disc at grid point (x, y) of the (w + 1) x (h + 1) grid, and
// for a texel (x < w, y < h) its density, the colour's length (light.cpp:102).
PINE_HD void atmosphere_table_entry(int x, int y, int w, int h, f3 sun_dir, float* colors, float* density) {
  const f3 c = atmosphere_color_of(atmosphere_texel_direction(x, y, w, h), sun_dir, true);
  float* o = colors + (size_t(x) + size_t(y) * size_t(w + 1)) * 3;
  o[0] = c.x, o[1] = c.y, o[2] = c.z;
  if (x < w && y < h) density[size_t(x) + size_t(y) * size_t(w)] = length(c);
}

}  // namespace pine_gpu
