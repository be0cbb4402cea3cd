// pine_amd/csrc/pine_noise.h -- NodeNoisef / NodeNoise3f (node.h:209-225, node.cpp:7-13): the reference's fbm(vec3, int) and
// fbm3d(vec3, int) (noise.cpp:29-41, 53-75, 84-86, 102-104; perlin_interp vecmath.h:1035-1045), written once: the kernels'
// node evaluator runs it per hit, the host folds a noise node whose operands do not read the surface with it, and the PRL
// front-end's fbm / fbm3d / pnoise / pnoise3d include it as plain C++.  It reads no memory.  It needs pine_math.h and
// pine_rng.h alone, so a plain build of the host code includes it.
//
// Arithmetic: binary32 in the reference's operand order, no contraction -- but for perlin_interp, whose corner weight is a
// binary64 expression (its `1.0` literals) and whose running sum is rounded to binary32 after every corner.
#pragma once
#include <limits.h>

#include "pine_math.h"
#include "pine_rng.h"

namespace pine_gpu {

constexpr int kNoiseMaxOctaves = 32;  // the device loop's bound
// The corner, channel and octave loops stay loops in the kernels: one copy of the body, no eight gradients live at once.
#if defined(__clang__)
#define PINE_KEEP_LOOP _Pragma("unroll 1")
#else
#define PINE_KEEP_LOOP
#endif

// float -> int as x86 converts (cvttss2si): truncation, INT_MIN for a NaN or a value outside [-2^31, 2^31).  The reference's
// conversion is undefined there; through this helper the host and the device builds agree everywhere.
PINE_HD int noise_float_to_int(float v) { return (v >= -0x1p31f && v < 0x1p31f) ? int(v) : INT_MIN; }
// The rounds fbm runs for a node's octaves value: its truncation to int (`fbm(p(ctx), octaves(ctx))`), bounded: below 1
// (-inf included) and NaN run none, above kNoiseMaxOctaves (+inf included) runs kNoiseMaxOctaves.
PINE_HD int noise_octaves(float v) {
  if (!(v >= 1.0f)) return 0;
  if (v >= float(kNoiseMaxOctaves)) return kNoiseMaxOctaves;
  return int(v);
}

// perlin_noise(vec3 np, int seed) noise.cpp:29-41 with perlin_interp folded into the corner loop: the corners are visited in
// perlin_interp's order (x, y, z; z innermost) and `ret` is accumulated in that order, so no gradient outlives its corner.
PINE_HD float perlin_noise3(f3 np, int seed) {
  const f3 fl{floorf(np.x), floorf(np.y), floorf(np.z)};
  f3 w = np - fl;
  w = f3{w.x * w.x * (3.0f - 2.0f * w.x), w.y * w.y * (3.0f - 2.0f * w.y), w.z * w.z * (3.0f - 2.0f * w.z)};
  float ret = 0;
  PINE_KEEP_LOOP
  for (int corner = 0; corner < 8; corner++) {
    const int x = corner >> 2, y = (corner >> 1) & 1, z = corner & 1;
    // vec3i(floor(np) + vec3i(x, y, z)): a float sum, then the conversion
    const uint64_t h = hash_cell(noise_float_to_int(fl.x + float(x)), noise_float_to_int(fl.y + float(y)),
                                 noise_float_to_int(fl.z + float(z)), seed);
    DRng g = rng_seed(h);
    const float ux = rng_nextf(g);  // next2f: x first
    const float uy = rng_nextf(g);
    // spherical_to_cartesian(u.x * Pi * 2, u.y * Pi)  vecmath.h:1197-1200
    float sin_phi, cos_phi, sin_theta, cos_theta;
    psincos(ux * kPi * 2, sin_phi, cos_phi);
    psincos(uy * kPi, sin_theta, cos_theta);
    const f3 c{sin_theta * cos_phi, sin_theta * sin_phi, cos_theta};
    // perlin_interp's term (vecmath.h:1040-1042): the difference from the SMOOTHED fraction, a binary32 dot, and the weight
    // in binary64 -- written as the reference writes it, so that every conversion is the language's own
    const f3 d{w.x - float(x), w.y - float(y), w.z - float(z)};
    const float dt = c.x * d.x + c.y * d.y + c.z * d.z;
    const double term = (x * w.x + (1 - x) * (1.0 - w.x)) * (y * w.y + (1 - y) * (1.0 - w.y)) * (z * w.z + (1 - z) * (1.0 - w.z)) * dt;
    ret = float(ret + term);
  }
  return 0.5f * (1.0f + ret);
}

// fbm(vec3, int) (`three` false: the value in every component) and fbm3d(vec3, int) (noise.cpp:63-75): channel k is
// perlin_noise(np, k), so fbm is channel 0 of fbm3d bit for bit, and the float form computes that channel alone.
// `octaves` is a count noise_octaves returned, or any int of a host caller: the loop is bounded here as well.
PINE_HD f3 noise_fbm(f3 np, int octaves, bool three) {
  f3 accum{0, 0, 0};
  float weight = 1.0f;
  const int rounds = octaves < kNoiseMaxOctaves ? octaves : kNoiseMaxOctaves;
  const int channels = three ? 3 : 1;
  PINE_KEEP_LOOP
  for (int i = 0; i < rounds; i++) {
    PINE_KEEP_LOOP
    for (int k = 0; k < channels; k++) {
      const float v = weight * perlin_noise3(np, k);
      if (k == 0) accum.x += v;
      else if (k == 1) accum.y += v;
      else accum.z += v;
    }
    weight *= 0.5f;
    np = np * 2.0f;
  }
  const float den = 2.0f - weight * 2;
  const float rx = accum.x / den;  // (no round: 0 / 0, the reference's NaN)
  if (!three) return f3{rx * rx, rx * rx, rx * rx};
  const float ry = accum.y / den, rz = accum.z / den;
  return f3{rx * rx, ry * ry, rz * rz};
}

}  // namespace pine_gpu
