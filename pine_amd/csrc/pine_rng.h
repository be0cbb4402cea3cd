// pine_amd/csrc/pine_rng.h -- the reference's hash and RNG (src/pine/core/rng.h:9-144), integer exact.  A header of its
// own since the noise nodes (pine_noise.h) draw from it in the kernels and in the host's constant folding alike; it needs
// pine_math.h alone.
#pragma once
#include "pine_math.h"

namespace pine_gpu {

PINE_HD uint64_t hash_pixel(int px, int py, int sample_index) {
  // murmur_hash64A over the 12 bytes {px, py, sample_index}, seed 0 (rng.h:9-49, :60-65)
  const uint64_t m = 0xc6a4a7935bd1e995ull;
  const int r = 47;
  uint64_t h = 0 ^ (12ull * m);
  uint64_t k = uint64_t(uint32_t(px)) | (uint64_t(uint32_t(py)) << 32);
  k *= m;
  k ^= k >> r;
  k *= m;
  h ^= k;
  h *= m;
  uint32_t t = uint32_t(sample_index);  // tail of 4 bytes: cases 4..1
  h ^= uint64_t((t >> 24) & 0xff) << 24;
  h ^= uint64_t((t >> 16) & 0xff) << 16;
  h ^= uint64_t((t >> 8) & 0xff) << 8;
  h ^= uint64_t(t & 0xff);
  h *= m;
  h ^= h >> r;
  h *= m;
  h ^= h >> r;
  return h;
}
PINE_HD uint64_t hash_cell(int cx, int cy, int cz, int seed) {
  // hash(vec3i, int): murmur_hash64A over the 16 bytes {cx, cy, cz, seed}, seed 0 -- two whole words, no tail (rng.h:9-49, :60-65)
  const uint64_t m = 0xc6a4a7935bd1e995ull;
  const int r = 47;
  uint64_t h = 0 ^ (16ull * m);
  uint64_t k = uint64_t(uint32_t(cx)) | (uint64_t(uint32_t(cy)) << 32);
  k *= m;
  k ^= k >> r;
  k *= m;
  h ^= k;
  h *= m;
  k = uint64_t(uint32_t(cz)) | (uint64_t(uint32_t(seed)) << 32);
  k *= m;
  k ^= k >> r;
  k *= m;
  h ^= k;
  h *= m;
  h ^= h >> r;
  h *= m;
  h ^= h >> r;
  return h;
}
struct DRng {
  uint64_t s0, s1;
};
PINE_HD uint64_t split_mix_64(uint64_t& s) {  // rng.h:72-77
  uint64_t r = s += 0x9E3779B97f4A7C15ULL;
  r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ULL;
  r = (r ^ (r >> 27)) * 0x94D049BB133111EBULL;
  return r ^ (r >> 31);
}
PINE_HD DRng rng_seed(uint64_t seed) {  // RNG::RNG rng.h:98-101
  DRng g;
  g.s0 = split_mix_64(seed);
  g.s1 = split_mix_64(seed);
  return g;
}
PINE_HD uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
PINE_HD uint64_t rng_next64(DRng& g) {  // rng.h:116-126
  const uint64_t s0 = g.s0;
  uint64_t s1 = g.s1;
  const uint64_t result = s0 + s1;
  s1 ^= s0;
  g.s0 = rotl64(s0, 24) ^ s1 ^ (s1 << 16);
  g.s1 = rotl64(s1, 37);
  return result;
}
PINE_HD float rng_nextf(DRng& g) {  // rng.h:132-135
  uint64_t u = rng_next64(g);
  return pmin(float(uint32_t(u ^ (u >> 32))) * 0x1p-32f, kOneMinusEps);
}

}  // namespace pine_gpu
