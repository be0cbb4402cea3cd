// oracle/pine_oracle.cpp -- TEST INFRASTRUCTURE ONLY (checker + "port" CPU baseline).
//
// A CPU restatement, in this repo's own words, of the algorithm of wicstas/pine's PathIntegrator
// hot path: per-pixel-sample ray generation, pine's binned-SAH BVH (build + ordered traversal),
// shape intersection, BSDF evaluation/sampling, next-event estimation with MIS, and the recursive
// per-level-clamped radiance fold.  It is deliberately written recursively and with pointer-y
// data structures (close to the reference's shape) so that it is independent of the product's
// iterative / flattened GPU formulation in pine_amd/csrc.
//
// Parity status: PINNED.  In the build container this restatement is checked bit-for-bit against
// the real reference compiled from /root/reference (oracle/_ref/pine_ref, oracle/Makefile); the
// outputs of that binary are committed as fixtures under tests/golden/ (tools/make_golden.py), and
// tests/test_oracle_golden.py re-checks this file against them everywhere.
//
// Every function cites the reference file:line it follows (paths relative to /root/reference/).
// All arithmetic is IEEE binary32 with no contraction (build with -ffp-contract=off), in the
// operand order of the reference; the two order-unspecified call sites use the g++ (right-to-left)
// order.
#include "pine_oracle.h"

#include <atomic>
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <utility>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------------
// constants (src/pine/core/math.h:10-16, src/psl/math.h:11-17)
// ------------------------------------------------------------------------------------------------
constexpr float Pi = 3.14159265358979323846f;
constexpr float kEpsilon = 1.1920928955078125e-07f;  // numeric_limits<float>::epsilon()
constexpr float kOneMinusEps = 0x1.fffffep-1f;
constexpr float kFloatMax = 3.40282346638528859812e+38f;

// psl::min/max (src/psl/math.h:19-26): a<b?a:b / a>b?a:b -- NaN and tie behaviour matter.
inline float fmin_(float a, float b) { return a < b ? a : b; }
inline float fmax_(float a, float b) { return a > b ? a : b; }
inline float sqr(float v) { return v * v; }
inline float clampf(float v, float a, float b) { return fmin_(fmax_(v, a), b); }  // math.h:110-112

// ------------------------------------------------------------------------------------------------
// vectors / matrices (src/pine/core/vecmath.h:160-300, 504-640, 690-800)
// ------------------------------------------------------------------------------------------------
struct vec2 {
  float x = 0, y = 0;
  vec2() = default;
  vec2(float x, float y) : x(x), y(y) {}
  float operator[](int i) const { return (&x)[i]; }
};
struct vec3 {
  float x = 0, y = 0, z = 0;
  vec3() = default;
  explicit vec3(float v) : x(v), y(v), z(v) {}
  vec3(float x, float y, float z) : x(x), y(y), z(z) {}
  float& operator[](int i) { return (&x)[i]; }
  float operator[](int i) const { return (&x)[i]; }
  vec3 operator-() const { return {-x, -y, -z}; }
  bool is_zero() const { return x == 0 && y == 0 && z == 0; }
};
inline vec3 operator+(vec3 a, vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline vec3 operator-(vec3 a, vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline vec3 operator*(vec3 a, vec3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline vec3 operator/(vec3 a, vec3 b) { return {a.x / b.x, a.y / b.y, a.z / b.z}; }
inline vec3 operator*(vec3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline vec3 operator*(float s, vec3 a) { return {s * a.x, s * a.y, s * a.z}; }
inline vec3 operator/(vec3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
inline vec3& operator+=(vec3& a, vec3 b) { return a = a + b; }
inline vec2 operator+(vec2 a, vec2 b) { return {a.x + b.x, a.y + b.y}; }
inline vec2 operator-(vec2 a, vec2 b) { return {a.x - b.x, a.y - b.y}; }
inline vec2 operator*(vec2 a, vec2 b) { return {a.x * b.x, a.y * b.y}; }
inline vec2 operator*(vec2 a, float s) { return {a.x * s, a.y * s}; }
inline vec2 operator*(float s, vec2 a) { return {s * a.x, s * a.y}; }

inline float dot(vec3 a, vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }  // vecmath.h:751
inline float absdot(vec3 a, vec3 b) { return std::abs(dot(a, b)); }             // :775
inline vec3 cross(vec3 a, vec3 b) {                                              // :780
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
inline float length_squared(vec3 v) { return v.x * v.x + v.y * v.y + v.z * v.z; }  // :713
inline float length(vec3 v) { return std::sqrt(length_squared(v)); }               // :722
inline float distance(vec3 a, vec3 b) { return length(a - b); }
inline vec3 normalize(vec3 v) {  // :736
  float len = length(v);
  if (len == 0) return v;
  return v / len;
}
inline vec3 normalize(vec3 v, float& len) {  // :742
  len = length(v);
  if (len == 0) return v;
  return v / len;
}
inline vec3 vmin(vec3 a, vec3 b) { return {fmin_(a.x, b.x), fmin_(a.y, b.y), fmin_(a.z, b.z)}; }
inline vec3 vmax(vec3 a, vec3 b) { return {fmax_(a.x, b.x), fmax_(a.y, b.y), fmax_(a.z, b.z)}; }
inline vec3 vabs(vec3 a) { return {std::abs(a.x), std::abs(a.y), std::abs(a.z)}; }
inline int max_axis(vec3 v) {  // vecmath.h:1263
  if (v[0] > v[1])
    return v[0] > v[2] ? 0 : 2;
  else
    return v[1] > v[2] ? 1 : 2;
}
// lerp(u, v, a, b, c) (vecmath.h:882): (1 - u - v) * a + u * b + v * c
inline vec3 lerp3(float u, float v, vec3 a, vec3 b, vec3 c) {
  return (1.0f - u - v) * a + u * b + v * c;
}

struct vec4 {
  float x = 0, y = 0, z = 0, w = 0;
  vec4() = default;
  vec4(float x, float y, float z, float w) : x(x), y(y), z(z), w(w) {}
  vec4(vec3 v, float w) : x(v.x), y(v.y), z(v.z), w(w) {}
  float& operator[](int i) { return (&x)[i]; }
  float operator[](int i) const { return (&x)[i]; }
};
inline vec4 operator+(vec4 a, vec4 b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
inline vec4 operator*(vec4 a, float s) { return {a.x * s, a.y * s, a.z * s, a.w * s}; }

struct mat3 {  // column vectors (vecmath.h:504-572)
  vec3 x{1, 0, 0}, y{0, 1, 0}, z{0, 0, 1};
  mat3() = default;
  mat3(vec3 x, vec3 y, vec3 z) : x(x), y(y), z(z) {}
  vec3& operator[](int i) { return (&x)[i]; }
  const vec3& operator[](int i) const { return (&x)[i]; }
  vec3 row(int i) const { return {x[i], y[i], z[i]}; }
};
inline vec3 operator*(const mat3& m, vec3 v) { return m.x * v.x + m.y * v.y + m.z * v.z; }  // :695
inline mat3 transpose(const mat3& m) { return {m.row(0), m.row(1), m.row(2)}; }

struct mat4 {  // column vectors; scalar ctor takes row-major arguments (vecmath.h:575-585)
  vec4 x{1, 0, 0, 0}, y{0, 1, 0, 0}, z{0, 0, 1, 0}, w{0, 0, 0, 1};
  mat4() = default;
  mat4(float x0, float y0, float z0, float w0, float x1, float y1, float z1, float w1, float x2,
       float y2, float z2, float w2, float x3, float y3, float z3, float w3)
      : x(x0, x1, x2, x3), y(y0, y1, y2, y3), z(z0, z1, z2, z3), w(w0, w1, w2, w3) {}
  mat4(vec4 x, vec4 y, vec4 z, vec4 w) : x(x), y(y), z(z), w(w) {}
  vec4& operator[](int i) { return (&x)[i]; }
  const vec4& operator[](int i) const { return (&x)[i]; }
};
inline mat3 to_mat3(const mat4& m) {  // vecmath.h:588
  return {vec3(m.x.x, m.x.y, m.x.z), vec3(m.y.x, m.y.y, m.y.z), vec3(m.z.x, m.z.y, m.z.z)};
}
inline vec3 operator*(const mat4& m, vec3 v) {  // affine point transform, vecmath.h:705
  vec4 r = m.x * v.x + m.y * v.y + m.z * v.z + m.w;
  return {r.x, r.y, r.z};
}
inline mat4 operator*(const mat4& l, const mat4& r) {  // vecmath.h:617
  mat4 ret(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  for (int c = 0; c < 4; c++)
    for (int rr = 0; rr < 4; rr++)
      for (int i = 0; i < 4; i++) ret[c][rr] += l[i][rr] * r[c][i];
  return ret;
}
mat4 inverse(const mat4& m) {  // vecmath.cpp:103-132
  mat4 r;
  float det = 0;
  for (int i = 0; i < 4; i++)
    det += (m[(1 + i) % 4][0] *
                (m[(2 + i) % 4][1] * m[(3 + i) % 4][2] - m[(3 + i) % 4][1] * m[(2 + i) % 4][2]) +
            m[(2 + i) % 4][0] *
                (m[(3 + i) % 4][1] * m[(1 + i) % 4][2] - m[(1 + i) % 4][1] * m[(3 + i) % 4][2]) +
            m[(3 + i) % 4][0] *
                (m[(1 + i) % 4][1] * m[(2 + i) % 4][2] - m[(2 + i) % 4][1] * m[(1 + i) % 4][2])) *
           m[i % 4][3] * (i % 2 ? -1 : 1);
  if (det == 0) return r;
  for (int v = 0; v < 4; v++)
    for (int i = 0; i < 4; i++)
      r[v][i] = (m[(1 + i) % 4][(1 + v) % 4] *
                     (m[(2 + i) % 4][(2 + v) % 4] * m[(3 + i) % 4][(3 + v) % 4] -
                      m[(3 + i) % 4][(2 + v) % 4] * m[(2 + i) % 4][(3 + v) % 4]) +
                 m[(2 + i) % 4][(1 + v) % 4] *
                     (m[(3 + i) % 4][(2 + v) % 4] * m[(1 + i) % 4][(3 + v) % 4] -
                      m[(1 + i) % 4][(2 + v) % 4] * m[(3 + i) % 4][(3 + v) % 4]) +
                 m[(3 + i) % 4][(1 + v) % 4] *
                     (m[(1 + i) % 4][(2 + v) % 4] * m[(2 + i) % 4][(3 + v) % 4] -
                      m[(2 + i) % 4][(2 + v) % 4] * m[(1 + i) % 4][(3 + v) % 4])) *
                ((v + i) % 2 ? 1 : -1);
  for (int c = 0; c < 4; c++)
    for (int rr = 0; rr < 4; rr++) r[c][rr] /= det;
  return r;
}
mat3 inverse(const mat3& m) {  // vecmath.cpp:80-102
  mat3 r;
  float det = m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) +
              m[1][0] * (m[2][1] * m[0][2] - m[0][1] * m[2][2]) +
              m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]);
  if (det == 0) return r;
  r[0][0] = m[1][1] * m[2][2] - m[2][1] * m[1][2];
  r[0][1] = m[2][1] * m[0][2] - m[0][1] * m[2][2];
  r[0][2] = m[0][1] * m[1][2] - m[1][1] * m[0][2];
  r[1][0] = m[1][2] * m[2][0] - m[2][2] * m[1][0];
  r[1][1] = m[2][2] * m[0][0] - m[0][2] * m[2][0];
  r[1][2] = m[0][2] * m[1][0] - m[1][2] * m[0][0];
  r[2][0] = m[1][0] * m[2][1] - m[2][0] * m[1][1];
  r[2][1] = m[2][0] * m[0][1] - m[0][0] * m[2][1];
  r[2][2] = m[0][0] * m[1][1] - m[1][0] * m[0][1];
  for (int c = 0; c < 3; c++)
    for (int rr = 0; rr < 3; rr++) r[c][rr] /= det;
  return r;
}
inline mat4 translate(vec3 v) {  // vecmath.h:1113
  return {1.0f, 0.0f, 0.0f, v.x, 0.0f, 1.0f, 0.0f, v.y, 0.0f, 0.0f, 1.0f, v.z, 0.0f, 0.0f, 0.0f, 1.0f};
}
inline mat4 scale(vec3 v) {  // :1131
  return {v.x, 0.0f, 0.0f, 0.0f, 0.0f, v.y, 0.0f, 0.0f, 0.0f, 0.0f, v.z, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
}
inline mat4 rotate_z(float r) {  // :1140
  return mat4{std::cos(r), -std::sin(r), 0, 0, std::sin(r), std::cos(r), 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
}
inline mat4 rotate_x(float r) {  // :1149
  return mat4{1, 0, 0, 0, 0, std::cos(r), -std::sin(r), 0, 0, std::sin(r), std::cos(r), 0, 0, 0, 0, 1};
}
inline mat4 rotate_y(float r) {  // :1158
  return mat4{std::cos(r), 0, std::sin(r), 0, 0, 1, 0, 0, -std::sin(r), 0, std::cos(r), 0, 0, 0, 0, 1};
}
inline mat4 look_at(vec3 from, vec3 at, vec3 up = vec3(0, 1, 0)) {  // :1172-1180
  vec3 z = normalize(at - from);
  if (std::abs(dot(z, up)) > 0.999f) z = normalize(z + vec3(0.0f, 0.0f, 1e-5f));
  vec3 x = normalize(cross(up, z));
  vec3 y = cross(z, x);
  return mat4(vec4(x, 0), vec4(y, 0), vec4(z, 0), vec4(from, 1.0f));
}
inline void coordinate_system(vec3 n, vec3& t, vec3& b) {  // :1182-1188
  if (std::abs(n.x) > std::abs(n.y))
    t = normalize(cross(n, vec3(0, 1, 0)));
  else
    t = normalize(cross(n, vec3(1, 0, 0)));
  b = cross(n, t);
}
inline mat3 coordinate_system(vec3 n) {  // :1190-1195
  mat3 m;
  m.z = n;
  coordinate_system(n, m.x, m.y);
  return m;
}
inline float phi2pi(float x, float y) {  // :1209
  float phi = std::atan2(y, x);
  return phi < 0.0f ? Pi * 2 + phi : phi;
}
inline vec2 cartesian_to_spherical(vec3 d) { return vec2(phi2pi(d.x, d.y), std::acos(d.z)); }
inline vec3 spherical_to_cartesian(float phi, float sin_theta, float cos_theta) {  // :1201
  return vec3(sin_theta * std::cos(phi), sin_theta * std::sin(phi), cos_theta);
}
inline vec3 face_same_hemisphere(vec3 v, vec3 ref) { return dot(v, ref) < 0 ? -v : v; }  // :1220
inline float safe_rcp(float v) { return v == 0.0f ? 1e+20f : 1.0f / v; }                  // :1062

// ------------------------------------------------------------------------------------------------
// hash / RNG (src/pine/core/rng.h:9-144)
// ------------------------------------------------------------------------------------------------
uint64_t murmur64A(const unsigned char* key, size_t len, uint64_t seed) {  // rng.h:9-49
  const uint64_t m = 0xc6a4a7935bd1e995ull;
  const int r = 47;
  uint64_t h = seed ^ (len * m);
  const unsigned char* end = key + 8 * (len / 8);
  while (key != end) {
    uint64_t k;
    memcpy(&k, key, 8);
    key += 8;
    k *= m;
    k ^= k >> r;
    k *= m;
    h ^= k;
    h *= m;
  }
  switch (len & 7) {
    case 7: h ^= uint64_t(key[6]) << 48; [[fallthrough]];
    case 6: h ^= uint64_t(key[5]) << 40; [[fallthrough]];
    case 5: h ^= uint64_t(key[4]) << 32; [[fallthrough]];
    case 4: h ^= uint64_t(key[3]) << 24; [[fallthrough]];
    case 3: h ^= uint64_t(key[2]) << 16; [[fallthrough]];
    case 2: h ^= uint64_t(key[1]) << 8; [[fallthrough]];
    case 1: h ^= uint64_t(key[0]); h *= m;
  }
  h ^= h >> r;
  h *= m;
  h ^= h >> r;
  return h;
}
uint64_t hash_pixel(int px, int py, int sample_index) {  // hash(vec2i, int): rng.h:60-65
  int buf[3] = {px, py, sample_index};
  return murmur64A((const unsigned char*)buf, 12, 0);
}
struct RNG {  // rng.h:97-144
  uint64_t s[2];
  explicit RNG(uint64_t seed = 0) {
    s[0] = split_mix(seed);
    s[1] = split_mix(seed);
  }
  static uint64_t split_mix(uint64_t& st) {  // rng.h:72-77
    uint64_t r = st += 0x9E3779B97f4A7C15ULL;
    r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ULL;
    r = (r ^ (r >> 27)) * 0x94D049BB133111EBULL;
    return r ^ (r >> 31);
  }
  static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  uint64_t next64u() {  // rng.h:116-126
    const uint64_t s0 = s[0];
    uint64_t s1 = s[1];
    const uint64_t result = s0 + s1;
    s1 ^= s0;
    s[0] = rotl(s0, 24) ^ s1 ^ (s1 << 16);
    s[1] = rotl(s1, 37);
    return result;
  }
  float nextf() {  // rng.h:132-135
    uint64_t u = next64u();
    return fmin_(uint32_t(u ^ (u >> 32)) * 0x1p-32f, kOneMinusEps);
  }
  vec2 next2f() {  // braced init list: x first, then y (rng.h:136-138)
    float a = nextf();
    float b = nextf();
    return {a, b};
  }
};

// ------------------------------------------------------------------------------------------------
// BlueSobolSampler + Sampler wrapper (sampler.h:166-201,275-324; sampler.cpp:115-143;
// src/contrib/bluesobol/bluenoise_16spp.cpp:14-34)
// ------------------------------------------------------------------------------------------------
struct BlueTables {
  const uint8_t* sobol = nullptr;     // [256*256]
  const uint8_t* scramble = nullptr;  // [128*128*8] for the chosen spp
  const uint8_t* rank = nullptr;      // [128*128*8]
};
int roundup2(int x) {  // src/psl/math.h:86-94
  if (x == 0) return 0;
  x -= 1;
  for (size_t i = 1; i != sizeof(x) * 8; i <<= 1) x |= x >> i;
  return x + 1;
}
int bluesobol_effective_spp(int spp) {  // sampler.cpp:115-121
  if (spp > 256) spp = 256;
  return roundup2(spp);
}
BlueTables select_tables(const uint8_t* blob, int spp_eff) {
  int k = 0;
  while ((1 << k) < spp_eff) k++;
  BlueTables t;
  t.sobol = blob;
  t.scramble = blob + 65536 + size_t(k) * 262144;
  t.rank = t.scramble + 131072;
  return t;
}
// ---- SobolSampler (sampler.h:83-164, sampler.cpp:81-113, lowdiscrepancy.h:73-80) ------------------
inline uint64_t mix_bits(uint64_t v) {  // rng.h:81-88
  v ^= (v >> 31);
  v *= 0x7fb5d329728ea185ull;
  v ^= (v >> 27);
  v *= 0x81dadef4bc2dd44dull;
  v ^= (v >> 33);
  return v;
}
inline uint32_t reverse_bits32(uint32_t x) {  // math.h:20-27
  x = (x & 0x55555555) << 1 | (x & 0xaaaaaaaa) >> 1;
  x = (x & 0x33333333) << 2 | (x & 0xcccccccc) >> 2;
  x = (x & 0x0f0f0f0f) << 4 | (x & 0xf0f0f0f0) >> 4;
  x = (x & 0x00ff00ff) << 8 | (x & 0xff00ff00) >> 8;
  return (x << 16) | (x >> 16);
}
inline uint64_t left_shift_64x2(uint64_t x) {  // vecmath.h:1231-1239
  x &= 0xffffffff;
  x = (x ^ (x << 16)) & 0x0000ffff0000ffffull;
  x = (x ^ (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x ^ (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x ^ (x << 2)) & 0x3333333333333333ull;
  x = (x ^ (x << 1)) & 0x5555555555555555ull;
  return x;
}
inline uint64_t encode_morton64x2(uint32_t x, uint32_t y) {  // vecmath.h:1243-1245
  return (left_shift_64x2(y) << 1) | left_shift_64x2(x);
}
inline int log2i_(int y) {  // psl::log2i = hsb = ieeeexp(float(x)) (src/psl/math.h:77-81,262-264)
  float f = float(uint32_t(y));
  uint32_t u;
  memcpy(&u, &f, 4);
  return int(0xff & (u >> 23)) - 127;
}
inline uint32_t fast_owen(uint32_t v, uint32_t seed) {  // SobolSampler::FastOwenScrambler sampler.h:95-109
  v = reverse_bits32(v);
  v ^= v * 0x3d20adeau;
  v += seed;
  v *= (seed >> 16) | 1;
  v ^= v * 0x05526c56u;
  v ^= v * 0x53a22864u;
  return reverse_bits32(v);
}
// The first two of the 1024 Sobol' generator matrices (sobolmatrices.cpp:40-: 52 columns each) have closed
// forms: dimension 0 is the bit reversal (column i = 2^31 >> i, zero from i = 32), dimension 1 follows
// v[0] = 2^31, v[i+1] = v[i] ^ (v[i] >> 1) through all 52 columns.  SobolSampler only ever reads these two.
inline uint32_t sobol_matrix(int dim, int i) {
  if (dim == 0) return i < 32 ? 0x80000000u >> i : 0u;
  uint32_t v = 0x80000000u;
  for (int k = 0; k < i; k++) v ^= v >> 1;
  return v;
}
inline float sobol_sample(int64_t a, int dim, uint32_t seed) {  // lowdiscrepancy.h:73-80 with FastOwenScrambler
  uint32_t v = 0;
  for (int i = 0; a != 0; a >>= 1, i++)
    if (a & 1) v ^= sobol_matrix(dim, i);
  v = fast_owen(v, seed);
  return fmin_(float(v) * 0x1p-32f, kOneMinusEps);
}

// ---- HaltonSampler (sampler.h:40-81, sampler.cpp:16-79, lowdiscrepancy.h:10-52, lowdiscrepancy.cpp:5-17) --------
// Oracle only so far (the device refuses it): the tables are derived, not stored -- Primes[] is the first 1000
// primes and PrimeSums[] their prefix sums (primes.cpp), the digit permutations come from a default-seeded RNG.
struct HaltonTables {
  std::vector<int> primes, sums;
  std::vector<uint16_t> perms;
  int baseScales[2], baseExponents[2], multInverse[2], sampleStride;
  static void extended_gcd(uint64_t a, uint64_t b, int64_t& gcd, int64_t& x, int64_t& y) {  // sampler.cpp:16-31 (int d, r as there)
    int d = int(a / b);
    int r = int(a - uint64_t(d) * b);
    if (r == 0) {
      gcd = int64_t(b);
      x = 0;
      y = 1;
      return;
    }
    int64_t nx, ny;
    extended_gcd(b, uint64_t(r), gcd, nx, ny);
    x = ny;
    y = nx - d * ny;
  }
  static int64_t mod_(int64_t a, int64_t b) {  // psl::mod src/psl/math.h:103-107
    int64_t r = a - (a / b) * b;
    return r < 0 ? r + b : r;
  }
  HaltonTables() {
    for (int n = 2; int(primes.size()) < 1000; n++) {
      bool is_prime = true;
      for (int d = 2; d * d <= n; d++)
        if (n % d == 0) {
          is_prime = false;
          break;
        }
      if (is_prime) primes.push_back(n);
    }
    int acc = 0;
    for (int p : primes) {
      sums.push_back(acc);
      acc += p;
    }
    perms.resize(size_t(acc));
    RNG rng;  // HaltonSampler ctor: `RNG rng;` (seed 0)
    uint16_t* p = perms.data();
    for (int i = 0; i < 1000; i++) {
      for (int j = 0; j < primes[i]; j++) p[j] = uint16_t(j);
      for (int k = 0; k < primes[i]; k++) {  // shuffle(p, count, 1, rng) lowdiscrepancy.h:55-61
        uint64_t h = rng.next64u();
        uint32_t other = uint32_t(k) + uint32_t(h ^ (h >> 32)) % uint32_t(primes[i] - k);
        std::swap(p[k], p[other]);
      }
      p += primes[i];
    }
    for (int i = 0; i < 2; i++) {
      int base = i == 0 ? 2 : 3, scale = 1, exp = 0;
      while (scale < 128) {  // MaxHaltonResolution
        scale *= base;
        ++exp;
      }
      baseScales[i] = scale;
      baseExponents[i] = exp;
    }
    auto mult_inverse = [](int64_t a, int64_t n) {
      int64_t gcd, x, y;
      extended_gcd(uint64_t(a), uint64_t(n), gcd, x, y);
      return uint64_t(mod_(x, n));
    };
    multInverse[0] = int(mult_inverse(baseScales[0], baseScales[1]));
    multInverse[1] = int(mult_inverse(baseScales[1], baseScales[0]));
    sampleStride = baseScales[0] * baseScales[1];
  }
  float scrambled_radical_inverse(int baseIndex, uint64_t a) const {  // lowdiscrepancy.h:26-40
    const uint16_t* perm = &perms[size_t(sums[baseIndex])];
    int base = primes[baseIndex];
    float invBase = 1.0f / base, invBaseN = 1.0f;
    uint64_t reversedDigits = 0;
    while (a) {
      uint64_t next = a / uint64_t(base);
      uint64_t digits = a - next * uint64_t(base);
      reversedDigits = reversedDigits * uint64_t(base) + perm[digits];
      invBaseN *= invBase;
      a = next;
    }
    float series = perm[0] / (base + 1.0f);
    return fmin_((float(reversedDigits) + series) * invBaseN, kOneMinusEps);
  }
  static uint64_t inverse_radical_inverse(uint64_t inverse, int base, int nDigits) {  // lowdiscrepancy.h:42-51
    uint64_t index = 0;
    for (int i = 0; i < nDigits; i++) {
      uint64_t digit = inverse % uint64_t(base);
      inverse /= uint64_t(base);
      index = index * uint64_t(base) + digit;
    }
    return index;
  }
};
static const HaltonTables& halton_tables() {
  static const HaltonTables t;
  return t;
}

enum SamplerKind { SAMPLER_BLUE = 0, SAMPLER_SOBOL = 1, SAMPLER_HALTON = 2 };
struct Sampler {
  BlueTables t;
  int kind = SAMPLER_BLUE;
  int spp = 1;
  int dimension = 0;
  int px = 0, py = 0, index = 0;
  RNG rng;
  uint64_t* rng_draws = nullptr;
  // SobolSampler state
  int log2_spp = 0, nbase4_digits = 0;
  uint64_t sobol_index = 0;
  // HaltonSampler state
  int64_t halton_index = 0;

  void init(int W, int H) {  // Sampler::init -> SobolSampler::init sampler.cpp:81-84 (a no-op for the others)
    log2_spp = log2i_(spp);  // SobolSampler ctor sampler.h:127-129
    int res = roundup2(std::max(W, H));
    nbase4_digits = log2i_(res) + (log2_spp + 1) / 2;
  }
  void start_pixel(int x, int y, int sample_index) {  // sampler.h:286-290 + :174-177 / :135-138
    rng = RNG(hash_pixel(x, y, sample_index));
    px = x;
    py = y;
    index = sample_index;  // NB: BlueSobolSampler does NOT reset its dimension here
    if (kind == SAMPLER_SOBOL) {
      dimension = 0;
      sobol_index = (encode_morton64x2(uint32_t(x), uint32_t(y)) << log2_spp) | uint64_t(sample_index);
    }
    if (kind == SAMPLER_HALTON) {  // sampler.cpp:64-79
      const HaltonTables& H = halton_tables();
      halton_index = 0;
      if (H.sampleStride > 1) {
        const int pm[2] = {int(HaltonTables::mod_(x, 128)), int(HaltonTables::mod_(y, 128))};
        for (int i = 0; i < 2; i++) {
          uint64_t dimOffset = HaltonTables::inverse_radical_inverse(uint64_t(pm[i]), i == 0 ? 2 : 3, H.baseExponents[i]);
          halton_index += int64_t(dimOffset * uint64_t(H.baseScales[1 - i]) * uint64_t(H.multInverse[1 - i]));
        }
        halton_index %= H.sampleStride;
      }
      halton_index += int64_t(sample_index) * H.sampleStride;
      dimension = 2;
    }
  }
  void start_next_sample() {  // sampler.h:178-181 / :139-142 / :48-51
    dimension = kind == SAMPLER_HALTON ? 2 : 0;
    index++;
    sobol_index++;
    halton_index += halton_tables().sampleStride;
  }
  uint64_t sobol_compute_sample_index() const {  // sampler.cpp:86-113
    static const uint8_t permutations[24][4] = {
        {0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 2, 1}, {0, 3, 1, 2},
        {1, 0, 2, 3}, {1, 0, 3, 2}, {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 2, 0}, {1, 3, 0, 2},
        {2, 1, 0, 3}, {2, 1, 3, 0}, {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 3, 0, 1}, {2, 3, 1, 0},
        {3, 1, 2, 0}, {3, 1, 0, 2}, {3, 2, 1, 0}, {3, 2, 0, 1}, {3, 0, 2, 1}, {3, 0, 1, 2}};
    uint64_t si = 0;
    const bool only_power_of_2 = (log2_spp & 1) != 0;
    const int last_digit = only_power_of_2 ? 1 : 0;
    for (int i = nbase4_digits - 1; i >= last_digit; --i) {
      int digit_shift = 2 * i - (only_power_of_2 ? 1 : 0);
      int digit = int((sobol_index >> digit_shift) & 3);
      uint64_t higher_digits = sobol_index >> (digit_shift + 2);
      int p = int((mix_bits(higher_digits ^ (0x55555555u * uint32_t(dimension))) >> 24) % 24);
      digit = permutations[p][digit];
      si |= uint64_t(digit) << digit_shift;
    }
    if (only_power_of_2) {
      int digit = int(sobol_index & 1);
      si |= uint64_t(digit ^ int(mix_bits((sobol_index >> 1) ^ (0x55555555u * uint32_t(dimension))) & 1));
    }
    return si;
  }
  static uint64_t hash_int(int v) { return murmur64A(reinterpret_cast<const unsigned char*>(&v), 4, 0); }  // hash(dimension) rng.h:60-65
  float sample_dimension(int dim) const {  // bluenoise_*spp.cpp:14-34
    int pi = px & 127, pj = py & 127;
    int si = index & 255;
    int sd = dim & 255;
    int ranked = si ^ t.rank[(sd + (pi + pj * 128) * 8) % (128 * 128 * 8)];
    int value = t.sobol[sd + ranked * 256];
    value = value ^ t.scramble[(sd % 8) + (pi + pj * 128) * 8];
    return (0.5f + value) / 256.0f;
  }
  float get1d() {  // sampler.h:183-187 / :143-148 / :52-56
    if (kind == SAMPLER_HALTON) {
      if (dimension >= 1000) dimension = 2;
      return halton_tables().scrambled_radical_inverse(dimension++, uint64_t(halton_index));
    }
    if (kind == SAMPLER_SOBOL) {
      uint64_t si = sobol_compute_sample_index();
      dimension += 1;
      uint64_t u = hash_int(dimension);
      return sobol_sample(int64_t(si), 0, uint32_t(u));
    }
    if (dimension >= 256) dimension = 2;
    return sample_dimension(dimension++);
  }
  vec2 get2d() {  // sampler.h:188-194 / :149-155 / :57-63
    if (kind == SAMPLER_HALTON) {
      if (dimension + 1 >= 1000) dimension = 2;
      const int dim = dimension;
      dimension += 2;
      const float a = halton_tables().scrambled_radical_inverse(dim, uint64_t(halton_index));
      const float b = halton_tables().scrambled_radical_inverse(dim + 1, uint64_t(halton_index));
      return {a, b};
    }
    if (kind == SAMPLER_SOBOL) {
      uint64_t si = sobol_compute_sample_index();
      dimension += 2;
      uint64_t u = hash_int(dimension);
      float a = sobol_sample(int64_t(si), 0, uint32_t(u));
      float b = sobol_sample(int64_t(si), 1, uint32_t(u >> 32));
      return {a, b};
    }
    if (dimension + 1 >= 256) dimension = 2;
    int dim = dimension;
    dimension += 2;
    float a = sample_dimension(dim);
    float b = sample_dimension(dim + 1);
    return {a, b};
  }
  float randf() { return rng.nextf(); }
  vec2 rand2f() { return rng.next2f(); }
};
// with_probability (sampler.h:317-324): draws from the RNG only when prob is strictly in (0,1)
bool with_probability(float prob, Sampler& s) {
  if (prob == 0) return false;
  if (prob == 1) return true;
  return s.randf() < prob;
}

// ------------------------------------------------------------------------------------------------
// sampling.h:8-89
// ------------------------------------------------------------------------------------------------
vec2 sample_disk_polar(vec2 u) {
  float r = std::sqrt(u[0]);
  float theta = 2 * Pi * u[1];
  return {r * std::cos(theta), r * std::sin(theta)};
}
vec2 sample_disk_concentric(vec2 u) {
  u = vec2(u.x * 2 - 1.0f, u.y * 2 - 1.0f);
  float theta, r;
  if (std::abs(u.x) > std::abs(u.y)) {
    r = u.x;
    theta = Pi / 4.0f * u.y / u.x;
  } else {
    r = u.y;
    theta = Pi / 2.0f - Pi / 4.0f * (u.x / u.y);
  }
  return r * vec2(std::cos(theta), std::sin(theta));
}
vec3 cosine_weighted_hemisphere(vec2 u) {
  vec2 d = sample_disk_concentric(u);
  float z = std::sqrt(fmax_(1.0f - d.x * d.x - d.y * d.y, 0.0f));
  return vec3(d.x, d.y, z);
}
vec3 uniform_sphere(vec2 u) {
  const float phi = u.x * Pi * 2;
  const float cos_theta = 1 - 2 * u.y;
  const float sin_theta = std::sqrt(1.0f - sqr(cos_theta));
  return vec3(sin_theta * std::cos(phi), sin_theta * std::sin(phi), cos_theta);
}
float balance_heuristic(float pF, float pG) { return pF / (pF + pG); }

// ------------------------------------------------------------------------------------------------
// Ray + spawn (src/pine/core/ray.h:8-57, interaction.cpp:6-13)
// ------------------------------------------------------------------------------------------------
struct Ray {
  vec3 o, d;
  float tmin = 0.0f, tmax = kFloatMax;
  Ray() = default;
  Ray(vec3 o, vec3 d) : o(o), d(d) {}
  Ray(vec3 o, vec3 d, float tmin, float tmax) : o(o), d(d), tmin(tmin), tmax(tmax) {}
  vec3 operator()() const { return o + tmax * d; }
  vec3 operator()(float t) const { return o + t * d; }
};
inline float bits_add(float f, int di) {
  int32_t b;
  memcpy(&b, &f, 4);
  b += di;
  memcpy(&f, &b, 4);
  return f;
}
vec3 offset_ray_origin(vec3 p, vec3 n) {  // ray.h:25-37 (integer ULP stepping)
  const float origin = 1.0f / 32.0f;
  const float float_scale = 1.0f / 65536.0f;
  const float int_scale = 256.0f;
  int ox = int(int_scale * n.x), oy = int(int_scale * n.y), oz = int(int_scale * n.z);
  vec3 p_i(bits_add(p.x, p.x < 0 ? -ox : ox), bits_add(p.y, p.y < 0 ? -oy : oy),
           bits_add(p.z, p.z < 0 ? -oz : oz));
  return {std::abs(p.x) < origin ? p.x + n.x * float_scale : p_i.x,
          std::abs(p.y) < origin ? p.y + n.y * float_scale : p_i.y,
          std::abs(p.z) < origin ? p.z + n.z * float_scale : p_i.z};
}
Ray spawn_ray_pn(vec3 p, vec3 n, vec3 wo, float dist = kFloatMax) {  // ray.h:39-46
  Ray r;
  r.o = offset_ray_origin(p, n);
  r.d = wo;
  r.tmin = 0.0f;
  r.tmax = dist * (1.0f - 1e-3f);
  return r;
}

struct SurfaceInteraction {  // interaction.h:9-33
  vec3 p, n;
  vec2 uv;
  mat3 w2l, l2w;
  int geom = -1;
  void compute_transformation() {
    l2w = coordinate_system(n);
    w2l = transpose(l2w);
  }
  vec3 to_world(vec3 w) const { return l2w * w; }
  vec3 to_local(vec3 w) const { return w2l * w; }
  Ray spawn_ray(vec3 wo, float tmax = kFloatMax) const {  // interaction.cpp:6-13
    Ray r;
    r.d = wo;
    r.o = offset_ray_origin(p, face_same_hemisphere(n, r.d));
    r.tmin = 0.0f;
    r.tmax = tmax * (1.0f - 1e-3f);
    return r;
  }
};

// ------------------------------------------------------------------------------------------------
// AABB (bbox.h:29-84, bbox.cpp:8-143)
// ------------------------------------------------------------------------------------------------
struct RayOctant {  // bbox.h:18-27
  int octantx3[3];
  vec3 dir_inv, org_div_dir;
  explicit RayOctant(const Ray& r) {
    for (int i = 0; i < 3; i++) octantx3[i] = (r.d[i] < 0 ? 1 : 0) * 3;
    dir_inv = vec3(safe_rcp(r.d.x), safe_rcp(r.d.y), safe_rcp(r.d.z));
    org_div_dir = r.o * dir_inv;
  }
};
struct AABB {
  vec3 lower{kFloatMax, kFloatMax, kFloatMax}, upper{-kFloatMax, -kFloatMax, -kFloatMax};
  AABB() = default;
  AABB(vec3 lo, vec3 hi) : lower(lo), upper(hi) {}
  vec3 centroid() const { return (lower + upper) / 2.0f; }
  float centroid(int d) const { return (lower[d] + upper[d]) / 2; }
  vec3 diagonal() const { return upper - lower; }
  float surface_area() const {  // bbox.cpp:37-40
    vec3 d = diagonal();
    return 2.0f * (d.x * d.y + d.x * d.z + d.y * d.z);
  }
  float area() const {  // bbox.cpp:139-142
    vec3 d = diagonal();
    return 2 * (d.x * d.y + d.x * d.z + d.y * d.z);
  }
  AABB& extend(vec3 p) {
    lower = vmin(lower, p);
    upper = vmax(upper, p);
    return *this;
  }
  AABB& extend(const AABB& b) {
    lower = vmin(lower, b.lower);
    upper = vmax(upper, b.upper);
    return *this;
  }
  AABB& extend_by(float a) {
    lower = lower - vec3(a);
    upper = upper + vec3(a);
    return *this;
  }
  bool degenerated(int d) const { return upper[d] <= lower[d]; }
  float relative_position(float p, int dim) const {  // bbox.cpp:32-36
    float o = p - lower[dim];
    float d = upper[dim] - lower[dim];
    return d > 0.0f ? o / d : o;
  }
  // slab test used by the BVH (bbox.h:59-72)
  bool hit(const RayOctant& r, float tmin, float& tmax) const {
    const float* p = &lower.x;  // lower(3) then upper(3), contiguous
    float q[6] = {lower.x, lower.y, lower.z, upper.x, upper.y, upper.z};
    (void)p;
    float tmin0 = q[0 + r.octantx3[0]] * r.dir_inv[0] - r.org_div_dir[0];
    float tmin1 = q[1 + r.octantx3[1]] * r.dir_inv[1] - r.org_div_dir[1];
    float tmin2 = q[2 + r.octantx3[2]] * r.dir_inv[2] - r.org_div_dir[2];
    float tmax0 = q[3 - r.octantx3[0]] * r.dir_inv[0] - r.org_div_dir[0];
    float tmax1 = q[4 - r.octantx3[1]] * r.dir_inv[1] - r.org_div_dir[1];
    float tmax2 = q[5 - r.octantx3[2]] * r.dir_inv[2] - r.org_div_dir[2];
    // psl::max(a,b,c,d) = max(a, max(b, max(c, d))) (src/psl/math.h:52-61)
    tmin = fmax_(tmin0, fmax_(tmin1, fmax_(tmin2, tmin)));
    tmax = fmin_(tmax0, fmin_(tmax1, fmin_(tmax2, tmax)));
    return tmin <= tmax;
  }
  // the same slab test, reporting the ENTRY distance (order mode "nearest", below)
  bool entry(const RayOctant& r, float tmin, float tmax, float& tnear) const {
    float q[6] = {lower.x, lower.y, lower.z, upper.x, upper.y, upper.z};
    float tmin0 = q[0 + r.octantx3[0]] * r.dir_inv[0] - r.org_div_dir[0];
    float tmin1 = q[1 + r.octantx3[1]] * r.dir_inv[1] - r.org_div_dir[1];
    float tmin2 = q[2 + r.octantx3[2]] * r.dir_inv[2] - r.org_div_dir[2];
    float tmax0 = q[3 - r.octantx3[0]] * r.dir_inv[0] - r.org_div_dir[0];
    float tmax1 = q[4 - r.octantx3[1]] * r.dir_inv[1] - r.org_div_dir[1];
    float tmax2 = q[5 - r.octantx3[2]] * r.dir_inv[2] - r.org_div_dir[2];
    tnear = fmax_(tmin0, fmax_(tmin1, fmax_(tmin2, tmin)));
    const float tfar = fmin_(tmax0, fmin_(tmax1, fmin_(tmax2, tmax)));
    return tnear <= tfar;
  }
  bool hit(const Ray& ray) const {  // bbox.cpp:75-93
    float tmin = ray.tmin, tmax = ray.tmax;
    if (tmin > tmax) return false;
    for (int i = 0; i < 3; i++) {
      if (std::abs(ray.d[i]) < 1e-6f) {
        if (ray.o[i] < lower[i] || ray.o[i] > upper[i]) return false;
        continue;
      }
      float inv_d = 1.0f / ray.d[i];
      float t_near = (lower[i] - ray.o[i]) * inv_d;
      float t_far = (upper[i] - ray.o[i]) * inv_d;
      if (inv_d < 0.0f) std::swap(t_far, t_near);
      tmin = fmax_(t_near, tmin);
      tmax = fmin_(t_far, tmax);
      if (tmin > tmax) return false;
    }
    return true;
  }
  bool intersect(vec3 o, vec3 d, float& tmin, float& tmax) const {  // bbox.cpp:94-111
    for (int i = 0; i < 3; i++) {
      if (std::abs(d[i]) < 1e-6f) {
        if (o[i] < lower[i] || o[i] > upper[i]) return false;
        continue;
      }
      float inv_d = 1.0f / d[i];
      float t_near = (lower[i] - o[i]) * inv_d;
      float t_far = (upper[i] - o[i]) * inv_d;
      if (inv_d < 0.0f) std::swap(t_far, t_near);
      tmin = fmax_(t_near, tmin);
      tmax = fmin_(t_far, tmax);
      if (tmin > tmax) return false;
    }
    return true;
  }
  bool intersect(Ray& ray) const {  // bbox.cpp:112-121
    float tmin = ray.tmin, tmax = ray.tmax;
    if (intersect(ray.o, ray.d, tmin, tmax)) {
      ray.tmax = tmin > ray.tmin ? tmin : tmax;
      return true;
    }
    return false;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // bbox.cpp:122-129
    it.p = p;
    vec3 pu = (p - centroid()) / diagonal();
    int axis = max_axis(vabs(pu));
    it.n = vec3(0.0f);
    it.n[axis] = pu[axis] > 0 ? 1 : -1;
    it.p[axis] = pu[axis] > 0 ? upper[axis] : lower[axis];
  }
};
inline AABB union_(AABB l, AABB r) { return {vmin(l.lower, r.lower), vmax(l.upper, r.upper)}; }

// ------------------------------------------------------------------------------------------------
// Shapes (geometry.h / geometry.cpp / bbox.cpp)
// ------------------------------------------------------------------------------------------------
struct ShapeSample {  // bbox.h:8-16
  vec3 p, n;
  vec2 uv;
  vec3 w;
  float distance = 0.0f, pdf = 0.0f;
};
bool intersect_quadratic(float a, float b, float c, float tmin, float& tmax) {  // geometry.cpp:20-29
  float d = b * b - 4 * a * c;
  if (d <= 0.0f) return false;
  d = std::sqrt(d);
  float t = (-b - d) / (2 * a);
  if (t < tmin) t += d / a;
  if (t < tmin || t > tmax) return false;
  tmax = t;
  return true;
}

struct Rect {  // geometry.cpp:255-408
  vec3 position, ex, ey, n;
  float lx, ly;
  vec3 rx, ry;
  Rect(vec3 position_, vec3 ex_, vec3 ey_, bool flip) : position(position_) {
    ex = normalize(ex_);
    ey = normalize(ey_);
    n = normalize(cross(ex, ey)) * float(flip ? -1 : 1);
    lx = length(ex_);
    ly = length(ey_);
    rx = ex / lx;
    ry = ey / ly;
  }
  float area() const { return lx * ly; }
  bool hit(const Ray& ray) const {  // :275-286
    float denom = dot(ray.d, n);
    if (denom == 0.0f) return false;
    float t = (dot(position - ray.o, n)) / denom;
    if (t <= ray.tmin || t >= ray.tmax) return false;
    vec3 p = ray(t) - position;
    float u = dot(p, rx);
    if (u < -0.5f || u > 0.5f) return false;
    float v = dot(p, ry);
    if (v < -0.5f || v > 0.5f) return false;
    return true;
  }
  bool intersect(Ray& ray) const {  // :287-299
    float denom = dot(ray.d, n);
    if (denom == 0.0f) return false;
    float t = (dot(position - ray.o, n)) / denom;
    if (t <= ray.tmin || t >= ray.tmax) return false;
    vec3 p = ray(t) - position;
    float u = dot(p, rx);
    if (u < -0.5f || u > 0.5f) return false;
    float v = dot(p, ry);
    if (v < -0.5f || v > 0.5f) return false;
    ray.tmax = t;
    return true;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :300-307
    vec3 rp = p - position;
    float u = dot(rp, rx);
    float v = dot(rp, ry);
    it.p = position + lx * ex * u + ly * ey * v;
    it.n = n;
    it.uv = vec2(u, v) + vec2(0.5f, 0.5f);
  }
  ShapeSample sample(vec3 o, vec2 u) const {  // :308-316
    ShapeSample ss;
    ss.p = position + (u[0] - 0.5f) * ex * lx + (u[1] - 0.5f) * ey * ly;
    ss.n = n;
    ss.uv = u;
    ss.w = normalize(ss.p - o, ss.distance);
    ss.pdf = sqr(ss.distance) / (absdot(ss.w, ss.n) * area());
    return ss;
  }
  float pdf(const Ray& ray, vec3 ns) const {  // :368-370  (NB multiplies by cos -- Appendix A4)
    return sqr(ray.tmax) / area() * absdot(ns, ray.d);
  }
  AABB get_aabb() const {  // :401-408
    AABB b;
    b.extend(position - ex * lx / 2.0f - ey * ly / 2.0f);
    b.extend(position - ex * lx / 2.0f + ey * ly / 2.0f);
    b.extend(position + ex * lx / 2.0f - ey * ly / 2.0f);
    b.extend(position + ex * lx / 2.0f + ey * ly / 2.0f);
    return b;
  }
};

struct OBB {  // bbox.cpp:144-182
  AABB base;
  mat4 m, m_inv;
  OBB(AABB b, mat4 m_) : base(b), m(m_), m_inv(inverse(m_)) {}
  bool hit(Ray ray) const {  // :145-149
    ray.o = m_inv * ray.o;
    ray.d = normalize(to_mat3(m_inv) * ray.d);
    return base.hit(ray);
  }
  bool intersect(vec3 o, vec3 d, float& tmin, float& tmax) const {  // :150-163
    vec3 org = o;
    o = m_inv * o;
    d = normalize(to_mat3(m_inv) * d);
    if (base.intersect(o, d, tmin, tmax)) {
      vec3 ps = o + tmin * d;
      vec3 pe = o + tmax * d;
      tmin = distance(m * ps, org);
      tmax = distance(m * pe, org);
      return true;
    }
    return false;
  }
  bool intersect(Ray& ray) const {  // :164-172
    float tmin = ray.tmin, tmax = ray.tmax;
    if (intersect(ray.o, ray.d, tmin, tmax)) {
      ray.tmax = tmin > ray.tmin ? tmin : tmax;
      return true;
    }
    return false;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :173-177
    base.compute_surface_info(m_inv * p, it);
    it.p = m * it.p;
    it.n = normalize(transpose(to_mat3(m_inv)) * it.n);
  }
  AABB get_aabb() const {  // bbox.cpp:8-16 (no epsilon pad, bbox.h:93)
    AABB r;
    for (int i = 0; i < 8; i++) {
      vec3 p = base.lower;
      if (i % 2 >= 1) p[0] = base.upper[0];
      if (i % 4 >= 2) p[1] = base.upper[1];
      if (i % 8 >= 4) p[2] = base.upper[2];
      r.extend(m * p);
    }
    return r;
  }
};

struct Sphere {  // geometry.cpp:72-121
  vec3 c;
  float r;
  static float compute_t(vec3 ro, vec3 rd, float tmin, vec3 p, float r) {  // :73-83
    vec3 ro_p = ro - p;
    float b = dot(ro_p, rd);
    float c = dot(ro_p, ro_p) - r * r;
    float d = b * b - c;
    if (d <= 0.0f) return -1.0f;
    d = std::sqrt(d);
    float t = -b - d;
    if (t < tmin) t = -b + d;
    return t;
  }
  bool hit(const Ray& ray) const {
    float t = compute_t(ray.o, ray.d, ray.tmin, c, r);
    return t > ray.tmin && t < ray.tmax;
  }
  bool intersect(Ray& ray) const {
    float t = compute_t(ray.o, ray.d, ray.tmin, c, r);
    if (t < ray.tmin || t > ray.tmax) return false;
    ray.tmax = t;
    return true;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :94-98
    it.n = normalize(p - c);
    it.p = c + it.n * r;
    it.uv = cartesian_to_spherical(it.n);
  }
  ShapeSample sample(vec3 p, vec2 u) const {  // :99-114
    ShapeSample ss;
    float l = length(c - p);
    float cos_theta = std::sqrt(1 - sqr(r / l));
    float S = 2 * Pi * (1 - cos_theta);
    float cos_theta_wo = 1 - u.y * (1 - cos_theta);
    float sin_theta_wo = std::sqrt(1 - cos_theta_wo * cos_theta_wo);
    ss.w = spherical_to_cartesian(u.x * 2 * Pi, sin_theta_wo, cos_theta_wo);
    ss.w = coordinate_system((c - p) / l) * ss.w;
    ss.distance = compute_t(p, ss.w, 0.0f, c, r);
    ss.pdf = 1.0f / S;
    ss.p = p + ss.w * ss.distance;
    ss.n = (ss.p - c) / r;
    ss.uv = cartesian_to_spherical(ss.n);
    return ss;
  }
  float pdf(const Ray& ray) const {  // :115-120
    float l = length(c - ray.o);
    float cos_theta = std::sqrt(1 - sqr(r / l));
    float S = 2 * Pi * (1 - cos_theta);
    return 1.0f / S;
  }
  AABB get_aabb() const { return {c - vec3(r), c + vec3(r)}; }
};

struct Disk {  // geometry.cpp:123-169
  vec3 position, n, u, v;
  float r;
  Disk(vec3 p, vec3 normal, float r) : position(p), n(normalize(normal)), r(r) {
    coordinate_system(n, u, v);
  }
  float area() const { return Pi * r * r; }
  bool hit(const Ray& ray) const {  // :128-137
    float denom = dot(ray.d, n);
    if (denom == 0.0f) return false;
    float t = (dot(position, n) - dot(ray.o, n)) / denom;
    if (t < ray.tmin) return false;
    if (t >= ray.tmax) return false;
    vec3 p = ray(t) - position;
    if (length_squared(p) > sqr(r)) return false;
    return true;
  }
  bool intersect(Ray& ray) const {  // :138-148
    float denom = dot(ray.d, n);
    if (denom == 0.0f) return false;
    float t = (dot(position, n) - dot(ray.o, n)) / denom;
    if (t < ray.tmin || t > ray.tmax) return false;
    vec3 p = ray(t) - position;
    if (length_squared(p) > sqr(r)) return false;
    ray.tmax = t;
    return true;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :149-155
    it.n = n;
    float ex = dot(p - position, u);
    float ey = dot(p - position, v);
    it.uv = {ex, ey};
    it.p = position + ex * u + ey * v;
  }
  ShapeSample sample(vec3 p, vec2 u2) const {  // :156-165
    ShapeSample ss;
    vec2 uv = sample_disk_concentric(u2);
    ss.p = position + r * u * uv[0] + r * v * uv[1];
    ss.n = n;
    ss.uv = u2;
    ss.w = normalize(ss.p - p, ss.distance);
    ss.pdf = sqr(ss.distance) / fmax_(absdot(ss.w, ss.n) * area(), kEpsilon);
    return ss;
  }
  float pdf(const Ray& ray, vec3 ns) const {  // :166-168
    return sqr(ray.tmax) / (area() * absdot(ns, ray.d));
  }
  AABB get_aabb() const { return Sphere{position, r}.get_aabb(); }  // :169
};

struct Cone {  // geometry.cpp:409-464, geometry.h:122-142
  Disk bottom;
  vec3 p, n;
  float r, h, A, A2, S;
  Cone(vec3 p_, vec3 n_, float r, float h)
      : bottom(p_, n_, r), p(p_ + n_ * h), n(normalize(n_)), r(r), h(h) {
    A2 = sqr(r / h) + 1;
    A = std::sqrt(A2);
    S = r / std::sqrt(r * r + h * h);
  }
  float area() const { return std::sqrt(r * r + h * h) * Pi * r + bottom.area(); }
  bool hit(const Ray& ray) const {  // :415-427
    vec3 o = ray.o - p;
    const vec3& d = ray.d;
    float a = -A2 * sqr(dot(d, n)) + dot(d, d);
    float b = 2 * (-A2 * dot(o, n) * dot(d, n) + dot(o, d));
    float c = -A2 * sqr(dot(o, n)) + dot(o, o);
    float tmax = ray.tmax;
    return intersect_quadratic(a, b, c, ray.tmin, tmax) && dot(o + tmax * d, n) <= 0;
  }
  bool intersect(Ray& ray) const {  // :428-454
    vec3 o = ray.o - p;
    const vec3& d = ray.d;
    float a = -A2 * sqr(dot(d, n)) + dot(d, d);
    float b = 2 * (-A2 * dot(o, n) * dot(d, n) + dot(o, d));
    float c = -A2 * sqr(dot(o, n)) + dot(o, o);
    float tmax = ray.tmax;
    if (intersect_quadratic(a, b, c, ray.tmin, tmax) && dot(o + tmax * d, n) < 0) {
      ray.tmax = tmax;
      return true;
    }
    return false;
  }
  void compute_surface_info(vec3 ps, SurfaceInteraction& it) const {  // :455-460
    float l = length(ps - p) * A;
    vec3 x = p - n * l;
    it.n = normalize(ps - x);
    it.p = x + it.n * l * S;
  }
  float pdf(const Ray& ray, vec3 ns) const {  // :462-464
    return sqr(ray.tmax) / area() * absdot(ns, ray.d);
  }
  AABB get_aabb() const { return bottom.get_aabb().extend(p); }  // geometry.h:129
};

vec3 uniform_hemisphere(vec2 u) {  // sampling.h:56-62
  const float phi = u.x * Pi * 2;
  const float cos_theta = u.y;
  const float sin_theta = std::sqrt(1.0f - sqr(cos_theta));
  return vec3(sin_theta * std::cos(phi), sin_theta * std::sin(phi), cos_theta);
}

struct Plane {  // geometry.cpp:31-70
  vec3 position, n, u, v;
  Plane(vec3 p, vec3 normal) : position(p), n(normalize(normal)) { coordinate_system(n, u, v); }
  bool hit(const Ray& ray) const {  // :35-39
    float t = (dot(position, n) - dot(ray.o, n)) / dot(ray.d, n);
    if (t <= ray.tmin) return false;
    return t < ray.tmax;
  }
  bool intersect(Ray& ray) const {  // :40-45
    float t = (dot(position, n) - dot(ray.o, n)) / dot(ray.d, n);
    if (t < ray.tmin || t > ray.tmax) return false;
    ray.tmax = t;
    return true;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :46-51
    it.n = n;
    vec3 dp = p - position;
    it.uv = vec2(dot(dp, u), dot(dp, v));
    it.p = position + it.uv.x * u + it.uv.y * v;
  }
  AABB get_aabb() const { return {position + vec3(-100.0f), position + vec3(100.0f)}; }  // :52
  ShapeSample sample(vec3 p, vec2 u2) const {  // :57-69
    ShapeSample ss;
    vec3 p_sphere = uniform_hemisphere(u2);
    float l = absdot(p - position, n);
    float ex = l * p_sphere.x / p_sphere.z;
    float ey = l * p_sphere.y / p_sphere.z;
    vec3 dp = p - position;  // project_to_plane :53-56
    ss.p = (position + u * dot(u, dp) + v * dot(v, dp)) + u * ex + v * ey;
    ss.n = n;
    ss.uv = {ex, ey};
    ss.w = normalize(ss.p - p, ss.distance);
    ss.pdf = 1.0f / (2 * Pi);
    return ss;
  }
  float pdf() const { return 1.0f / (2 * Pi); }  // :70
};

struct Line {  // geometry.cpp:171-244
  vec3 p0, p1;
  mat3 tbn;
  float thickness, len;
  Line(vec3 a, vec3 b, float th)
      : p0(a), p1(b), tbn(coordinate_system(normalize(b - a))), thickness(th), len(length(b - a)) {}
  float area() const { return thickness * 2 * Pi * len; }  // geometry.h:70
  // the closest approach of the segment to the ray axis, in the ray's look_at frame (:181-192, :197-208)
  bool closest(const Ray& ray, float& z) const {
    mat4 r2o = look_at(ray.o, ray.o + ray.d);
    mat4 o2r = inverse(r2o);
    vec3 q0 = o2r * p0;  // mat4 * vec3 and vec3{mat4 * vec4(p,1)} are the same arithmetic (vecmath.h:700-707)
    vec3 q1 = o2r * p1;
    vec3 o = q0;
    vec3 d = q1 - q0;
    // inverse(mat2(dot(d,d), -d.z, -d.z, 1)) * vec2(-dot(o,d), o.z)   (vecmath.h:1079-1087): only .x is used
    float m00 = dot(d, d), m01 = -d.z, m10 = -d.z, m11 = 1.0f;  // m[c][r]
    float det = m00 * m11 - m10 * m01;
    float ix0 = m11 / det, iy0 = -m10 / det;  // row 0 of the inverse: x[0], y[0]
    float b0 = -dot(o, d), b1 = o.z;
    float tzx = ix0 * b0 + iy0 * b1;
    float t = clampf(tzx, 0.0f, 1.0f);
    z = clampf(o.z + t * d.z, ray.tmin + thickness, ray.tmax);
    float D = length(o + t * d - vec3(0.0f, 0.0f, z));
    return D <= thickness;
  }
  bool hit(const Ray& ray) const {
    float z;
    return closest(ray, z);
  }
  bool intersect(Ray& ray) const {
    float z;
    if (!closest(ray, z)) return false;
    ray.tmax = z;
    return true;
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :215-222
    float lt = dot(p - p0, tbn.z);
    vec3 lp = lt * p1 + (1.0f - lt) * p0;  // lerp(lt, p0, p1) vecmath.h:877-880
    it.p = p;
    it.n = normalize(p - lp);
    it.uv = {lt, 0.0f};
  }
  ShapeSample sample(vec3 p, vec2 u2) const {  // :223-233
    ShapeSample ss;
    float phi = u2[1] * 2 * Pi;
    ss.p = (u2[0] * p1 + (1.0f - u2[0]) * p0) + thickness * std::cos(phi) * tbn.x +
           thickness * std::sin(phi) * tbn.y;
    ss.n = std::cos(phi) * tbn.x + std::sin(phi) * tbn.y;
    ss.uv = u2;
    ss.w = normalize(ss.p - p, ss.distance);
    ss.pdf = sqr(ss.distance) / (absdot(ss.w, ss.n) * area());
    return ss;
  }
  float pdf(const Ray& ray, vec3 ns) const {  // :234-236
    return sqr(ray.tmax) / (area() * absdot(ns, ray.d));
  }
  AABB get_aabb() const {  // :237-244
    AABB aabb;
    aabb.extend(p0 - vec3(thickness));
    aabb.extend(p1 - vec3(thickness));
    aabb.extend(p0 + vec3(thickness));
    aabb.extend(p1 + vec3(thickness));
    return aabb;
  }
};

struct Cylinder {  // geometry.h:139-157, geometry.cpp:466-523: lateral surface only, no caps
  vec3 p0, p1, n;
  float r;
  Cylinder(vec3 a, vec3 b, float r) : p0(a), p1(b), n(normalize(b - a)), r(r) {}
  bool solve(const Ray& ray, float& t, vec3& hit_point, vec3& projection) const {  // :467-488 == :491-511
    vec3 m = ray.o - p0;
    vec3 v = ray.d - dot(ray.d, n) * n;
    vec3 w = m - dot(m, n) * n;
    float a = dot(v, v);
    float b = 2 * dot(v, w);
    float c = dot(w, w) - r * r;
    float discriminant = b * b - 4 * a * c;
    if (discriminant < 0) return false;
    float sqrtDisc = std::sqrt(discriminant);
    t = (-b - sqrtDisc) / (2 * a);
    if (t < ray.tmin) t = (-b + sqrtDisc) / (2 * a);
    if (t > ray.tmax) return false;
    hit_point = ray(t);
    projection = p0 + dot(hit_point - p0, n) * n;
    if (dot(projection - p0, n) < 0 || dot(projection - p1, n) > 0) return false;
    return true;
  }
  bool hit(const Ray& ray) const {
    float t;
    vec3 hp, pr;
    return solve(ray, t, hp, pr);
  }
  // Cylinder::intersect writes it.n / it.p itself and compute_surface_info is empty (:512-523); the
  // winning shape's intersect is always the last one that succeeded, so the values it left are the
  // ones recomputed here from the final ray (same t, same ray -> same bits)
  bool intersect(Ray& ray) const {
    float t;
    vec3 hp, pr;
    if (!solve(ray, t, hp, pr)) return false;
    ray.tmax = t;
    return true;
  }
  void compute_surface_info(vec3 hit_point, SurfaceInteraction& it) const {
    vec3 projection = p0 + dot(hit_point - p0, n) * n;
    it.n = normalize(hit_point - projection);
    it.p = hit_point;
  }
  // bottom(p0,-n,r), top(p0,n,r): both cap disks sit at p0 (geometry.h:141), so the box ignores p1
  AABB get_aabb() const { return union_(Disk(p0, -n, r).get_aabb(), Disk(p0, n, r).get_aabb()); }
};

struct Tri {  // geometry.cpp:525-599 (static helpers)
  static bool hit(const Ray& ray, vec3 v0, vec3 v1, vec3 v2) {  // :532-547
    vec3 E1 = v1 - v0, E2 = v2 - v0, T = ray.o - v0;
    vec3 P = cross(ray.d, E2), Q = cross(T, E1);
    float D = dot(P, E1);
    if (D == 0.0f) return false;
    float t = dot(Q, E2) / D;
    if (t < ray.tmin || t > ray.tmax) return false;
    float u = dot(P, T) / D;
    if (u < 0.0f || u > 1.0f) return false;
    float v = dot(Q, ray.d) / D;
    if (v < 0.0f || v > 1.0f) return false;
    return u + v < 1.0f;
  }
  static bool intersect(Ray& ray, vec3 v0, vec3 v1, vec3 v2) {  // :548-565
    vec3 E1 = v1 - v0, E2 = v2 - v0, T = ray.o - v0;
    vec3 P = cross(ray.d, E2), Q = cross(T, E1);
    float D = dot(P, E1);
    if (D == 0.0f) return false;
    float t = dot(Q, E2) / D;
    if (t <= ray.tmin || t >= ray.tmax) return false;
    float u = dot(P, T) / D;
    if (u < 0.0f || u > 1.0f) return false;
    float v = dot(Q, ray.d) / D;
    if (v < 0.0f || v > 1.0f) return false;
    if (u + v > 1.0f) return false;
    ray.tmax = t;
    return true;
  }
};

struct Triangle {  // the stand-alone shape, geometry.cpp:525-595
  vec3 v0, v1, v2, n;
  Triangle(vec3 a, vec3 b, vec3 c) : v0(a), v1(b), v2(c), n(normalize(cross(a - b, a - c))) {
    if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) n = vec3(0, 0, 1);
  }
  float area() const { return length(cross(v1 - v0, v2 - v0)) / 2; }  // geometry.h:113
  bool hit(const Ray& ray) const { return Tri::hit(ray, v0, v1, v2); }
  bool intersect(Ray& ray) const { return Tri::intersect(ray, v0, v1, v2); }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {  // :568-574 (uv are plain dot products)
    float u = dot(p - v0, v1 - v0);
    float v = dot(p - v0, v2 - v0);
    it.uv = vec2(u, v);
    it.p = lerp3(it.uv[0], it.uv[1], v0, v1, v2);
    it.n = n;
  }
  ShapeSample sample(vec3 p, vec2 u) const {  // :575-584
    ShapeSample ss;
    if (u.x + u.y > 1.0f) u = vec2(1.0f, 1.0f) - u;
    ss.p = lerp3(u.x, u.y, v0, v1, v2);
    ss.n = n;
    ss.uv = u;
    ss.w = normalize(ss.p - p, ss.distance);
    ss.pdf = sqr(ss.distance) / fmax_(absdot(ss.w, ss.n) * area(), kEpsilon);
    return ss;
  }
  float pdf(const Ray& ray, vec3 ns) const {  // :585-587
    return sqr(ray.tmax) / (area() * absdot(ns, ray.d));
  }
  AABB get_aabb() const {  // :588-594
    AABB aabb;
    aabb.extend(v0);
    aabb.extend(v1);
    aabb.extend(v2);
    return aabb;
  }
};

struct BVHImpl;
struct Mesh {  // geometry.h:158-232, geometry.cpp:601-650
  std::vector<vec3> vertices;
  std::vector<vec3> normals;      // per vertex, or empty (geometry.h:215)
  std::vector<vec2> texcoords;    // per vertex, or empty (:216)
  std::vector<uint32_t> indices;  // 3 per face
  std::shared_ptr<BVHImpl> bvh;   // per-mesh BVH (bvh.cpp:459-475 == ShapeBVH, :549-567)
  size_t num_triangles() const { return indices.size() / 3; }
  void face(size_t i, vec3& a, vec3& b, vec3& c) const {
    a = vertices[indices[3 * i]];
    b = vertices[indices[3 * i + 1]];
    c = vertices[indices[3 * i + 2]];
  }
  bool hit(const Ray& ray, int i) const {
    vec3 a, b, c;
    face(i, a, b, c);
    return Tri::hit(ray, a, b, c);
  }
  bool intersect(Ray& ray, int i) const {
    vec3 a, b, c;
    face(i, a, b, c);
    return Tri::intersect(ray, a, b, c);
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it, int i) const {  // :632-646
    vec3 v0, v1, v2;
    face(i, v0, v1, v2);
    vec3 e1 = v1 - v0, e2 = v2 - v0;
    it.n = cross(e1, e2);
    mat3 tbn = inverse(mat3(e1, e2, it.n));
    vec3 q = tbn * (p - v0);
    it.uv = vec2(q.x, q.y);
    it.p = lerp3(it.uv[0], it.uv[1], v0, v1, v2);
    if (!normals.empty())  // normal_of geometry.h:199-204
      it.n = normalize(lerp3(it.uv[0], it.uv[1], normals[indices[3 * i]], normals[indices[3 * i + 1]], normals[indices[3 * i + 2]]));
    else
      it.n = normalize(it.n);
    if (!texcoords.empty()) {  // texcoord_of :205-210 (read with the barycentric uv)
      const float u = it.uv[0], v = it.uv[1];
      const vec2 a = texcoords[indices[3 * i]], b = texcoords[indices[3 * i + 1]], c = texcoords[indices[3 * i + 2]];
      it.uv = vec2((1.0f - u - v) * a.x + u * b.x + v * c.x, (1.0f - u - v) * a.y + u * b.y + v * c.y);
    }
  }
  AABB get_aabb(size_t i) const {  // :647-652
    vec3 a, b, c;
    face(i, a, b, c);
    AABB r;
    r.extend(a);
    r.extend(b);
    r.extend(c);
    return r;
  }
  float tri_area(size_t i) const {  // geometry.h:118
    vec3 a, b, c;
    face(i, a, b, c);
    return length(cross(b - a, c - a)) / 2;
  }
  float area() const { return tri_area(0) * num_triangles(); }  // geometry.h:167-169 (quirk A4)
  float pdf(const Ray& ray, vec3 ns) const {                    // geometry.h:180-182
    return sqr(ray.tmax) / (area() * absdot(ns, ray.d));
  }
  ShapeSample sample_tri(size_t i, vec3 p, vec2 u) const {  // Triangle::sample geometry.cpp:575-584
    vec3 v0, v1, v2;
    face(i, v0, v1, v2);
    vec3 n = normalize(cross(v0 - v1, v0 - v2));  // Triangle(v0,v1,v2) ctor :528-531
    if (n.is_zero()) n = vec3(0, 0, 1);
    ShapeSample ss;
    if (u.x + u.y > 1.0f) u = vec2(1.0f, 1.0f) - u;
    ss.p = lerp3(u.x, u.y, v0, v1, v2);
    ss.n = n;
    ss.uv = u;
    ss.w = normalize(ss.p - p, ss.distance);
    float a = length(cross(v1 - v0, v2 - v0)) / 2;
    ss.pdf = sqr(ss.distance) / fmax_(absdot(ss.w, ss.n) * a, kEpsilon);
    return ss;
  }
};

// ------------------------------------------------------------------------------------------------
// Materials / BXDFs (material.h, material.cpp, bxdf.h, bxdf.cpp, scattering.h)
// ------------------------------------------------------------------------------------------------
inline float CosTheta(vec3 w) { return w.z; }
inline float Cos2Theta(vec3 w) { return sqr(w.z); }
inline float AbsCosTheta(vec3 w) { return std::abs(w.z); }
inline float Sin2Theta(vec3 w) { return 1.0f - Cos2Theta(w); }
inline float SinTheta(vec3 w) { return std::sqrt(Sin2Theta(w)); }
inline float Tan2Theta(vec3 w) { return Sin2Theta(w) / fmax_(Cos2Theta(w), kEpsilon); }
inline float CosPhi(vec3 w) {
  float s = SinTheta(w);
  return (s == 0) ? 1 : clampf(w.x / s, -1.0f, 1.0f);
}
inline float SinPhi(vec3 w) {
  float s = SinTheta(w);
  return (s == 0) ? 1 : clampf(w.y / s, -1.0f, 1.0f);
}
inline bool SameHemisphere(vec3 a, vec3 b) { return a.z * b.z > 0.0f; }
inline vec3 FaceNormal(vec3 v) { return v.z < 0.0f ? -v : v; }
inline vec3 Reflect(vec3 w) { return vec3(-w.x, -w.y, w.z); }
inline vec3 Reflect(vec3 wi, vec3 n) { return 2.0f * dot(wi, n) * n - wi; }
bool Refract(vec3 wi, vec3 n, float eta, vec3& wt, float* etap = nullptr) {  // scattering.h:58-77
  float cosThetaI = dot(n, wi);
  if (cosThetaI < 0) {
    eta = 1.0f / eta;
    cosThetaI = -cosThetaI;
    n = -n;
  }
  float sin2ThetaI = fmax_(0.0f, 1.0f - sqr(cosThetaI));
  float sin2ThetaT = sin2ThetaI / sqr(eta);
  if (sin2ThetaT >= 1) return false;
  float cosThetaT = std::sqrt(1.0f - sin2ThetaT);
  wt = -wi / eta + (cosThetaI / eta - cosThetaT) * n;
  if (etap) *etap = eta;
  return true;
}
float FrDielectric(float cosThetaI, float eta) {  // scattering.h:79-94
  if (cosThetaI < 0) {
    eta = 1 / eta;
    cosThetaI = -cosThetaI;
  }
  float sin2ThetaI = 1.0f - sqr(cosThetaI);
  float sin2ThetaT = sin2ThetaI / sqr(eta);
  if (sin2ThetaT >= 1.0f) return 1.0f;
  float cosThetaT = std::sqrt(1.0f - sin2ThetaT);
  float rParl = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
  float rPerp = (cosThetaI - eta * cosThetaT) / (cosThetaI + eta * cosThetaT);
  return (sqr(rParl) + sqr(rPerp)) / 2.0f;
}
vec3 FrSchlick(vec3 F0, float cosTheta) {  // scattering.h:96-98
  return F0 + (vec3(1.0f) - F0) * std::pow(1.0f - cosTheta, 5.0f);
}
struct TRDist {  // scattering.h:100-150
  float ax, ay;
  float D(vec3 wm) const {
    float tan2Theta = Tan2Theta(wm);
    float cos4Theta = sqr(Cos2Theta(wm));
    if (cos4Theta < 1e-6f) return 0.0f;
    float e = tan2Theta * (sqr(CosPhi(wm) / ax) + sqr(SinPhi(wm) / ay));
    return 1.0f / (Pi * ax * ay * cos4Theta * sqr(1 + e));
  }
  float Lambda(vec3 w) const {
    float tan2Theta = Tan2Theta(w);
    float alpha2 = sqr(CosPhi(w) * ax) + sqr(SinPhi(w) * ay);
    return (std::sqrt(1.0f + alpha2 * tan2Theta) - 1.0f) / 2.0f;
  }
  float G1(vec3 w) const { return 1.0f / (1.0f + Lambda(w)); }
  float G(vec3 wi, vec3 wo) const { return 1.0f / (1.0f + Lambda(wi) + Lambda(wo)); }
  float D_G(vec3 wi, vec3 wm, vec3 wo) const { return D(wm) * G(wi, wo); }
  float D(vec3 w, vec3 wm) const { return G1(w) / AbsCosTheta(w) * D(wm) * absdot(w, wm); }
  float pdf(vec3 w, vec3 wm) const { return fmax_(D(w, wm), kEpsilon); }
  vec3 SampleWm(vec3 w, vec2 u) const {
    vec3 wh = normalize(vec3(ax * w.x, ay * w.y, w.z));
    if (wh.z < 0.0f) wh = -wh;
    vec3 T1 = (wh.z < 0.99999f) ? normalize(cross(vec3(0, 0, 1), wh)) : vec3(1, 0, 0);
    vec3 T2 = cross(wh, T1);
    vec2 p = sample_disk_polar(u);
    float h = std::sqrt(1.0f - sqr(p.x));
    // psl::lerp(t, a, b) = a * (1 - t) + b * t (src/psl/math.h:118-121)
    float t = (1.0f + wh.z) / 2;
    p.y = h * (1.0f - t) + p.y * t;
    float pz = std::sqrt(fmax_(0.0f, 1.0f - (p.x * p.x + p.y * p.y)));
    vec3 nh = p.x * T1 + p.y * T2 + pz * wh;
    return normalize(vec3(ax * nh.x, ay * nh.y, fmax_(1e-6f, nh.z)));
  }
};

struct BSDFSample {
  vec3 wo, f;
  float pdf = 0.0f;
  bool is_delta = false;
};
enum BxdfKind { BX_DIFFUSE, BX_CONDUCTOR, BX_REFRACTIVE, BX_REFR_DIEL, BX_DIFF_DIEL, BX_BSSRDF };
struct BXDF {  // bxdf.h:36-157 flattened into one tagged struct
  BxdfKind kind = BX_DIFFUSE;
  vec3 albedo;
  float roughness = 0, ior = 1;
  vec3 sigma_s;
  vec3 wi;  // local
  bool is_delta() const {
    switch (kind) {
      case BX_DIFFUSE: case BX_DIFF_DIEL: case BX_BSSRDF: return false;
      default: return roughness < 1e-2f;
    }
  }
  bool sample(Sampler& sampler, BSDFSample& bs) const;
  vec3 f(vec3 wo) const;
  float pdf(vec3 wo) const;
};
bool BXDF::sample(Sampler& sampler, BSDFSample& bs) const {
  switch (kind) {
    case BX_DIFFUSE: {  // bxdf.cpp:11-23
      vec3 wo = cosine_weighted_hemisphere(sampler.get2d());
      if (CosTheta(wi) < 0) wo = -wo;
      bs.wo = wo;
      bs.pdf = AbsCosTheta(bs.wo) / Pi;
      bs.f = albedo / Pi;
      return true;
    }
    case BX_CONDUCTOR: {  // bxdf.cpp:39-64
      float alpha = sqr(roughness);
      if (alpha < 1e-4f) {
        bs.wo = Reflect(wi);
        bs.f = FrSchlick(albedo, AbsCosTheta(bs.wo)) / AbsCosTheta(bs.wo);
        bs.pdf = 1.0f;
        bs.is_delta = true;
        return true;
      }
      TRDist distrib{alpha, alpha};
      vec3 wm = distrib.SampleWm(wi, sampler.get2d());
      vec3 wo = Reflect(wi, wm);
      if (!SameHemisphere(wi, wo)) return false;
      vec3 fr = FrSchlick(albedo, absdot(wi, wm));
      bs.wo = wo;
      bs.pdf = distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
      bs.f = fr * (distrib.D_G(wo, wm, wi) / (4 * CosTheta(wi) * CosTheta(wo)));
      return true;
    }
    case BX_REFRACTIVE: {  // bxdf.cpp:102-124
      float alpha = sqr(roughness);
      if (alpha < 1e-4f) {
        bs.wo = Reflect(wi);
        bs.f = albedo;
        bs.pdf = AbsCosTheta(bs.wo);
        bs.is_delta = true;
        return true;
      }
      TRDist distrib{alpha, alpha};
      vec3 wm = distrib.SampleWm(wi, sampler.get2d());
      vec3 wo = Reflect(wi, wm);
      if (!SameHemisphere(wi, wo)) return false;
      bs.wo = wo;
      bs.pdf = distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
      bs.f = albedo * (distrib.D_G(wo, wm, wi) / (4 * CosTheta(wi) * CosTheta(wo)));
      return true;
    }
    case BX_REFR_DIEL: {  // bxdf.cpp:162-208
      float fr = FrDielectric(CosTheta(wi), ior);
      float alpha = sqr(roughness);
      if (alpha < 1e-4f) {
        if (sampler.get1d() < fr) {
          bs.wo = Reflect(wi);
          bs.f = albedo * (fr / AbsCosTheta(bs.wo));
          bs.pdf = fr;
          bs.is_delta = true;
        } else {
          if (!Refract(wi, vec3(0, 0, 1), ior, bs.wo)) return false;
          bs.f = albedo * ((1 - fr) / AbsCosTheta(bs.wo));
          bs.pdf = 1 - fr;
          bs.is_delta = true;
        }
        return true;
      }
      TRDist distrib{alpha, alpha};
      vec3 wm = distrib.SampleWm(wi, sampler.get2d());
      if (sampler.get1d() < fr) {
        vec3 wo = Reflect(wi, wm);
        if (!SameHemisphere(wi, wo)) return false;
        bs.wo = wo;
        bs.pdf = fr * distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
        bs.f = albedo * (fr * distrib.D_G(wo, wm, wi) / (4 * CosTheta(wi) * CosTheta(wo)));
      } else {
        float eta = 1.0f;
        if (!Refract(wi, wm, ior, bs.wo, &eta)) return false;
        const vec3& wo = bs.wo;
        float denom = sqr(dot(wo, wm) + dot(wi, wm) / eta);
        bs.pdf = (1 - fr) * distrib.pdf(wi, wm) * absdot(wo, wm) / denom;
        bs.f = albedo * ((1 - fr) * distrib.D(wm) * distrib.G(wi, wo) *
                         std::abs(dot(wo, wm) * dot(wi, wm) / (denom * CosTheta(wi) * CosTheta(wo))));
      }
      return true;
    }
    case BX_DIFF_DIEL: {  // bxdf.cpp:250-287
      float fr = FrDielectric(CosTheta(wi), ior);
      float alpha = sqr(roughness);
      if (alpha < 1e-4f) {
        if (sampler.get1d() < fr) {
          bs.wo = Reflect(wi);
          bs.f = vec3(fr);
          bs.pdf = fr * AbsCosTheta(bs.wo);
          bs.is_delta = true;
        } else {
          bs.wo = cosine_weighted_hemisphere(sampler.get2d());
          bs.f = albedo * ((1 - fr) / Pi);
          bs.pdf = (1 - fr) * AbsCosTheta(bs.wo) / Pi;
        }
        return true;
      }
      TRDist distrib{alpha, alpha};
      vec3 wm = distrib.SampleWm(wi, sampler.get2d());
      if (sampler.get1d() < fr) {
        vec3 wo = Reflect(wi, wm);
        if (!SameHemisphere(wi, wo)) return false;
        bs.wo = wo;
        bs.f = vec3(fr * distrib.D_G(wi, wm, wo) / (4 * CosTheta(wi) * CosTheta(wo)));
        bs.pdf = fr * distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
      } else {
        bs.wo = cosine_weighted_hemisphere(sampler.get2d());
        bs.f = albedo * ((1 - fr) / Pi);
        bs.pdf = AbsCosTheta(bs.wo) * (1 - fr) / Pi;
      }
      return true;
    }
    case BX_BSSRDF: {  // bxdf.cpp:356-367
      vec3 wo = cosine_weighted_hemisphere(sampler.get2d());
      if (CosTheta(wi) > 0) wo = -wo;
      bs.wo = wo;
      bs.pdf = AbsCosTheta(bs.wo) / Pi;
      bs.f = albedo / Pi;
      return true;
    }
  }
  return false;
}
vec3 BXDF::f(vec3 wo) const {
  switch (kind) {
    case BX_DIFFUSE:  // bxdf.cpp:24-28
      if (!SameHemisphere(wi, wo)) return vec3(0.0f);
      return albedo / Pi;
    case BX_CONDUCTOR: {  // bxdf.cpp:65-79
      if (!SameHemisphere(wi, wo)) return {};
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      vec3 wm = normalize(wi + wo);
      if (wm.is_zero()) return {};
      vec3 fr = FrSchlick(albedo, absdot(wi, wm));
      return fr * (distrib.D_G(wo, wm, wi) / (4 * AbsCosTheta(wo) * AbsCosTheta(wi)));
    }
    case BX_REFRACTIVE: {  // bxdf.cpp:125-140
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      bool reflect = cosThetaI * cosThetaO > 0;
      if (!reflect) return {};
      vec3 wm = FaceNormal(normalize(wo + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return {};
      return albedo * (distrib.D_G(wi, wm, wo) / std::abs(4 * cosThetaI * cosThetaO));
    }
    case BX_REFR_DIEL: {  // bxdf.cpp:209-230  (NB `auto eta = 1` is an int there)
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      bool reflect = cosThetaI * cosThetaO > 0;
      int eta = 1;
      if (!reflect) eta = int(cosThetaI > 0 ? ior : 1 / ior);
      vec3 wm = FaceNormal(normalize(wo * float(eta) + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return {};
      float fr = FrDielectric(dot(wi, wm), ior);
      if (reflect) {
        return albedo * (fr * distrib.D_G(wi, wm, wo) / std::abs(4 * cosThetaI * cosThetaO));
      } else {
        float denom = sqr(dot(wo, wm) + dot(wi, wm) / eta) * cosThetaI * cosThetaO;
        return albedo * ((1 - fr) * distrib.D(wm) * distrib.G(wi, wo) *
                         std::abs(dot(wo, wm) * dot(wi, wm) / denom));
      }
    }
    case BX_DIFF_DIEL: {  // bxdf.cpp:288-306
      if (!SameHemisphere(wi, wo)) return {};
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      vec3 wm = FaceNormal(normalize(wo + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return {};
      float fr = FrDielectric(dot(wi, wm), ior);
      vec3 diffused = albedo * (1 - fr) / Pi;
      if (alpha < 1e-4f) return diffused;
      float reflected = fr * distrib.D_G(wo, wm, wi) / std::abs(4 * cosThetaI * cosThetaO);
      return vec3(reflected) + diffused;
    }
    case BX_BSSRDF:  // bxdf.cpp:368-370
      return albedo / Pi;
  }
  return {};
}
float BXDF::pdf(vec3 wo) const {
  switch (kind) {
    case BX_DIFFUSE:  // bxdf.cpp:29-33
      if (!SameHemisphere(wi, wo)) return 0.0f;
      return AbsCosTheta(wo) / Pi;
    case BX_CONDUCTOR: {  // bxdf.cpp:80-95
      if (!SameHemisphere(wi, wo)) return 0.0f;
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      vec3 wm = normalize(wi + wo);
      if (wm.is_zero()) return 0.0f;
      wm = FaceNormal(wm);
      return distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
    }
    case BX_REFRACTIVE: {  // bxdf.cpp:141-157
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      bool reflect = cosThetaI * cosThetaO > 0;
      if (!reflect) return 0.0f;
      vec3 wm = FaceNormal(normalize(wo + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return 0.0f;
      return distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
    }
    case BX_REFR_DIEL: {  // bxdf.cpp:231-245
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      bool reflect = cosThetaI * cosThetaO > 0;
      int eta = 1;
      if (!reflect) eta = int(cosThetaI > 0 ? ior : 1 / ior);
      vec3 wm = FaceNormal(normalize(wo * float(eta) + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return 0.0f;
      float fr = FrDielectric(dot(wi, wm), ior);
      if (reflect) {
        return fr * distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
      } else {
        float denom = sqr(dot(wo, wm) + dot(wi, wm) / eta);
        float dwm_dwo = absdot(wo, wm) / denom;
        return (1 - fr) * distrib.pdf(wi, wm) * dwm_dwo;
      }
    }
    case BX_DIFF_DIEL: {  // bxdf.cpp:307-324
      if (!SameHemisphere(wi, wo)) return 0.0f;
      float alpha = sqr(roughness);
      TRDist distrib{alpha, alpha};
      float cosThetaO = CosTheta(wo), cosThetaI = CosTheta(wi);
      vec3 wm = FaceNormal(normalize(wo + wi));
      if (dot(wm, wo) * cosThetaO <= 0 || dot(wm, wi) * cosThetaI <= 0) return 0.0f;
      float fr = FrDielectric(dot(wi, wm), ior);
      float pt = (1 - fr) * AbsCosTheta(wo) / Pi;
      if (alpha < 1e-4f) return pt;
      float pr = fr * distrib.pdf(wi, wm) / (4 * absdot(wi, wm));
      return pr + pt;
    }
    case BX_BSSRDF:  // bxdf.cpp:371-373
      return AbsCosTheta(wo) / Pi;
  }
  return 0.0f;
}

// Shading nodes (node.h:13-297): a node table in creation order; a material parameter is either a
// literal or a node id.  Evaluation recurses over the tree exactly as Mnode<T>::operator() does.
struct NodeEvalCtx {
  vec3 p, n;
  vec2 uv;
};
struct ShadingNode {
  enum Kind { ConstF, Const3, Position, Normal, UV, BinF, Bin3, UnF, Un3, Comp, ToVec3, Checker, Splat } kind = ConstF;
  char op = 0;
  int a = -1, b = -1, c = -1, n = 0;
  float f = 0;  // ConstF value / Checkerboard ratio
  vec3 v;
};
struct NodeTable {
  std::vector<ShadingNode> nodes;
  static float un(char op, float x) {  // NodeUnary::eval node.h:158-175
    switch (op) {
      case '-': return -x;
      case 'a': return std::abs(x);
      case 's': return x * x;
      case 'r': return std::sqrt(x);
      default: return x - std::floor(x);  // 'f': psl::fract math.h:152-154
    }
  }
  static float bin(char op, float x, float y) {  // NodeBinary::eval node.h:134-150
    switch (op) {
      case '+': return x + y;
      case '-': return x - y;
      case '*': return x * y;
      case '/': return x / y;
      default: return std::pow(x, y);  // psl::pow == std::pow (math.h:201-202)
    }
  }
  float evalf(int id, const NodeEvalCtx& c) const {
    const ShadingNode& k = nodes[size_t(id)];
    switch (k.kind) {
      case ShadingNode::ConstF: return k.f;
      case ShadingNode::BinF: return bin(k.op, evalf(k.a, c), evalf(k.b, c));
      case ShadingNode::UnF: return un(k.op, evalf(k.a, c));
      case ShadingNode::Comp: return eval3(k.a, c)[k.n];
      case ShadingNode::Checker: {  // node.cpp:15-18
        const vec3 q = eval3(k.a, c);
        const vec3 x = vec3(un('f', q.x), un('f', q.y), un('f', q.z)) - vec3(k.f, k.f, k.f);
        return float(x.x * x.y * x.z > 0);
      }
      default: return 0.0f;
    }
  }
  vec3 eval3(int id, const NodeEvalCtx& c) const {
    const ShadingNode& k = nodes[size_t(id)];
    switch (k.kind) {
      case ShadingNode::Const3: return k.v;
      case ShadingNode::Position: return c.p;
      case ShadingNode::Normal: return c.n;
      case ShadingNode::UV: return vec3(c.uv.x, c.uv.y, 0.0f);  // explicit Vector3(Vector2) vecmath.h:167
      case ShadingNode::Bin3: {
        const vec3 x = eval3(k.a, c), y = eval3(k.b, c);
        return vec3(bin(k.op, x.x, y.x), bin(k.op, x.y, y.y), bin(k.op, x.z, y.z));
      }
      case ShadingNode::Un3: {
        const vec3 x = eval3(k.a, c);
        return vec3(un(k.op, x.x), un(k.op, x.y), un(k.op, x.z));
      }
      case ShadingNode::ToVec3: {  // node.h:197-208
        const float x = evalf(k.a, c);
        if (k.b < 0) return vec3(x, x, x);
        return vec3(x, evalf(k.b, c), evalf(k.c, c));
      }
      case ShadingNode::Splat: {  // a Nodef held by a Node3f: vec3{x.eval(nc)} (node.h:291-293)
        const float x = evalf(k.a, c);
        return vec3(x, x, x);
      }
      default: return vec3(0.0f, 0.0f, 0.0f);
    }
  }
};

enum MatKind { M_EMISSIVE, M_DIFFUSE, M_UBER, M_SUBSURFACE, M_METAL, M_GLOSSY, M_GLASS };
struct Material {
  MatKind kind = M_DIFFUSE;
  vec3 color;  // albedo / emission
  float roughness = 0, metallic = 0, transmission = 0, ior = 1.45f;
  vec3 sigma_s;
  // node ids (>= 0) overriding the literals above: albedo (Node3f), roughness / metallic /
  // transmission / ior (Nodef)
  int n_albedo = -1, n_rough = -1, n_metal = -1, n_trans = -1, n_ior = -1;
  const NodeTable* table = nullptr;
  vec3 albedo_at(const NodeEvalCtx& c) const { return n_albedo >= 0 ? table->eval3(n_albedo, c) : color; }
  float roughness_at(const NodeEvalCtx& c) const { return n_rough >= 0 ? table->evalf(n_rough, c) : roughness; }
  float metallic_at(const NodeEvalCtx& c) const { return n_metal >= 0 ? table->evalf(n_metal, c) : metallic; }
  float transmission_at(const NodeEvalCtx& c) const { return n_trans >= 0 ? table->evalf(n_trans, c) : transmission; }
  float ior_at(const NodeEvalCtx& c) const { return n_ior >= 0 ? table->evalf(n_ior, c) : ior; }
};

// Material::sample_bxdf without the frame (material.h:30-131, material.cpp:9-28): the lobe a material answers with at a
// surface point.  BxdfSampleCtx (bxdf.h:10-21): min_roughness only once diffused.
BXDF material_sample_bxdf(const Material& mat, const NodeEvalCtx& nc, vec3 wi, vec3 n, bool diffused, Sampler& sampler) {
  const float min_roughness = diffused ? 0.6f : 0.0f;
  BXDF bxdf;
  switch (mat.kind) {  // material.h:30-131, material.cpp:9-28
    case M_DIFFUSE:
      bxdf.kind = BX_DIFFUSE;
      bxdf.albedo = mat.albedo_at(nc);
      break;
    case M_METAL:  // material.h:39-50
      bxdf.kind = BX_CONDUCTOR;
      bxdf.albedo = mat.albedo_at(nc);
      bxdf.roughness = fmax_(mat.roughness_at(nc), min_roughness);
      break;
    case M_GLOSSY:  // material.h:52-64
      bxdf.kind = BX_DIFF_DIEL;
      bxdf.albedo = mat.albedo_at(nc);
      bxdf.roughness = fmax_(mat.roughness_at(nc), min_roughness);
      bxdf.ior = mat.ior_at(nc);
      break;
    case M_GLASS:  // material.h:66-78
      bxdf.kind = BX_REFR_DIEL;
      bxdf.albedo = mat.albedo_at(nc);
      bxdf.roughness = fmax_(mat.roughness_at(nc), min_roughness);
      bxdf.ior = mat.ior_at(nc);
      break;
    case M_UBER:
      if (with_probability(mat.metallic_at(nc), sampler)) {
        bxdf.kind = BX_CONDUCTOR;
        bxdf.albedo = mat.albedo_at(nc);
        bxdf.roughness = mat.roughness_at(nc);
      } else if (with_probability(mat.transmission_at(nc), sampler)) {
        bxdf.kind = BX_REFR_DIEL;
        bxdf.albedo = mat.albedo_at(nc);
        bxdf.roughness = mat.roughness_at(nc);
        bxdf.ior = mat.ior;
      } else {
        bxdf.kind = BX_DIFF_DIEL;
        bxdf.albedo = mat.albedo_at(nc);
        bxdf.roughness = mat.roughness_at(nc);
        bxdf.ior = mat.ior;
      }
      break;
    case M_SUBSURFACE: {
      const float ior = 1.4f;  // material.h:110
      float fr = FrDielectric(dot(wi, n), ior);
      if (sampler.get1d() < fr) {
        bxdf.kind = BX_REFRACTIVE;
        bxdf.albedo = mat.color;
        bxdf.roughness = fmax_(mat.roughness, min_roughness);
        bxdf.ior = ior;
      } else if (diffused) {
        bxdf.kind = BX_DIFFUSE;
        bxdf.albedo = mat.color;
      } else {
        bxdf.kind = BX_BSSRDF;
        bxdf.albedo = mat.color;
        bxdf.ior = ior;
        bxdf.sigma_s = mat.sigma_s;
      }
      break;
    }
    default: break;
  }
  return bxdf;
}

// ------------------------------------------------------------------------------------------------
// Geometry variant + Scene
// ------------------------------------------------------------------------------------------------
enum ShapeKind { S_RECT, S_AABB, S_OBB, S_SPHERE, S_DISK, S_CONE, S_MESH, S_PLANE, S_LINE, S_CYLINDER, S_TRIANGLE };
struct Geometry {
  ShapeKind kind;
  std::shared_ptr<void> impl;
  int material = -1;
  template <class T> const T& as() const { return *static_cast<const T*>(impl.get()); }
  bool hit(const Ray& r) const {
    switch (kind) {
      case S_RECT: return as<Rect>().hit(r);
      case S_AABB: return as<AABB>().hit(r);
      case S_OBB: return as<OBB>().hit(r);
      case S_SPHERE: return as<Sphere>().hit(r);
      case S_DISK: return as<Disk>().hit(r);
      case S_CONE: return as<Cone>().hit(r);
      case S_PLANE: return as<Plane>().hit(r);
      case S_LINE: return as<Line>().hit(r);
      case S_CYLINDER: return as<Cylinder>().hit(r);
      case S_TRIANGLE: return as<Triangle>().hit(r);
      default: return false;
    }
  }
  bool intersect(Ray& r) const {
    switch (kind) {
      case S_RECT: return as<Rect>().intersect(r);
      case S_AABB: return as<AABB>().intersect(r);
      case S_OBB: return as<OBB>().intersect(r);
      case S_SPHERE: return as<Sphere>().intersect(r);
      case S_DISK: return as<Disk>().intersect(r);
      case S_CONE: return as<Cone>().intersect(r);
      case S_PLANE: return as<Plane>().intersect(r);
      case S_LINE: return as<Line>().intersect(r);
      case S_CYLINDER: return as<Cylinder>().intersect(r);
      case S_TRIANGLE: return as<Triangle>().intersect(r);
      default: return false;
    }
  }
  void compute_surface_info(vec3 p, SurfaceInteraction& it) const {
    switch (kind) {
      case S_RECT: as<Rect>().compute_surface_info(p, it); break;
      case S_AABB: as<AABB>().compute_surface_info(p, it); break;
      case S_OBB: as<OBB>().compute_surface_info(p, it); break;
      case S_SPHERE: as<Sphere>().compute_surface_info(p, it); break;
      case S_DISK: as<Disk>().compute_surface_info(p, it); break;
      case S_CONE: as<Cone>().compute_surface_info(p, it); break;
      case S_PLANE: as<Plane>().compute_surface_info(p, it); break;
      case S_LINE: as<Line>().compute_surface_info(p, it); break;
      case S_CYLINDER: as<Cylinder>().compute_surface_info(p, it); break;
      case S_TRIANGLE: as<Triangle>().compute_surface_info(p, it); break;
      default: break;
    }
  }
  AABB get_aabb() const {
    switch (kind) {
      case S_RECT: return as<Rect>().get_aabb();
      case S_AABB: { AABB b = as<AABB>(); return b.extend_by(kEpsilon); }  // bbox.h:77
      case S_OBB: return as<OBB>().get_aabb();
      case S_SPHERE: return as<Sphere>().get_aabb();
      case S_DISK: return as<Disk>().get_aabb();
      case S_CONE: return as<Cone>().get_aabb();
      case S_PLANE: return as<Plane>().get_aabb();
      case S_LINE: return as<Line>().get_aabb();
      case S_CYLINDER: return as<Cylinder>().get_aabb();
      case S_TRIANGLE: return as<Triangle>().get_aabb();
      default: return AABB();
    }
  }
  // Shape::sample (geometry.h:331-340): nullopt if pdf <= 0 or inf
  bool sample(vec3 p, vec2 u, float u1, ShapeSample& ss) const {
    switch (kind) {
      case S_RECT: ss = as<Rect>().sample(p, u); break;
      case S_SPHERE: ss = as<Sphere>().sample(p, u); break;
      case S_DISK: ss = as<Disk>().sample(p, u); break;
      case S_PLANE: ss = as<Plane>().sample(p, u); break;
      case S_LINE: ss = as<Line>().sample(p, u); break;
      case S_TRIANGLE: ss = as<Triangle>().sample(p, u); break;
      case S_MESH: {  // geometry.h:170-178
        const Mesh& m = as<Mesh>();
        if (m.num_triangles() == 0) return false;
        ss = m.sample_tri(size_t(int(m.num_triangles() * u1)), p, u);
        ss.pdf /= m.num_triangles();
        break;
      }
      default: return false;  // Cone::sample returns {} (geometry.cpp:461); AABB/OBB unsupported
    }
    if (ss.pdf <= 0 || std::isinf(ss.pdf)) return false;
    return true;
  }
  float pdf(const Ray& ray, vec3 ns) const {
    switch (kind) {
      case S_RECT: return as<Rect>().pdf(ray, ns);
      case S_SPHERE: return as<Sphere>().pdf(ray);
      case S_DISK: return as<Disk>().pdf(ray, ns);
      case S_CONE: return as<Cone>().pdf(ray, ns);
      case S_PLANE: return as<Plane>().pdf();
      case S_LINE: return as<Line>().pdf(ray, ns);
      case S_TRIANGLE: return as<Triangle>().pdf(ray, ns);
      case S_MESH: return as<Mesh>().pdf(ray, ns);
      default: return 0.0f;
    }
  }
};

struct Camera {  // camera.cpp:7-33
  vec3 position;
  mat3 c2w;
  vec2 fov2d;
  float len_radius = 0, focus_distance = 1;
  int W = 0, H = 0;
  void init(int w, int h, vec3 from, vec3 to, float fov, float lr, float fd) {
    W = w;
    H = h;
    position = from;
    c2w = to_mat3(look_at(from, to));
    float aspect = float(w) / h;  // film.h:32
    fov2d = vec2(fov * aspect, fov);
    len_radius = lr;
    focus_distance = fd;
  }
  Ray gen_ray(vec2 p_film, vec2 u2) const {
    p_film = (p_film - vec2(0.5f, 0.5f)) * 2.0f;  // camera.cpp:17-20
    vec2 pc = p_film * fov2d;
    if (len_radius == 0.0f) {
      return Ray(position, normalize(c2w * vec3(pc.x, pc.y, 1.0f)));
    } else {
      vec3 dir = normalize(vec3(pc.x, pc.y, 1.0f));
      vec3 p_focus = focus_distance * dir / dir.z;
      vec2 d = len_radius * sample_disk_polar(u2);
      vec3 p_len(d.x, d.y, 0.0f);
      return Ray(position + p_len, c2w * normalize(p_focus - p_len));
    }
  }
};

// ------------------------------------------------------------------------------------------------
// pine's BVH (src/pine/impl/accel/bvh.cpp:30-147 build, :321-451 traversal, :453-548 two-level)
// ------------------------------------------------------------------------------------------------
struct BVHImpl {
  struct Primitive {
    AABB aabb;
    int index = 0;
  };
  struct Node {
    AABB aabbs[2];
    int children[2] = {-1, -1};
    std::vector<int> prims;
  };
  std::vector<Node> nodes;
  int root = -1;

  void build(std::vector<Primitive> prims) {  // :30-41
    AABB aabb;
    for (auto& p : prims) aabb.extend(p.aabb);
    nodes.reserve(prims.size());
    build_rec(prims.data(), prims.data() + prims.size(), aabb);
    root = int(nodes.size()) - 1;
  }
  AABB get_aabb() const { return union_(nodes[root].aabbs[0], nodes[root].aabbs[1]); }

  int build_rec(Primitive* begin, Primitive* end, AABB aabb) {  // build_sah_binned :43-147
    Node node;
    int n = int(end - begin);
    auto make_leaf = [&]() {
      for (int i = 0; i < n; i++) node.prims.push_back(begin[i].index);
      for (Primitive* p = begin; p != end; p++) node.aabbs[0].extend(p->aabb);
      node.aabbs[1] = node.aabbs[0];
      nodes.push_back(node);
      return int(nodes.size()) - 1;
    };
    if (n == 1) return make_leaf();

    AABB cb;
    for (int i = 0; i < n; i++) cb.extend(begin[i].aabb.centroid());
    float surfaceArea = aabb.surface_area();
    const int nBuckets = 16;
    float minCost = kFloatMax;
    int bestAxis = -1, splitBucket = -1;
    for (int axis = 0; axis < 3; axis++) {
      if (cb.degenerated(axis)) continue;
      struct Bucket {
        int count = 0;
        AABB aabb;
      } buckets[nBuckets];
      for (int i = 0; i < n; i++) {
        int b = std::min(int(nBuckets * cb.relative_position(begin[i].aabb.centroid(axis), axis)),
                         nBuckets - 1);
        buckets[b].count++;
        buckets[b].aabb.extend(begin[i].aabb);
      }
      float cost[nBuckets - 1] = {};
      AABB bF;
      int cF = 0;
      for (int i = 0; i < nBuckets - 1; i++) {
        bF.extend(buckets[i].aabb);
        cF += buckets[i].count;
        cost[i] += cF * bF.surface_area();
      }
      AABB bB;
      int cB = 0;
      for (int i = nBuckets - 1; i >= 1; i--) {
        bB.extend(buckets[i].aabb);
        cB += buckets[i].count;
        cost[i - 1] += cB * bB.surface_area();
      }
      for (int i = 0; i < nBuckets - 1; i++) cost[i] = 1.0f + cost[i] / surfaceArea;
      float axisMin = kFloatMax;
      int axisSplit = -1;
      for (int i = 0; i < nBuckets - 1; i++)
        if (cost[i] < axisMin) {
          axisMin = cost[i];
          axisSplit = i;
        }
      if (axisMin < minCost) {
        minCost = axisMin;
        bestAxis = axis;
        splitBucket = axisSplit;
      }
    }
    float leafCost = float(n);
    if (minCost > leafCost) return make_leaf();

    // psl::partition (src/psl/algorithm.h:394-402): Lomuto, swap(tail++, i) when pred holds
    Primitive* tail = begin;
    for (Primitive* i = begin; i != end; ++i) {
      int b = int(nBuckets * cb.relative_position(i->aabb.centroid(bestAxis), bestAxis));
      if (b == nBuckets) b = nBuckets - 1;
      if (b <= splitBucket) std::swap(*tail++, *i);
    }
    Primitive* pmid = tail;
    for (Primitive* p = begin; p != pmid; p++) node.aabbs[0].extend(p->aabb);
    for (Primitive* p = pmid; p != end; p++) node.aabbs[1].extend(p->aabb);
    node.children[0] = build_rec(begin, pmid, node.aabbs[0]);
    node.children[1] = build_rec(pmid, end, node.aabbs[1]);
    nodes.push_back(node);
    return int(nodes.size()) - 1;
  }

  template <class F>
  bool any_hit(const Ray& ray, F&& f) const {  // BVHImpl::hit :321-383
    if (nodes.empty()) return false;
    RayOctant oct(ray);
    int stack[32], ptr = 0, next = root;
    if (!nodes[next].prims.empty()) {
      for (int idx : nodes[next].prims)
        if (f(ray, idx)) return true;
      return false;
    }
    while (true) {
      const Node& node = nodes[next];
      int l = -1, r = -1;
      float t0 = ray.tmax, t1 = ray.tmax;
      if (node.aabbs[0].hit(oct, ray.tmin, t0)) {
        const Node& c = nodes[node.children[0]];
        if (c.prims.empty()) l = node.children[0];
        else
          for (int idx : c.prims)
            if (f(ray, idx)) return true;
      }
      if (node.aabbs[1].hit(oct, ray.tmin, t1)) {
        const Node& c = nodes[node.children[1]];
        if (c.prims.empty()) r = node.children[1];
        else
          for (int idx : c.prims)
            if (f(ray, idx)) return true;
      }
      if (l != -1) {
        if (r != -1) {
          if (t0 > t1) { stack[ptr++] = l; next = r; }
          else { stack[ptr++] = r; next = l; }
        } else next = l;
      } else if (r != -1) next = r;
      else {
        if (ptr == 0) break;
        next = stack[--ptr];
      }
    }
    return false;
  }
  template <class F>
  bool closest(Ray& ray, F&& f) const {  // BVHImpl::Intersect :385-451
    if (nodes.empty()) return false;
    RayOctant oct(ray);
    bool hit = false;
    int stack[32], ptr = 0, next = root;
    if (!nodes[next].prims.empty()) {
      for (int idx : nodes[next].prims)
        if (f(ray, idx)) hit = true;
      return hit;
    }
    while (true) {
      const Node& node = nodes[next];
      int l = -1, r = -1;
      float t0 = ray.tmax, t1 = ray.tmax;
      if (node.aabbs[0].hit(oct, ray.tmin, t0)) {
        const Node& c = nodes[node.children[0]];
        if (c.prims.empty()) l = node.children[0];
        else
          for (int idx : c.prims)
            if (f(ray, idx)) hit = true;
      }
      if (node.aabbs[1].hit(oct, ray.tmin, t1)) {
        const Node& c = nodes[node.children[1]];
        if (c.prims.empty()) r = node.children[1];
        else
          for (int idx : c.prims)
            if (f(ray, idx)) hit = true;
      }
      if (l != -1) {
        if (r != -1) {
          if (t0 > t1) { stack[ptr++] = l; next = r; }
          else { stack[ptr++] = r; next = l; }
        } else next = l;
      } else if (r != -1) next = r;
      else {
        if (ptr == 0) break;
        next = stack[--ptr];
      }
    }
    return hit;
  }
};

static thread_local bool t_trace_queries = false;  // $PINE_ORACLE_TRACE_PIXEL=x,y: every accel query of that pixel's paths on stderr (debugging aid)
static int g_order_mode = 0;  // test-infrastructure switch (oracle_set_order): 0 pine's BVH order, 1 nearest bounds first, 2 EmbreeAccel's order

// ------------------------------------------------------------------------------------------------
// Order mode "embree": the order in which the reference's DEFAULT accel, EmbreeAccel, tests the non-mesh shapes.
// pine registers every non-mesh shape as one Embree user primitive with pine's own bounds / intersect callbacks
// (src/pine/impl/accel/embree.cpp:12-40, :88-99), so the only thing Embree decides is WHICH primitives a closest-hit query
// tests, in WHICH order, with which tfar.  That is restated here from the vendored Embree 4.3.1 (src/contrib/embree), the
// code path an AVX2 x86 host takes: a BVH8 of `Object` leaves (one primitive each: kernels/common/state.cpp:76-77,
// kernels/common/scene.cpp:453-467) built by the binned-SAH builder (kernels/builders/bvh_builder_sah.h:220-330,
// heuristic_binning.h, heuristic_binning_array_aligned.h) and walked by the single-ray traverser
// (kernels/bvh/bvh_intersector1.cpp:30-107, bvh_traverser1.h:310-385, node_intersector1.h:26-60, :484-530).
// ------------------------------------------------------------------------------------------------
#include "../pine_amd/data/rcpps_table.h"  // the RCPPS estimates of the CPU that rendered tests/golden/film_embree_* (tools/extract_rcpps_table.c)
namespace embree_order {
constexpr float kInf = std::numeric_limits<float>::infinity();
inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// common/math/vec3fa.h:122-144 (AVX2 branch): r = RCPPS(a); r + r * (1 - a * r), both steps fused
inline float rcp_nr(float a) {
  const uint32_t u = f2u(a);
  const int e = int((u >> 23) & 0xffu);                                            // (zero_fix keeps |a| >= 1e-18; the triangle test's |den| may be anything)
  const uint32_t t = kRcppsTable[(u >> 12) & 0x7ffu];                              // estimate for the mantissa in [1, 2): in (0.5, 1]
  const int re = int((t >> 23) & 0xffu) + 127 - e;
  const float r = e == 0 || re >= 255 ? std::copysign(kInf, a)                     // RCPPS: zero and denormal operands give infinity,
                  : re <= 0           ? std::copysign(0.0f, a)                     //        results below the normal range are flushed to zero
                                      : u2f((u & 0x80000000u) | (uint32_t(re) << 23) | (t & 0x7fffffu));
  const float h = std::fmaf(-a, r, 1.0f);
  return std::fmaf(r, h, r);
}
inline float rcp_safe(float a) {  // vec3fa.h:167-172: min_rcp_input = 1e-18f (common/math/constants.h)
  return rcp_nr(std::fabs(a) < 1e-18f ? 1e-18f : a);
}
struct Box {
  float lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
  void extend(const float* l, const float* h) {
    for (int d = 0; d < 3; d++) lo[d] = std::min(lo[d], l[d]), hi[d] = std::max(hi[d], h[d]);
  }
  void extend(const float* p) { extend(p, p); }
  void extend(const Box& b) { extend(b.lo, b.hi); }
};
// common/math/vec3fa.h:349, bbox.h:129-139: madd(d.x, d.y + d.z, d.y * d.z).  The BUILDER is the AVX one ("building BVH8<object> using
// avx::BVH8BuilderSAH" under verbose=2; builders are not compiled for AVX2): its madd is a * b + c with two roundings (emath.h:328)
inline float half_area(const Box& b) {
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  return dx * (dy + dz) + dy * dz;
}
struct PrimRef {
  float lo[3], hi[3];
  int id;  // geomID (primID is 0: rtcSetGeometryUserPrimitiveCount(geom, 1))
  void center2(float* c) const { for (int d = 0; d < 3; d++) c[d] = lo[d] + hi[d]; }
};
struct Set {  // PrimInfoRange: [begin, end) of the PrimRef array with the bounds of the boxes and of the doubled centres
  size_t begin = 0, end = 0;
  Box geom, cent;
  size_t size() const { return end - begin; }
  void add(const PrimRef& p) {
    geom.extend(p.lo, p.hi);
    float c[3];
    p.center2(c);
    cent.extend(c);
  }
};
struct Split {  // BinSplit + its BinMapping
  float sah = kInf;
  int dim = -1, pos = 0;
  size_t num = 0;
  float ofs[3] = {0, 0, 0}, scale[3] = {0, 0, 0};
  int bin(const PrimRef& p, int d) const {  // BinMapping::bin_unsafe: floori((center2 - ofs) * scale)
    float c[3];
    p.center2(c);
    return int(std::floor((c[d] - ofs[d]) * scale[d]));
  }
};
struct Tree {
  struct Node {
    float lo[3][8], hi[3][8];
    int child[8];  // >= 0: node; < 0: ~geometry index (an Object leaf); kEmpty: no child
    int n = 0;
  };
  static constexpr int kEmpty = INT32_MIN;
  std::vector<Node> nodes;
  int root = kEmpty;
  std::vector<PrimRef> prims;

  // HeuristicArrayBinningSAH::find (heuristic_binning_array_aligned.h:100-114) = BinMapping (heuristic_binning.h:43-52), BinInfoT::bin (:210-255), ::best (:331-385)
  Split find(const Set& set) const {
    Split sp;
    constexpr size_t BINS = 32;  // NUM_OBJECT_BINS
    sp.num = std::min(BINS, size_t(4.0f + 0.05f * float(set.size())));
    for (int d = 0; d < 3; d++) {
      const float eps = 1E-34f, size = set.cent.hi[d] - set.cent.lo[d];
      const float diag = eps > size ? eps : size;  // _mm_max_ps(eps, size)
      sp.scale[d] = diag > eps ? (0.99f * float(sp.num)) / diag : 0.0f;
      sp.ofs[d] = set.cent.lo[d];
    }
    Box bounds[BINS][3];
    unsigned counts[BINS][3] = {};
    for (size_t i = set.begin; i < set.end; i++)
      for (int d = 0; d < 3; d++) {
        const int b = std::clamp(sp.bin(prims[i], d), 0, int(sp.num) - 1);  // BinMapping::bin clamps
        bounds[b][d].extend(prims[i].lo, prims[i].hi);
        counts[b][d]++;
      }
    float rAreas[BINS][3];
    unsigned rCounts[BINS][3];
    {
      unsigned count[3] = {0, 0, 0};
      Box bx[3];
      for (size_t i = sp.num - 1; i > 0; i--)
        for (int d = 0; d < 3; d++) {
          count[d] += counts[i][d];
          rCounts[i][d] = count[d];
          bx[d].extend(bounds[i][d]);
          rAreas[i][d] = half_area(bx[d]);
        }
    }
    float best_sah[3] = {kInf, kInf, kInf};
    int best_pos[3] = {0, 0, 0};
    {
      unsigned count[3] = {0, 0, 0};
      Box bx[3];
      for (size_t i = 1; i < sp.num; i++)
        for (int d = 0; d < 3; d++) {
          count[d] += counts[i - 1][d];
          bx[d].extend(bounds[i - 1][d]);
          const float lArea = half_area(bx[d]);
          // counts in blocks of 8: BVH8VirtualSceneBuilderSAH passes sahBlockSize = 8 (bvh_builder_sah.cpp:509-513)
          const float sah = lArea * float((count[d] + 7u) >> 3) + rAreas[i][d] * float((rCounts[i][d] + 7u) >> 3);
          if (sah < best_sah[d]) best_pos[d] = int(i), best_sah[d] = sah;
        }
    }
    for (int d = 0; d < 3; d++) {
      if (sp.scale[d] == 0.0f) continue;  // mapping.invalid(dim)
      if (best_sah[d] < sp.sah && best_pos[d] != 0) sp.dim = d, sp.pos = best_pos[d], sp.sah = best_sah[d];
    }
    return sp;
  }
  // HeuristicArrayBinningSAH::split (heuristic_binning_array_aligned.h:134-171): the array order inside the halves never
  // reaches the tree (sets are re-binned; the fallback sorts first), so a stable partition stands for serial_partitioning
  void split(const Split& sp, const Set& set, Set& l, Set& r) {
    if (sp.dim < 0) {  // deterministic_order + performFallbackSplit (:49-64, :173-181): by ID, then the median
      std::sort(prims.begin() + long(set.begin), prims.begin() + long(set.end), [](const PrimRef& a, const PrimRef& b) { return a.id < b.id; });
      const size_t center = (set.begin + set.end) / 2;
      l.begin = set.begin, l.end = center, r.begin = center, r.end = set.end;
    } else {
      auto mid = std::stable_partition(prims.begin() + long(set.begin), prims.begin() + long(set.end), [&](const PrimRef& p) { return sp.bin(p, sp.dim) < sp.pos; });
      l.begin = set.begin, l.end = size_t(mid - prims.begin()), r.begin = l.end, r.end = set.end;
    }
    for (size_t i = l.begin; i < l.end; i++) l.add(prims[i]);
    for (size_t i = r.begin; i < r.end; i++) r.add(prims[i]);
  }
  // GeneralBVHBuilder::BuilderT::recurse (bvh_builder_sah.h:220-330) with branchingFactor 8, minLeafSize = maxLeafSize = 1
  int recurse(const Set& current, int depth) {
    if (current.size() <= 1 || depth + 8 >= 40) {
      if (current.size() != 1) throw std::runtime_error("embree order: large leaves are not restated");
      return ~prims[current.begin].id;
    }
    Set children[8];
    int n = 2;
    split(find(current), current, children[0], children[1]);
    while (n < 8) {
      float best_area = -kInf;
      int best = -1;
      for (int i = 0; i < n; i++) {
        if (children[i].size() <= 1) continue;
        if (half_area(children[i].geom) > best_area) best = i, best_area = half_area(children[i].geom);
      }
      if (best < 0) break;
      Set l, r;
      split(find(children[best]), children[best], l, r);
      children[best] = l;
      children[n++] = r;
    }
    std::stable_sort(children, children + n, [](const Set& a, const Set& b) { return a.size() > b.size(); });  // std::sort of <= 8 records: an insertion sort
    const int me = int(nodes.size());
    nodes.emplace_back();
    {
      Node& nd = nodes[size_t(me)];
      nd.n = n;
      for (int i = 0; i < 8; i++) {
        nd.child[i] = kEmpty;
        for (int d = 0; d < 3; d++) nd.lo[d][i] = kInf, nd.hi[d][i] = -kInf;  // AABBNode::clear
      }
      for (int i = 0; i < n; i++)
        for (int d = 0; d < 3; d++) nd.lo[d][i] = children[i].geom.lo[d], nd.hi[d][i] = children[i].geom.hi[d];
    }
    for (int i = 0; i < n; i++) {
      const int c = recurse(children[i], depth + 1);
      nodes[size_t(me)].child[i] = c;
    }
    return me;
  }
  // createPrimRefArray (kernels/common/scene_user_geometry.h:35-47, accelset.h:105-110): boxes that are not finite
  // (|x| < FLT_LARGE = 1.844e18) or empty are left out of the hierarchy altogether
  void build(const std::vector<std::pair<AABB, int>>& boxes) {
    nodes.clear();
    prims.clear();
    root = kEmpty;
    Set all;
    for (auto& [b, id] : boxes) {
      PrimRef p{{b.lower.x, b.lower.y, b.lower.z}, {b.upper.x, b.upper.y, b.upper.z}, id};
      bool ok = true;
      for (int d = 0; d < 3; d++) ok = ok && p.lo[d] > -1.844E18f && p.hi[d] < 1.844E18f && p.lo[d] <= p.hi[d];
      if (!ok) continue;
      prims.push_back(p);
      all.add(p);
    }
    all.begin = 0, all.end = prims.size();
    if (prims.empty()) return;
    root = recurse(all, 1);
  }
};
// Meshes are Embree TRIANGLE geometry (embree.cpp:76-87): a BVH8 of Triangle4 blocks (kernels/common/scene.cpp:205-214, build
// quality HIGH) tested by TriangleMIntersector1Moeller<4, true> -- MoellerTrumboreIntersector1<4>::intersectEdge + finalize
// (kernels/geometry/triangle_intersector_moeller.h:66-140, :29-37; Triangle4 keeps v0, e1 = v0 - v1, e2 = v2 - v0,
// geometry/triangle.h) -- as the AVX2 build computes it: fused cross / dot products (common/math/vec3.h), the same RCPPS Newton
// step for 1 / |den|.  The four lanes of a block are independent; this is one lane.  Which triangles Embree's own hierarchy
// (spatial splits: not restated) hands to the test cannot change the closest hit: only an exact tie in t is decided by it.
struct TriHit {
  float t, u, v;
  float ng[3];
};
inline bool tri_test(const Ray& ray, vec3 a, vec3 b, vec3 c, float tnear, float tfar, TriHit& h) {
  auto cross_f = [](const float* x, const float* y, float* r) {  // (msub(a.y, b.z, a.z * b.y), msub(a.z, b.x, a.x * b.z), msub(a.x, b.y, a.y * b.x))
    r[0] = std::fmaf(x[1], y[2], -(x[2] * y[1]));
    r[1] = std::fmaf(x[2], y[0], -(x[0] * y[2]));
    r[2] = std::fmaf(x[0], y[1], -(x[1] * y[0]));
  };
  auto dot_f = [](const float* x, const float* y) { return std::fmaf(x[0], y[0], std::fmaf(x[1], y[1], x[2] * y[2])); };
  const float v0[3] = {a.x, a.y, a.z}, e1[3] = {a.x - b.x, a.y - b.y, a.z - b.z}, e2[3] = {c.x - a.x, c.y - a.y, c.z - a.z};
  const float O[3] = {ray.o.x, ray.o.y, ray.o.z}, D[3] = {ray.d.x, ray.d.y, ray.d.z};
  float ng[3], R[3];
  cross_f(e2, e1, ng);
  const float C[3] = {v0[0] - O[0], v0[1] - O[1], v0[2] - O[2]};
  cross_f(C, D, R);
  const float den = dot_f(ng, D), abs_den = std::fabs(den);
  const uint32_t sgn = f2u(den) & 0x80000000u;
  const float U = u2f(f2u(dot_f(R, e2)) ^ sgn), V = u2f(f2u(dot_f(R, e1)) ^ sgn);
  if (!(den != 0.0f && U >= 0.0f && V >= 0.0f && U + V <= abs_den)) return false;
  const float T = u2f(f2u(dot_f(ng, C)) ^ sgn);
  if (!(abs_den * tnear < T && T <= abs_den * tfar)) return false;
  const float r = rcp_nr(abs_den);
  h.t = T * r, h.u = U * r, h.v = V * r;
  h.ng[0] = ng[0], h.ng[1] = ng[1], h.ng[2] = ng[2];
  return true;
}

// BVHNIntersector1<8, BVH_AN1, false, ...>::intersect (kernels/bvh/bvh_intersector1.cpp:30-107): `leaf(geometry index)` is
// the user callback; it reads and may shorten ray.tmax.
template <class Leaf>
inline void traverse(const Tree& tree, Ray& ray, Leaf&& leaf) {
  if (tree.root == Tree::kEmpty) return;
  // TravRay<8, false> (node_intersector1.h:26-60): rdir = rcp_safe(dir), org_rdir = org * rdir, near / far planes by the sign of rdir
  const float org[3] = {ray.o.x, ray.o.y, ray.o.z}, dir[3] = {ray.d.x, ray.d.y, ray.d.z};
  float rdir[3], org_rdir[3];
  bool near_hi[3];
  for (int d = 0; d < 3; d++) {
    rdir[d] = rcp_safe(dir[d]);
    org_rdir[d] = org[d] * rdir[d];
    near_hi[d] = !(rdir[d] >= 0.0f);
  }
  const float tnear = std::max(ray.tmin, 0.0f);
  float tfar = std::max(ray.tmax, 0.0f);
  struct Item {
    int ref;
    uint32_t dist;
  };
  Item stack[1 + 7 * 40];
  int sp = 1;
  stack[0] = Item{tree.root, f2u(-kInf)};
  auto as_int = [](float f) { return int32_t(f2u(f)); };
  while (sp > 0) {
    sp--;
    int cur = stack[sp].ref;
    if (u2f(stack[sp].dist) > ray.tmax) continue;  // (ray.tfar: the RayHit's own, updated by the callback)
    bool popped = false;
    while (cur >= 0) {
      const Tree::Node& nd = tree.nodes[size_t(cur)];
      // intersectNode<8> (node_intersector1.h:484-530, AVX2 without AVX-512): fused a * rdir - org_rdir, integer max / min
      uint32_t dist[8];
      unsigned mask = 0;
      for (int i = 0; i < 8; i++) {
        int32_t tn = as_int(tnear), tf = as_int(tfar);
        for (int d = 0; d < 3; d++) {
          const float lo = nd.lo[d][i], hi = nd.hi[d][i];
          tn = std::max(tn, as_int(std::fmaf(near_hi[d] ? hi : lo, rdir[d], -org_rdir[d])));
          tf = std::min(tf, as_int(std::fmaf(near_hi[d] ? lo : hi, rdir[d], -org_rdir[d])));
        }
        dist[i] = uint32_t(tn);
        if (!(tn > tf)) mask |= 1u << i;
      }
      if (mask == 0) {
        popped = true;
        break;
      }
      // BVHNNodeTraverser1Hit<8>::traverseClosestHit (bvh_traverser1.h:310-385), children in ascending slot order
      Item hits[8];
      int nh = 0;
      for (int i = 0; i < 8; i++)
        if (mask & (1u << i)) hits[nh++] = Item{nd.child[i], dist[i]};
      auto cmp_xchg = [](Item& a, Item& b) {  // stack_item.h:54-66: a <= b afterwards (signed compare of the distance words)
        if (int32_t(b.dist) < int32_t(a.dist)) std::swap(a, b);
      };
      if (nh == 1) {
        cur = hits[0].ref;
      } else if (nh == 2) {
        if (hits[0].dist < hits[1].dist) stack[sp++] = hits[1], cur = hits[0].ref;
        else stack[sp++] = hits[0], cur = hits[1].ref;
      } else if (nh == 3) {
        Item &s0 = hits[0], &s1 = hits[1], &s2 = hits[2];
        cmp_xchg(s1, s0), cmp_xchg(s2, s1), cmp_xchg(s1, s0);  // sort3
        stack[sp++] = s0, stack[sp++] = s1, cur = s2.ref;
      } else if (nh == 4) {
        Item &s0 = hits[0], &s1 = hits[1], &s2 = hits[2], &s3 = hits[3];
        cmp_xchg(s1, s0), cmp_xchg(s3, s2), cmp_xchg(s2, s0), cmp_xchg(s3, s1), cmp_xchg(s2, s1);  // sort4
        stack[sp++] = s0, stack[sp++] = s1, stack[sp++] = s2, cur = s3.ref;
      } else {
        Item* first = stack + sp;
        for (int i = 0; i < nh; i++) stack[sp++] = hits[i];
        for (Item* i = first + 1; i != stack + sp; ++i) {  // sort(begin, end), stack_item.h:88-104: descending, stable
          const Item item = *i;
          Item* j = i;
          while (j != first && (j - 1)->dist < item.dist) *j = *(j - 1), --j;
          *j = item;
        }
        cur = stack[--sp].ref;
      }
    }
    if (popped || cur == Tree::kEmpty) continue;
    leaf(~cur);       // an Object leaf: the user callback, which may shorten ray.tmax (embree.cpp:24-40)
    tfar = ray.tmax;  // tray.tfar = ray.tfar
  }
}
// BVHNIntersector1<8, ...>::occluded (kernels/bvh/bvh_intersector1.cpp:117-195): every primitive whose box (and whose ancestors')
// the ray enters within [tnear, tfar] is handed to `leaf` until one reports a hit.  The ORDER cannot change an any-hit answer;
// WHICH primitives are asked can: a shape whose hit() succeeds where the ray misses its own bounds (Plane beyond its +-100 box,
// geometry.cpp:52) is found by pine's BVH when it shares a leaf box with a neighbour, and never by Embree.
template <class Leaf>
inline bool occluded(const Tree& tree, const Ray& ray, Leaf&& leaf) {
  if (tree.root == Tree::kEmpty) return false;
  if (ray.tmax < 0.0f) return false;
  const float org[3] = {ray.o.x, ray.o.y, ray.o.z}, dir[3] = {ray.d.x, ray.d.y, ray.d.z};
  float rdir[3], org_rdir[3];
  bool near_hi[3];
  for (int d = 0; d < 3; d++) {
    rdir[d] = rcp_safe(dir[d]);
    org_rdir[d] = org[d] * rdir[d];
    near_hi[d] = !(rdir[d] >= 0.0f);
  }
  auto as_int = [](float f) { return int32_t(f2u(f)); };
  const int32_t tnear = as_int(std::max(ray.tmin, 0.0f)), tfar = as_int(std::max(ray.tmax, 0.0f));
  std::vector<int> stack{tree.root};
  while (!stack.empty()) {
    const int cur = stack.back();
    stack.pop_back();
    if (cur < 0) {
      if (leaf(~cur)) return true;
      continue;
    }
    const Tree::Node& nd = tree.nodes[size_t(cur)];
    for (int i = nd.n - 1; i >= 0; i--) {
      int32_t tn = tnear, tf = tfar;
      for (int d = 0; d < 3; d++) {
        tn = std::max(tn, as_int(std::fmaf(near_hi[d] ? nd.hi[d][i] : nd.lo[d][i], rdir[d], -org_rdir[d])));
        tf = std::min(tf, as_int(std::fmaf(near_hi[d] ? nd.lo[d][i] : nd.hi[d][i], rdir[d], -org_rdir[d])));
      }
      if (!(tn > tf)) stack.push_back(nd.child[i]);
    }
  }
  return false;
}
}  // namespace embree_order

struct Scene {
  NodeTable node_table;
  std::vector<Material> materials;
  std::vector<std::string> material_names;
  std::vector<Geometry> geometries;
  // Scene::lights in add order (scene.cpp:16-33): an AreaLight per emissive geometry, explicit Point /
  // Spot / Directional lights; UniformLightSampler::build appends the environment light (lightsampler.cpp:6-10)
  struct Light {
    enum Kind { Area, Point, Spot, Directional, Sky } kind = Area;
    int geom = -1;
    vec3 position, direction, color;
    float falloff_cos = 0, cutoff_cos = 0;
    bool is_delta() const { return kind == Point || kind == Spot || kind == Directional; }  // light.h:111-113
  };
  std::vector<Light> lights;
  bool has_env = false;  // the LAST entry of `lights` is the environment light
  Camera camera;
  // accel (BVH::build bvh.cpp:453-495)
  std::vector<std::shared_ptr<BVHImpl>> lbvh;
  BVHImpl tbvh;
  std::vector<int> indices;
  std::vector<AABB> top_aabbs;  // the top-level primitives' boxes, in `indices` order (order mode "nearest")
  embree_order::Tree etree;     // order mode "embree": Embree's BVH8 over the non-mesh shapes

  int find_material(const std::string& n) const {
    for (int i = int(material_names.size()) - 1; i >= 0; i--)  // map semantics: last add wins
      if (material_names[i] == n) return i;
    return -1;
  }
  void build_accel() {
    lbvh.clear();
    tbvh = BVHImpl();
    indices.clear();
    if (geometries.empty()) return;
    for (size_t i = 0; i < geometries.size(); i++) {
      if (geometries[i].kind != S_MESH) continue;
      auto& mesh = *static_cast<Mesh*>(geometries[i].impl.get());
      if (mesh.num_triangles() == 0) continue;
      std::vector<BVHImpl::Primitive> prims;
      for (size_t t = 0; t < mesh.num_triangles(); t++) {
        BVHImpl::Primitive p;
        p.aabb = mesh.get_aabb(t);
        p.index = int(prims.size());
        prims.push_back(p);
      }
      auto b = std::make_shared<BVHImpl>();
      b->build(std::move(prims));
      mesh.bvh = b;
      lbvh.push_back(b);
      indices.push_back(int(i));
    }
    std::vector<BVHImpl::Primitive> prims;
    for (auto& s : lbvh) {
      BVHImpl::Primitive p;
      p.aabb = s->get_aabb();
      p.index = int(prims.size());
      prims.push_back(p);
    }
    for (size_t i = 0; i < geometries.size(); i++) {
      if (geometries[i].kind == S_MESH) continue;
      BVHImpl::Primitive p;
      p.aabb = geometries[i].get_aabb();
      p.index = int(prims.size());
      prims.push_back(p);
      indices.push_back(int(i));
    }
    top_aabbs.clear();
    for (auto& p : prims) top_aabbs.push_back(p.aabb);
    tbvh.build(prims);
    {
      std::vector<std::pair<AABB, int>> boxes;  // user primitives in geomID order (embree.cpp:113-117)
      for (size_t i = 0; i < geometries.size(); i++)
        if (geometries[i].kind != S_MESH) boxes.emplace_back(geometries[i].get_aabb(), int(i));
      etree.build(boxes);
    }
  }
  bool intersect_nearest(Ray& ray, SurfaceInteraction& it) const;
  bool intersect_embree(Ray& ray, SurfaceInteraction& it) const;
  bool hit(Ray ray) const {  // BVH::hit :497-511
    if (t_trace_queries) fprintf(stderr, "Q any %a %a %a %a %a %a %a %a\n", ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, ray.tmin, ray.tmax);
    if (geometries.empty()) return false;
    if (g_order_mode == 2) {  // EmbreeAccel::hit (embree.cpp:143-165): the meshes (Embree triangle geometry; pine's triangle tests stand in), then the user primitives
      // `return ray_.tfar < 0` (embree.cpp:164) is also what a query that STARTS with a negative tfar answers -- rtcOccluded1 leaves such
      // a ray alone (bvh_intersector1.cpp:128-129): "occluded", where pine's BVH finds nothing.  Light samples behind their own
      // distance (a negative ls.distance) reach this.
      if (ray.tmax < 0.0f) return true;
      for (size_t li = 0; li < lbvh.size(); li++) {
        const Mesh& m = geometries[indices[li]].as<Mesh>();
        if (lbvh[li]->any_hit(ray, [&](const Ray& rr, int idx) {
              vec3 a, b, c;
              m.face(size_t(idx), a, b, c);
              embree_order::TriHit h;
              return embree_order::tri_test(rr, a, b, c, std::max(rr.tmin, 0.0f), rr.tmax, h);
            }))
          return true;
      }
      return embree_order::occluded(etree, ray, [&](int gi) { return geometries[size_t(gi)].hit(Ray(ray.o, ray.d, ray.tmin, ray.tmax)); });
    }
    return tbvh.any_hit(ray, [&](const Ray& r, int li) {
      const Geometry& g = geometries[indices[li]];
      if (li < int(lbvh.size())) {
        const Mesh& m = g.as<Mesh>();
        return lbvh[li]->any_hit(r, [&](const Ray& rr, int idx) { return m.hit(rr, idx); });
      }
      return g.hit(r);
    });
  }
  bool intersect(Ray& ray, SurfaceInteraction& it) const {  // BVH::intersect :513-548
    if (t_trace_queries) fprintf(stderr, "Q closest %a %a %a %a %a %a %a %a\n", ray.o.x, ray.o.y, ray.o.z, ray.d.x, ray.d.y, ray.d.z, ray.tmin, ray.tmax);
    if (geometries.empty()) return false;
    uint32_t geom_index = 0, prim_index = 0;
    if (g_order_mode == 1) return intersect_nearest(ray, it);
    if (g_order_mode == 2) return intersect_embree(ray, it);
    bool hit = tbvh.closest(ray, [&](Ray& r, int li) {
      const Geometry& g = geometries[indices[li]];
      if (li < int(lbvh.size())) {
        const Mesh& m = g.as<Mesh>();
        bool h = lbvh[li]->closest(r, [&](Ray& rr, int idx) {
          bool hh = m.intersect(rr, idx);
          if (hh) prim_index = idx;
          return hh;
        });
        if (h) geom_index = indices[li];
        return h;
      }
      bool h = g.intersect(r);
      if (h) geom_index = indices[li];
      return h;
    });
    if (hit) {
      const Geometry& g = geometries[geom_index];
      it.geom = int(geom_index);
      if (g.kind == S_MESH)
        g.as<Mesh>().compute_surface_info(ray(), it, prim_index);
      else
        g.compute_surface_info(ray(), it);
    }
    return hit;
  }
};

// Order mode "nearest" (SURVEY.md Appendix A3's second traversal order; PINE_GPU_FLAG_ORDER_NEAREST on the device): the
// top-level primitives are tested in the order of their bounding boxes' ENTRY distances (ties: stored order), a primitive whose
// box is entered beyond the closest hit so far is skipped.  That is what a nearest-first traversal of ANY bounding-volume
// hierarchy with one primitive per leaf converges to -- Embree's BVH4 over the user primitives (embree.cpp:101-143: one user
// primitive per non-mesh shape, object leaves of size 1, children visited in tNear order) is one such -- so the
// order-dependent scaled Box(AABB, mat4) (bbox.cpp:149-171) behaves as under EmbreeAccel: it is tested before a farther wall
// has shortened ray.tmax.  Not the reference's BVH order, hence not bit-exact against O-gcc-bvh by construction; meshes keep
// their own BVH's order (triangles are not order dependent).  Any-hit queries are order independent and unchanged.
bool Scene::intersect_nearest(Ray& ray, SurfaceInteraction& it) const {
  struct Cand {
    float tnear;
    int li;
  };
  Cand cand[64];
  std::vector<Cand> big;
  const int n = int(top_aabbs.size());
  Cand* c = cand;
  if (n > 64) {
    big.resize(size_t(n));
    c = big.data();
  }
  RayOctant oct(ray);
  int m = 0;
  for (int li = 0; li < n; li++) {
    float tn;
    if (top_aabbs[size_t(li)].entry(oct, ray.tmin, ray.tmax, tn)) c[m++] = Cand{tn, li};
  }
  std::stable_sort(c, c + m, [](const Cand& a, const Cand& b) { return a.tnear < b.tnear; });
  uint32_t geom_index = 0, prim_index = 0;
  bool hit = false;
  for (int k = 0; k < m; k++) {
    if (c[k].tnear > ray.tmax) break;  // (sorted: every later box is entered beyond the hit too)
    const int li = c[k].li;
    const Geometry& g = geometries[indices[li]];
    bool h;
    if (li < int(lbvh.size())) {
      const Mesh& mm = g.as<Mesh>();
      h = lbvh[li]->closest(ray, [&](Ray& rr, int idx) {
        bool hh = mm.intersect(rr, idx);
        if (hh) prim_index = idx;
        return hh;
      });
    } else {
      h = g.intersect(ray);
    }
    if (h) {
      geom_index = indices[li];
      hit = true;
    }
  }
  if (hit) {
    const Geometry& g = geometries[geom_index];
    it.geom = int(geom_index);
    if (g.kind == S_MESH) g.as<Mesh>().compute_surface_info(ray(), it, prim_index);
    else g.compute_surface_info(ray(), it);
  }
  return hit;
}

// Order mode "embree": BVHNIntersector1<8, BVH_AN1, false, ...>::intersect (kernels/bvh/bvh_intersector1.cpp:30-107) over the
// tree above.  Meshes are Embree triangle geometry: they are asked first (the triangle accel precedes the user-geometry accel,
// kernels/common/scene.cpp:741-755) through Embree's own triangle test (tri_test above).
bool Scene::intersect_embree(Ray& ray, SurfaceInteraction& it) const {
  using namespace embree_order;
  uint32_t geom_index = 0, prim_index = 0;
  bool hit = false;
  TriHit th{};
  const float tnear = std::max(ray.tmin, 0.0f);
  for (size_t li = 0; li < lbvh.size(); li++) {
    const Mesh& mm = geometries[indices[li]].as<Mesh>();
    if (lbvh[li]->closest(ray, [&](Ray& rr, int idx) {  // (pine's per-mesh BVH only decides which triangles are looked at)
          vec3 a, b, c;
          mm.face(size_t(idx), a, b, c);
          TriHit h;
          if (!tri_test(rr, a, b, c, tnear, rr.tmax, h)) return false;
          rr.tmax = h.t;
          th = h;
          prim_index = uint32_t(idx);
          return true;
        }))
      geom_index = indices[li], hit = true;
  }
  embree_order::traverse(etree, ray, [&](int gi) {
    Ray r(ray.o, ray.d, ray.tmin, ray.tmax);  // (the callback builds its own Ray from Embree's, embree.cpp:31-33)
    if (geometries[size_t(gi)].intersect(r)) {
      ray.tmax = r.tmax;
      geom_index = uint32_t(gi);
      hit = true;
    }
  });
  if (hit) {
    const Geometry& g = geometries[geom_index];
    it.geom = int(geom_index);
    if (g.kind == S_MESH) {  // embree.cpp:233-247: position, normal and texcoord from Embree's barycentrics and geometric normal
      const Mesh& m = g.as<Mesh>();
      vec3 v0, v1, v2;
      m.face(prim_index, v0, v1, v2);
      it.p = lerp3(th.u, th.v, v0, v1, v2);
      const uint32_t i0 = m.indices[3 * prim_index], i1 = m.indices[3 * prim_index + 1], i2 = m.indices[3 * prim_index + 2];
      if (!m.normals.empty()) it.n = normalize(lerp3(th.u, th.v, m.normals[i0], m.normals[i1], m.normals[i2]));
      else it.n = normalize(vec3(th.ng[0], th.ng[1], th.ng[2]));
      if (!m.texcoords.empty()) {
        const vec2 a = m.texcoords[i0], b = m.texcoords[i1], c = m.texcoords[i2];
        it.uv = vec2((1.0f - th.u - th.v) * a.x + th.u * b.x + th.v * c.x, (1.0f - th.u - th.v) * a.y + th.u * b.y + th.v * c.y);
      } else {
        it.uv = vec2(th.u, th.v);
      }
    } else {
      g.compute_surface_info(ray(), it);
    }
  }
  return hit;
}

// Mesh::intersect(ray, it) via ShapeBVH (bvh.cpp:568-582) -- used by the BSSRDF walk only
bool mesh_intersect_full(const Mesh& m, Ray& ray, SurfaceInteraction& it) {
  int prim = 0;
  bool hit = m.bvh->closest(ray, [&](Ray& r, int idx) {
    bool h = m.intersect(r, idx);
    if (h) prim = idx;
    return h;
  });
  if (hit) m.compute_surface_info(ray(), it, prim);
  return hit;
}

// ------------------------------------------------------------------------------------------------
// PathIntegrator (src/pine/impl/integrator/path.cpp:26-124, src/pine/core/integrator.cpp:26-81)
// ------------------------------------------------------------------------------------------------
struct Counters {
  uint64_t vertices = 0, shadow = 0, bsdf = 0;
};
struct Vertex {  // path.cpp:15-25
  int length, diffuse_length;
  float pdf;
  bool is_delta;
};
struct RadianceResult {
  vec3 Lo;
  bool has_light_pdf = false;
  float light_pdf = 0;
};

struct LightSample {
  vec3 le, wo;
  float distance = 0, pdf = 0;
  bool is_delta = false;
};

struct Integrator {
  const Scene* scene;
  int max_path_length;

  vec3 material_le(const Material& m, vec3 n, vec3 wo) const {  // material.h:22-25
    if (m.kind != M_EMISSIVE) return vec3(0.0f);
    if (dot(wo, n) < 0.0f) return vec3(0.0f);
    return m.color;
  }
  // UniformLightSampler::sample (lightsampler.cpp:12-26) + AreaLight::sample (light.cpp:55-69)
  bool sample_light(vec3 p, float u1, vec2 u2, LightSample& ls) const {
    int N = int(scene->lights.size());
    if (N == 0) return false;
    u1 *= N;
    int index = int(u1);
    const Scene::Light& L = scene->lights[index];
    if (L.kind == Scene::Light::Area) {
      const Geometry& g = scene->geometries[L.geom];
      ShapeSample gs;
      if (!g.sample(p, u2, u1 - index, gs)) return false;
      ls.wo = gs.w;
      ls.pdf = gs.pdf;
      ls.distance = gs.distance;
      ls.le = material_le(scene->materials[g.material], gs.n, -ls.wo);
      if (ls.le.is_zero()) return false;
    } else if (!sample_other_light(L, p, u2, ls)) {
      return false;
    }
    ls.pdf = ls.pdf / N;
    ls.is_delta = L.is_delta();
    return true;
  }
  // Light::sample of the lights that are no AreaLight (light.cpp:11-54, 74-81)
  static bool sample_other_light(const Scene::Light& L, vec3 p, vec2 u2, LightSample& ls) {
    switch (L.kind) {
      case Scene::Light::Area: return false;
      case Scene::Light::Point:  // light.cpp:11-17
        ls.wo = normalize(L.position - p, ls.distance);
        ls.pdf = ls.distance * ls.distance;
        ls.le = L.color;
        break;
      case Scene::Light::Spot: {  // light.cpp:35-47
        ls.wo = normalize(L.position - p, ls.distance);
        const float cs = -dot(ls.wo, L.direction);
        if (cs > L.falloff_cos) ls.le = L.color;
        else if (cs > L.cutoff_cos) ls.le = L.color * (cs - L.cutoff_cos) / (L.falloff_cos - L.cutoff_cos);
        else return false;
        ls.pdf = ls.distance * ls.distance;
        break;
      }
      case Scene::Light::Directional:  // light.cpp:48-54
        ls.distance = 1e+10f;
        ls.wo = L.direction;
        ls.pdf = 1.0f;
        ls.le = L.color;
        break;
      case Scene::Light::Sky:  // light.cpp:71-84
        ls.wo = uniform_sphere(u2);
        ls.pdf = 1 / (4 * Pi);
        ls.distance = kFloatMax;
        ls.le = sky_color_of(L.color, ls.wo);
        break;
    }
    return true;
  }
  static vec3 sky_color_of(vec3 sun_color, vec3 wo) {  // Sky::color light.cpp:71-73, sky_color color.cpp:100-103
    const float t = wo.y / 2 + 0.7f;
    const vec3 a(1.0f, 0.8f, 0.6f), b(0.6f, 0.8f, 1.0f);
    const vec3 l = a * (1 - t) + b * t;  // psl::lerp(t, a, b) math.h
    return sun_color * (l * l);
  }

  // BSSRDF::sample_p (bxdf.cpp:329-353) + BXDF::sample_p (:375-382)
  void bssrdf_walk(BXDF& bxdf, vec3& beta, SurfaceInteraction& it, vec3 bc_p, vec3 bc_n, vec3 bc_wi,
                   Sampler& sampler) const {
    vec3 p = bc_p;
    vec3 w = -bc_wi;
    if (!Refract(bc_wi, bc_n, bxdf.ior, w)) return;
    int channel = int(sampler.randf() * 3);
    vec3 b(0.0f);
    b[channel] = 3;
    float sigma_t_inv = 1 / bxdf.sigma_s[channel];
    const Geometry& g = scene->geometries[it.geom];
    for (int i = 0;; i++) {
      Ray ray = i == 0 ? spawn_ray_pn(p, bc_n, w) : Ray(p, w);
      SurfaceInteraction sit;  // p, n zero-initialised (Appendix A5)
      bool h;
      if (g.kind == S_MESH) h = mesh_intersect_full(g.as<Mesh>(), ray, sit);
      else h = g.intersect(ray);  // non-mesh shapes do not fill it.p/it.n
      if (!h) return;
      float t = -std::log(1 - sampler.get1d()) * sigma_t_inv;
      if (ray.tmax < t) {
        beta = b;
        it.p = sit.p;
        it.n = sit.n;
        it.compute_transformation();
        bxdf.wi = it.to_local(-w);
        return;
      } else {
        p = ray(t);
        w = uniform_sphere(sampler.get2d());
      }
    }
  }

  RadianceResult radiance(Ray ray, Sampler& sampler, Vertex pv, Counters& cnt) const {
    RadianceResult result;
    cnt.vertices++;
    vec3 wi = -ray.d;
    vec3& Lo = result.Lo;

    SurfaceInteraction it;
    bool hit = scene->intersect(ray, it);
    if (hit) it.compute_transformation();  // integrator.cpp:36-41
    // medium block (path.cpp:50-72) is dead: no mediums.  Tr == vec3(1) (integrator.cpp:75-81)
    if (!hit) {  // path.cpp:75-81
      if (scene->has_env) {
        const Scene::Light& env = scene->lights.back();
        Lo += vec3(1.0f) * sky_color_of(env.color, ray.d);
        if (!pv.is_delta) {
          result.has_light_pdf = true;
          result.light_pdf = 1 / (4 * Pi);  // Sky::pdf, NOT divided by the light count
        }
      }
      return result;
    }

    const Geometry& g = scene->geometries[it.geom];
    const Material& mat = scene->materials[g.material];
    if (mat.kind == M_EMISSIVE) {  // path.cpp:83-87
      Lo += vec3(1.0f) * material_le(mat, it.n, wi);
      if (!pv.is_delta) {
        result.has_light_pdf = true;
        result.light_pdf = g.pdf(ray, it.n) / float(scene->lights.size());  // lightsampler.cpp:27-29
      }
      return result;
    }
    if (pv.length + 1 >= max_path_length) return result;  // path.cpp:89

    // BxdfSampleCtx (bxdf.h:10-21): copies p,n,uv now
    bool diffused = pv.diffuse_length > 0;
    vec3 bc_p = it.p, bc_n = it.n;
    const NodeEvalCtx nc{it.p, it.n, it.uv};  // BxdfSampleCtx -> NodeEvalCtx(it) (bxdf.h:10-21, node.h:13-20)
    BXDF bxdf = material_sample_bxdf(mat, nc, wi, bc_n, diffused, sampler);
    bxdf.wi = it.to_local(wi);  // material.h:119

    vec3 beta(1.0f);
    if (bxdf.kind == BX_BSSRDF) bssrdf_walk(bxdf, beta, it, bc_p, bc_n, wi, sampler);

    vec3 lo(0.0f);
    if (!bxdf.is_delta()) {  // path.cpp:98-113
      // g++ evaluates LightSampler::sample's arguments right-to-left (lightsampler.h:27):
      vec2 u2 = sampler.get2d();
      float u1 = sampler.get1d();
      LightSample ls;
      if (sample_light(it.p, u1, u2, ls)) {
        cnt.shadow++;
        if (!scene->hit(it.spawn_ray(ls.wo, ls.distance))) {
          float cosine = absdot(ls.wo, it.n);
          vec3 tr(1.0f);
          vec3 wo = it.to_local(ls.wo);
          vec3 f = bxdf.f(wo);
          if (ls.is_delta) {  // path.cpp:104-106
            lo += ls.le * tr * cosine * f / ls.pdf;
          } else {
            float mis = balance_heuristic(ls.pdf, bxdf.pdf(wo));
            lo += ls.le * tr * cosine * f / ls.pdf * mis;
          }
        }
      }
    }
    BSDFSample bs;
    if (bxdf.sample(sampler, bs)) {  // path.cpp:114-120
      cnt.bsdf++;
      bs.wo = it.to_world(bs.wo);
      float cosine = absdot(bs.wo, it.n);
      Vertex nv{pv.length + 1, pv.diffuse_length + (bs.is_delta ? 0 : 1), bs.pdf, bs.is_delta};
      RadianceResult child = radiance(it.spawn_ray(bs.wo), sampler, nv, cnt);
      float mis = child.has_light_pdf ? balance_heuristic(bs.pdf, child.light_pdf) : 1.0f;
      lo += child.Lo * bs.f * (cosine / bs.pdf * mis);
    }
    Lo += vmin(vec3(1.0f) * beta * lo, vec3(8.0f));  // path.cpp:121 per-level clamp
    return result;
  }
};

// ------------------------------------------------------------------------------------------------
// pscene parser (format: pine_amd/scene_io.py)
// ------------------------------------------------------------------------------------------------
std::string g_error;
float rdf(std::istream& in) {
  std::string tok;
  in >> tok;
  return strtof(tok.c_str(), nullptr);
}
vec3 rd3(std::istream& in) {
  float x = rdf(in), y = rdf(in), z = rdf(in);
  return vec3(x, y, z);
}
bool parse_pscene(const char* text, Scene& scene) {
  std::istringstream f(text);
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    std::string kw;
    in >> kw;
    if (kw == "node") {  // node <id> <kind> args (ids are consecutive from 0)
      int id = -1;
      std::string kind;
      in >> id >> kind;
      if (id != int(scene.node_table.nodes.size())) {
        g_error = "node ids must be consecutive";
        return false;
      }
      ShadingNode k;
      auto opc = [&]() {
        std::string o;
        in >> o;
        return o.empty() ? '?' : o[0];
      };
      if (kind == "constf") { k.kind = ShadingNode::ConstF; k.f = rdf(in); }
      else if (kind == "const3") { k.kind = ShadingNode::Const3; k.v = rd3(in); }
      else if (kind == "position") k.kind = ShadingNode::Position;
      else if (kind == "normal") k.kind = ShadingNode::Normal;
      else if (kind == "uv") k.kind = ShadingNode::UV;
      else if (kind == "binf") { k.kind = ShadingNode::BinF; k.op = opc(); in >> k.a >> k.b; }
      else if (kind == "bin3") { k.kind = ShadingNode::Bin3; k.op = opc(); in >> k.a >> k.b; }
      else if (kind == "unf") { k.kind = ShadingNode::UnF; k.op = opc(); in >> k.a; }
      else if (kind == "un3") { k.kind = ShadingNode::Un3; k.op = opc(); in >> k.a; }
      else if (kind == "comp") { k.kind = ShadingNode::Comp; in >> k.a >> k.n; }
      else if (kind == "tovec3") { k.kind = ShadingNode::ToVec3; in >> k.a; if (!(in >> k.b >> k.c)) k.b = k.c = -1; }
      else if (kind == "checker") { k.kind = ShadingNode::Checker; in >> k.a; k.f = rdf(in); }
      else if (kind == "splat") { k.kind = ShadingNode::Splat; in >> k.a; }
      else {
        g_error = "unknown node kind " + kind;
        return false;
      }
      scene.node_table.nodes.push_back(k);
    } else if (kw == "material") {
      std::string name, kind;
      in >> name >> kind;
      Material m;
      m.table = &scene.node_table;
      if (kind == "diffuse_n") {
        m.kind = M_DIFFUSE;
        in >> m.n_albedo;
      } else if (kind == "uber_n") {
        m.kind = M_UBER;
        in >> m.n_albedo >> m.n_rough >> m.n_metal >> m.n_trans;
        m.ior = rdf(in);
      } else if (kind == "metal") {
        m.kind = M_METAL;
        in >> m.n_albedo >> m.n_rough;
      } else if (kind == "glossy" || kind == "glass") {
        m.kind = kind == "glossy" ? M_GLOSSY : M_GLASS;
        in >> m.n_albedo >> m.n_rough >> m.n_ior;
      } else if (kind == "emissive") {
        m.kind = M_EMISSIVE;
        m.color = rd3(in);
      } else if (kind == "diffuse") {
        m.kind = M_DIFFUSE;
        m.color = rd3(in);
      } else if (kind == "uber") {
        m.kind = M_UBER;
        m.color = rd3(in);
        m.roughness = rdf(in);
        m.metallic = rdf(in);
        m.transmission = rdf(in);
        m.ior = rdf(in);
      } else if (kind == "subsurface") {
        m.kind = M_SUBSURFACE;
        m.color = rd3(in);
        m.roughness = rdf(in);
        m.sigma_s = rd3(in);
      } else {
        g_error = "unknown material kind " + kind;
        return false;
      }
      scene.materials.push_back(m);
      scene.material_names.push_back(name);
    } else if (kw == "shape") {
      std::string kind, mat;
      in >> kind >> mat;
      Geometry g;
      g.material = scene.find_material(mat);
      if (g.material < 0) {
        g_error = "Can't find material `" + mat + "`";
        return false;
      }
      if (kind == "rect") {
        vec3 p = rd3(in), ex = rd3(in), ey = rd3(in);
        int flip;
        in >> flip;
        g.kind = S_RECT;
        g.impl = std::make_shared<Rect>(p, ex, ey, flip != 0);
      } else if (kind == "box") {
        vec3 lo = rd3(in), hi = rd3(in);
        g.kind = S_AABB;
        g.impl = std::make_shared<AABB>(lo, hi);
      } else if (kind == "obb") {
        vec3 lo = rd3(in), hi = rd3(in);
        float m[16];
        for (auto& v : m) v = rdf(in);
        mat4 M(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12],
               m[13], m[14], m[15]);
        g.kind = S_OBB;
        g.impl = std::make_shared<OBB>(AABB(lo, hi), M);
      } else if (kind == "sphere") {
        vec3 c = rd3(in);
        float r = rdf(in);
        g.kind = S_SPHERE;
        g.impl = std::make_shared<Sphere>(Sphere{c, r});
      } else if (kind == "disk") {
        vec3 p = rd3(in), n = rd3(in);
        float r = rdf(in);
        g.kind = S_DISK;
        g.impl = std::make_shared<Disk>(p, n, r);
      } else if (kind == "cone") {
        vec3 p = rd3(in), n = rd3(in);
        float r = rdf(in), h = rdf(in);
        g.kind = S_CONE;
        g.impl = std::make_shared<Cone>(p, n, r, h);
      } else if (kind == "plane") {
        vec3 p = rd3(in), n = rd3(in);
        g.kind = S_PLANE;
        g.impl = std::make_shared<Plane>(p, n);
      } else if (kind == "line") {
        vec3 a = rd3(in), b = rd3(in);
        float th = rdf(in);
        g.kind = S_LINE;
        g.impl = std::make_shared<Line>(a, b, th);
      } else if (kind == "cylinder") {
        vec3 a = rd3(in), b = rd3(in);
        float r = rdf(in);
        g.kind = S_CYLINDER;
        g.impl = std::make_shared<Cylinder>(a, b, r);
      } else if (kind == "triangle") {
        vec3 a = rd3(in), b = rd3(in), c = rd3(in);
        g.kind = S_TRIANGLE;
        g.impl = std::make_shared<Triangle>(a, b, c);
      } else if (kind == "rect_state") {
        // state-level records (pine_gpu_scene_add_*_state): the members of an already constructed object of the reference,
        // in member order (geometry.h:92-96, :56-60, :23-25, :134-140, :115-117) -- set as they are, nothing recomputed
        auto r = std::make_shared<Rect>(vec3(0, 0, 0), vec3(1, 0, 0), vec3(0, 1, 0), false);
        r->position = rd3(in), r->ex = rd3(in), r->ey = rd3(in), r->n = rd3(in);
        r->lx = rdf(in), r->ly = rdf(in);
        r->rx = rd3(in), r->ry = rd3(in);
        g.kind = S_RECT;
        g.impl = r;
      } else if (kind == "disk_state") {
        auto d = std::make_shared<Disk>(vec3(0, 0, 0), vec3(0, 0, 1), 1.0f);
        d->position = rd3(in), d->n = rd3(in), d->u = rd3(in), d->v = rd3(in);
        d->r = rdf(in);
        g.kind = S_DISK;
        g.impl = d;
      } else if (kind == "plane_state") {
        auto pl = std::make_shared<Plane>(vec3(0, 0, 0), vec3(0, 0, 1));
        pl->position = rd3(in), pl->n = rd3(in), pl->u = rd3(in), pl->v = rd3(in);
        g.kind = S_PLANE;
        g.impl = pl;
      } else if (kind == "cone_state") {
        auto c = std::make_shared<Cone>(vec3(0, 0, 0), vec3(0, 0, 1), 1.0f, 1.0f);
        c->p = rd3(in), c->n = rd3(in);
        c->r = rdf(in), c->h = rdf(in), c->A = rdf(in), c->A2 = rdf(in), c->S = rdf(in);
        c->bottom.position = rd3(in);  // (of the bottom Disk only the centre and the radius are ever read: Cone::get_aabb, area)
        c->bottom.r = c->r;
        g.kind = S_CONE;
        g.impl = c;
      } else if (kind == "triangle_state") {
        auto t = std::make_shared<Triangle>(vec3(0, 0, 0), vec3(1, 0, 0), vec3(0, 1, 0));
        t->v0 = rd3(in), t->v1 = rd3(in), t->v2 = rd3(in), t->n = rd3(in);
        g.kind = S_TRIANGLE;
        g.impl = t;
      } else if (kind == "mesh" || kind == "mesh_full") {
        int nv, nt;
        in >> nv >> nt;
        auto m = std::make_shared<Mesh>();
        for (int i = 0; i < nv; i++) m->vertices.push_back(rd3(in));
        for (int i = 0; i < 3 * nt; i++) {
          uint32_t a;
          in >> a;
          m->indices.push_back(a);
        }
        if (kind == "mesh_full") {  // per-vertex normals / texcoords (Mesh(vertices, indices, texcoords, normals))
          int has_n, has_t;
          in >> has_n >> has_t;
          if (has_n)
            for (int i = 0; i < nv; i++) m->normals.push_back(rd3(in));
          if (has_t)
            for (int i = 0; i < nv; i++) {
              const float tx = rdf(in), ty = rdf(in);
              m->texcoords.push_back(vec2(tx, ty));
            }
        }
        g.kind = S_MESH;
        g.impl = m;
      } else {
        g_error = "unknown shape kind " + kind;
        return false;
      }
      scene.geometries.push_back(g);
      if (scene.materials[g.material].kind == M_EMISSIVE) {
        Scene::Light L;
        L.kind = Scene::Light::Area;
        L.geom = int(scene.geometries.size()) - 1;
        if (scene.has_env) scene.lights.insert(scene.lights.end() - 1, L);
        else scene.lights.push_back(L);
      }
    } else if (kw == "light") {  // light point|spot|directional ... (user-level ctor arguments)
      std::string kind;
      in >> kind;
      Scene::Light L;
      if (kind == "point") {
        L.kind = Scene::Light::Point;
        L.position = rd3(in);
        L.color = rd3(in);
      } else if (kind == "spot") {  // SpotLight ctor light.cpp:18-34
        L.kind = Scene::Light::Spot;
        L.position = rd3(in);
        L.direction = normalize(rd3(in));
        L.color = rd3(in);
        const float falloff = rdf(in), extra = rdf(in);
        L.falloff_cos = std::cos(falloff);
        L.cutoff_cos = std::cos(falloff + extra);
      } else if (kind == "directional") {
        L.kind = Scene::Light::Directional;
        L.direction = normalize(rd3(in));
        L.color = rd3(in);
      } else {
        g_error = "unknown light kind " + kind;
        return false;
      }
      if (scene.has_env) scene.lights.insert(scene.lights.end() - 1, L);
      else scene.lights.push_back(L);
    } else if (kw == "envlight") {  // envlight sky <sun colour>
      std::string kind;
      in >> kind;
      if (kind != "sky") {
        g_error = "unknown environment light " + kind;
        return false;
      }
      Scene::Light L;
      L.kind = Scene::Light::Sky;
      L.color = rd3(in);
      if (scene.has_env) scene.lights.back() = L;
      else scene.lights.push_back(L);
      scene.has_env = true;
    } else if (kw == "camera") {
      std::string kind;
      int W, H;
      in >> kind >> W >> H;
      if (kind == "thinlens_state") {  // the members of a constructed ThinLenCamera (camera.h:21-26), as they are
        Camera& c = scene.camera;
        c.W = W, c.H = H;
        c.position = rd3(in);
        const vec3 cx = rd3(in), cy = rd3(in), cz = rd3(in);
        c.c2w = mat3(cx, cy, cz);
        const float fx = rdf(in), fy = rdf(in);  // (two reads in one argument list would be evaluated right to left by g++)
        c.fov2d = vec2(fx, fy);
        c.len_radius = rdf(in);
        c.focus_distance = rdf(in);
        continue;
      }
      vec3 from = rd3(in), to = rd3(in);
      float fov = rdf(in), lr = rdf(in), fd = rdf(in);
      scene.camera.init(W, H, from, to, fov, lr, fd);
    } else {
      g_error = "unknown keyword " + kw;
      return false;
    }
  }
  return true;
}

static int g_sampler_kind = SAMPLER_BLUE;  // test-infrastructure switch (oracle_set_sampler)

// PathIntegrator::render (path.cpp:26-41) with parallel_for's scheduling shape (parallel.h:19-57)
// shard_world > 1: only pixels of 8x8 tiles t = ty*tiles_x + tx with t % world == rank are rendered
// (the product's multi-GPU partition, pine_amd/csrc/pine_kernels.hip decode_item); others untouched.
void render_impl(const Scene& scene, const uint8_t* tables, int spp_req, int depth, int threads,
                 int y0, int y1, float* film, float* samples_out, oracle_stats* stats,
                 int shard_rank = 0, int shard_world = 1) {
  int W = scene.camera.W, H = scene.camera.H;
  const int sampler_kind = g_sampler_kind;
  int spp = sampler_kind != SAMPLER_BLUE ? spp_req : bluesobol_effective_spp(spp_req);  // Sobol / Halton: spp() is the request as given
  BlueTables bt = select_tables(tables, sampler_kind != SAMPLER_BLUE ? 1 : spp);
  Integrator integ{&scene, depth};
  if (threads <= 0) threads = int(std::thread::hardware_concurrency());
  if (threads <= 0) threads = 1;
  if (y1 <= y0) {
    y0 = 0;
    y1 = H;
  }
  int first = y0 * W, n_items = (y1 - y0) * W;
  int trace_x = -1, trace_y = -1;  // $PINE_ORACLE_TRACE_PIXEL=x,y (tools/embree_trace_pixel.py): that pixel's accel queries on stderr
  if (const char* e = getenv("PINE_ORACLE_TRACE_PIXEL"))
    if (sscanf(e, "%d,%d", &trace_x, &trace_y) != 2) trace_x = trace_y = -1;
  int batch_count = std::max(threads, n_items / 64);
  int batch_size = std::max(n_items / batch_count, 1);
  std::atomic<int> global_index{0};
  std::vector<Counters> counters(threads);
  auto work = [&](int tid) {
    Sampler sampler;
    sampler.t = bt;
    sampler.kind = sampler_kind;
    sampler.spp = spp;
    sampler.init(W, H);  // RTIntegrator::render integrator.cpp:29
    Counters& cnt = counters[tid];
    while (true) {
      int index = (global_index += batch_size) - batch_size;
      int end_index = std::min(index + batch_size, n_items);
      for (int i = index; i < end_index; i++) {
        int px = (first + i) % W, py = (first + i) / W;
        if (shard_world > 1) {
          int tiles_x = (W + 7) / 8;
          int tile = (py / 8) * tiles_x + px / 8;
          if (tile % shard_world != shard_rank) continue;
        }
        sampler.start_pixel(px, py, 0);
        t_trace_queries = px == trace_x && py == trace_y;
        vec3 L(0.0f);
        for (int si = 0; si < spp; si++, sampler.start_next_sample()) {
          // g++ right-to-left: lens sample first, then pixel jitter (path.cpp:35, Appendix A2)
          vec2 u_lens = sampler.rand2f();
          vec2 jitter = sampler.rand2f();
          vec2 pf((float(px) + jitter.x) / float(W), (float(py) + jitter.y) / float(H));
          Ray ray = scene.camera.gen_ray(pf, u_lens);
          uint64_t v0 = cnt.vertices;
          vec3 Ls = integ.radiance(ray, sampler, Vertex{0, 0, 0.0f, true}, cnt).Lo;
          L += Ls;
          if (samples_out) {
            float* o = samples_out + (size_t(py * W + px) * spp + si) * 4;
            o[0] = Ls.x;
            o[1] = Ls.y;
            o[2] = Ls.z;
            o[3] = float(cnt.vertices - v0);
          }
        }
        if (film) {
          float* o = film + size_t(py * W + px) * 4;
          vec3 m = L / float(spp);
          o[0] = m.x;
          o[1] = m.y;
          o[2] = m.z;
          o[3] = 1.0f;
        }
      }
      if (end_index >= n_items) break;
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto& t : pool) t.join();
  if (stats) {
    stats->camera_samples = uint64_t(n_items) * spp;
    stats->vertices = stats->shadow_rays = stats->bsdf_samples = 0;
    for (auto& c : counters) {
      stats->vertices += c.vertices;
      stats->shadow_rays += c.shadow;
      stats->bsdf_samples += c.bsdf;
    }
    stats->threads = threads;
    stats->spp_effective = spp;
  }
}

}  // namespace

extern "C" {

const char* oracle_last_error(void) { return g_error.c_str(); }

// test hook (tests/test_embree_order.py, tools/embree_order_check.py): the order in which order mode "embree" calls the user callback for
// one ray over n boxes (lower xyz, upper xyz each); hit_t[i] >= 0: primitive i reports a hit at that distance when it lies inside
// (tnear, tfar).  -> number of calls (ids[0 .. cap) filled), *hit_id = closest primitive or -1, *tfar = final ray.tfar
int oracle_embree_order(const float* boxes, int n, const float* ray8, const float* hit_t, int* ids, int cap, int* hit_id, float* tfar) {
  std::vector<std::pair<AABB, int>> bx;
  for (int i = 0; i < n; i++) bx.emplace_back(AABB(vec3(boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]), vec3(boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5])), i);
  embree_order::Tree tree;
  tree.build(bx);
  Ray ray(vec3(ray8[0], ray8[1], ray8[2]), vec3(ray8[3], ray8[4], ray8[5]), ray8[6], ray8[7]);
  int calls = 0;
  *hit_id = -1;
  embree_order::traverse(tree, ray, [&](int gi) {
    if (calls < cap) ids[calls] = gi;
    calls++;
    const float t = hit_t[gi];
    if (t >= 0.0f && t > ray.tmin && t < ray.tmax) ray.tmax = t, *hit_id = gi;
  });
  *tfar = ray.tmax;
  return calls;
}
// test hook (tests/test_embree_order.py): Embree's triangle test as restated, over a triangle list in index order (closest hit; the
// fixture tests/golden/embree_triangles.npz holds the REAL Embree's answers): per ray 7 floats -- prim (-1: miss), t, u, v, Ng
int oracle_embree_triangles(const float* verts, const uint32_t* idx, int nt, const float* rays, int64_t nrays, float* out) {
  for (int64_t i = 0; i < nrays; i++) {
    const float* q = rays + i * 8;
    Ray ray(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7]);
    embree_order::TriHit best{};
    int prim = -1;
    for (int t = 0; t < nt; t++) {
      auto vtx = [&](uint32_t k) { return vec3(verts[3 * k], verts[3 * k + 1], verts[3 * k + 2]); };
      embree_order::TriHit h;
      if (embree_order::tri_test(ray, vtx(idx[3 * t]), vtx(idx[3 * t + 1]), vtx(idx[3 * t + 2]), std::max(ray.tmin, 0.0f), ray.tmax, h)) ray.tmax = h.t, best = h, prim = t;
    }
    float* o = out + i * 7;
    o[0] = float(prim), o[1] = ray.tmax, o[2] = best.u, o[3] = best.v, o[4] = best.ng[0], o[5] = best.ng[1], o[6] = best.ng[2];
  }
  return 0;
}
// test hook: the hierarchy of order mode "embree" over n boxes, one line of 8 child words per node in creation order (>= 0 a node,
// < 0 the complement of a box index, INT32_MIN unused), preceded by the root's child word -> words written, -1 when cap is too small
int oracle_embree_tree(const float* boxes, int n, int* words, int cap) {
  std::vector<std::pair<AABB, int>> bx;
  for (int i = 0; i < n; i++) bx.emplace_back(AABB(vec3(boxes[6 * i], boxes[6 * i + 1], boxes[6 * i + 2]), vec3(boxes[6 * i + 3], boxes[6 * i + 4], boxes[6 * i + 5])), i);
  embree_order::Tree tree;
  tree.build(bx);
  if (1 + 8 * int(tree.nodes.size()) > cap) return -1;
  int k = 0;
  words[k++] = tree.root;
  for (auto& nd : tree.nodes)
    for (int i = 0; i < 8; i++) words[k++] = nd.child[i];
  return k;
}
// test hook: the queries of order mode "embree" on a scene, ray by ray: per ray cap + 10 words -- [count, the geometry indices
// handed to their tests in order ...] (cap words), hit, geometry, tmax bits of the closest-hit query (meshes: their word only),
// the any-hit query's answer, the surface point and normal (bits; zero on a miss)
int oracle_embree_traverse(const char* pscene, const float* rays, int64_t nrays, int cap, uint32_t* out) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  scene.build_accel();
  for (int64_t i = 0; i < nrays; i++) {
    const float* q = rays + i * 8;
    uint32_t* o = out + i * (cap + 10);
    Ray ray(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7]);
    {
      const int keep = g_order_mode;
      g_order_mode = 2;
      o[cap + 3] = scene.hit(ray) ? 1u : 0u;
      g_order_mode = keep;
    }
    int n = 0, hit_geom = -1;
    {  // the answer: Scene::intersect in this order mode (meshes through Embree's triangle test)
      const int keep = g_order_mode;
      g_order_mode = 2;
      Ray r2 = ray;
      SurfaceInteraction it;
      if (scene.intersect(r2, it)) hit_geom = it.geom;
      g_order_mode = keep;
      const float pn[6] = {it.p.x, it.p.y, it.p.z, it.n.x, it.n.y, it.n.z};
      for (int k = 0; k < 6; k++) o[cap + 4 + k] = hit_geom >= 0 ? embree_order::f2u(pn[k]) : 0u;
      // ... and the order of the calls: the meshes, then the user primitives as the hierarchy hands them over
      for (size_t li = 0; li < scene.lbvh.size(); li++) {
        if (1 + n < cap) o[1 + n] = uint32_t(scene.indices[li]);
        n++;
      }
      Ray r3 = ray;  // (replay with the log)
      embree_order::TriHit th;
      const float tnear = std::max(r3.tmin, 0.0f);
      for (size_t li = 0; li < scene.lbvh.size(); li++) {
        const Mesh& mm = scene.geometries[size_t(scene.indices[li])].as<Mesh>();
        scene.lbvh[li]->closest(r3, [&](Ray& rr, int idx) {
          vec3 a, b, c;
          mm.face(size_t(idx), a, b, c);
          if (!embree_order::tri_test(rr, a, b, c, tnear, rr.tmax, th)) return false;
          rr.tmax = th.t;
          return true;
        });
      }
      embree_order::traverse(scene.etree, r3, [&](int gi) {
        if (1 + n < cap) o[1 + n] = uint32_t(gi);
        n++;
        Ray r(r3.o, r3.d, r3.tmin, r3.tmax);
        if (scene.geometries[size_t(gi)].intersect(r)) r3.tmax = r.tmax;
      });
      ray.tmax = r2.tmax;
    }
    o[0] = uint32_t(n);
    o[cap] = hit_geom >= 0 ? 1u : 0u;
    o[cap + 1] = hit_geom >= 0 ? uint32_t(hit_geom) : 0u;
    o[cap + 2] = embree_order::f2u(ray.tmax);
  }
  return 0;
}
void oracle_set_order(int mode) { g_order_mode = mode == 1 || mode == 2 ? mode : 0; }
void oracle_set_sampler(int kind) { g_sampler_kind = kind == SAMPLER_SOBOL ? SAMPLER_SOBOL : kind == SAMPLER_HALTON ? SAMPLER_HALTON : SAMPLER_BLUE; }

int oracle_render(const char* pscene, const uint8_t* tables, int spp, int depth, int threads,
                  int y0, int y1, float* film_out, oracle_stats* stats) {
  if (depth <= 0) {
    g_error = "`PathIntegrator` expect `max_path_length` to be positive";  // path.cpp:12-13
    return 1;
  }
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  auto t0 = std::chrono::steady_clock::now();
  scene.build_accel();  // inside render() in the reference too (integrator.cpp:33)
  render_impl(scene, tables, spp, depth, threads, y0, y1, film_out, nullptr, stats);
  auto t1 = std::chrono::steady_clock::now();
  if (stats) stats->seconds = std::chrono::duration<double>(t1 - t0).count();
  return 0;
}

int oracle_render_shard(const char* pscene, const uint8_t* tables, int spp, int depth, int threads,
                        int shard_rank, int shard_world, float* film_out) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  scene.build_accel();
  render_impl(scene, tables, spp, depth, threads, 0, 0, film_out, nullptr, nullptr, shard_rank, shard_world);
  return 0;
}

int oracle_render_samples(const char* pscene, const uint8_t* tables, int spp, int depth,
                          int threads, float* samples_out) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  scene.build_accel();
  render_impl(scene, tables, spp, depth, threads, 0, 0, nullptr, samples_out, nullptr);
  return 0;
}

static const int kPixels[][2] = {{0, 0}, {1, 0}, {3, 5}, {127, 127}, {128, 5}, {639, 639}};

int oracle_sampler_stream(const uint8_t* tables, int spp_req, float* out, int64_t capacity) {
  int spp = bluesobol_effective_spp(spp_req);
  int64_t need = int64_t(6) * spp * (260 + 270);
  if (capacity < need) return int(-1);
  Sampler s;
  s.t = select_tables(tables, spp);
  s.spp = spp;
  int64_t k = 0;
  for (auto& px : kPixels) {
    s.dimension = 0;
    s.start_pixel(px[0], px[1], 0);
    for (int i = 0; i < spp; i++) {
      for (int d = 0; d < 130; d++) {
        vec2 v = s.get2d();
        out[k++] = v.x;
        out[k++] = v.y;
      }
      s.start_next_sample();
    }
    s.start_pixel(px[0], px[1], 0);
    for (int i = 0; i < spp; i++) {
      for (int d = 0; d < 90; d++) {
        out[k++] = s.get1d();
        vec2 v = s.get2d();
        out[k++] = v.x;
        out[k++] = v.y;
      }
      s.start_next_sample();
    }
  }
  return 0;
}

int64_t oracle_sampler_draws(const uint8_t* tables, const int32_t* cases, int64_t ncases, float* out, int64_t capacity) {
  int64_t k = 0;
  for (int64_t c = 0; c < ncases; c++) {
    const int32_t* q = cases + c * 9;  // kind, spp, film w, film h, px, py, sample index, pattern, calls
    if (q[0] < 0 || q[0] > 2 || q[1] <= 0 || q[6] < 0 || q[7] < 0 || q[7] > 2 || q[8] < 0) return -1;
    const int64_t floats = q[7] == 0 ? 2 * int64_t(q[8]) : q[7] == 1 ? q[8] + q[8] / 2 : q[8];
    if (k + floats > capacity) return -1;
    Sampler s;  // as render_impl sets one up
    s.kind = q[0];
    s.spp = q[0] == SAMPLER_BLUE ? bluesobol_effective_spp(q[1]) : q[1];
    s.t = select_tables(tables, q[0] == SAMPLER_BLUE ? s.spp : 1);
    s.init(q[2], q[3]);
    s.start_pixel(q[4], q[5], 0);
    for (int i = 0; i < q[6]; i++) s.start_next_sample();
    for (int i = 0; i < q[8]; i++) {
      if (q[7] == 2 || (q[7] == 1 && i % 2 == 0)) {
        out[k++] = s.get1d();
      } else {
        const vec2 v = s.get2d();
        out[k++] = v.x;
        out[k++] = v.y;
      }
    }
  }
  return k;
}

int oracle_rng_stream(uint64_t* out, int64_t capacity) {
  if (capacity < 6 * 19) return -1;
  int64_t k = 0;
  for (auto& px : kPixels) {
    uint64_t h = hash_pixel(px[0], px[1], 0);
    out[k++] = h;
    RNG r(h);
    out[k++] = r.s[0];
    out[k++] = r.s[1];
    for (int i = 0; i < 16; i++) {
      float f = r.nextf();
      uint32_t b;
      memcpy(&b, &f, 4);
      out[k++] = b;
    }
  }
  return 0;
}

int oracle_host_math(float* out, int64_t capacity) {
  if (capacity < 8 * 16 + 5 * 9) return -1;
  int64_t k = 0;
  auto push4 = [&](const mat4& m) {
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) out[k++] = m[c][r];
  };
  auto push3 = [&](const mat3& m) {
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) out[k++] = m[c][r];
  };
  mat4 m0 = translate(vec3(0.0f, 0.0f, 0.6f)) * rotate_y(0.4f) * scale(vec3(0.6f, 0.6f, 0.6f));
  mat4 m1 = translate(vec3(-0.6f, 0.0f, 1.0f)) * rotate_y(-0.4f) * scale(vec3(0.6f, 1.3f, 0.6f));
  push4(m0);
  push4(inverse(m0));
  push4(m1);
  push4(inverse(m1));
  push4(look_at(vec3(0, 0, 0), vec3(0, 0, 1)));
  push4(look_at(vec3(0, 1, -4), vec3(0, 1, 0)));
  push4(look_at(vec3(0, 4, -8), vec3(0, 1, 0)));
  push4(rotate_x(0.3f) * rotate_z(-1.1f));
  vec3 ns[] = {vec3(0, 1, 0), vec3(1, 0, 0), vec3(0, 0, -1), normalize(vec3(1, 2, 3)),
               normalize(vec3(-3, 2, 0.5f))};
  for (auto n : ns) push3(coordinate_system(n));
  return 0;
}

int oracle_shapes(const char* pscene, const float* rays, int64_t nrays, float* out,
                  int64_t capacity) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  int64_t k = 0;
  for (auto& g : scene.geometries) {
    if (g.kind == S_MESH) continue;
    for (int64_t i = 0; i < nrays; i++) {
      if (k + 11 > capacity) return -1;
      const float* q = rays + i * 8;
      Ray r(vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), q[6], q[7]);
      out[k++] = g.hit(r) ? 1.0f : 0.0f;
      SurfaceInteraction it;
      Ray r2 = r;
      bool h = g.intersect(r2);
      out[k++] = h ? 1.0f : 0.0f;
      out[k++] = r2.tmax;
      if (h) g.compute_surface_info(r2(), it);
      out[k++] = it.p.x;
      out[k++] = it.p.y;
      out[k++] = it.p.z;
      out[k++] = it.n.x;
      out[k++] = it.n.y;
      out[k++] = it.n.z;
      out[k++] = it.uv.x;
      out[k++] = it.uv.y;
    }
  }
  return 0;
}


int oracle_bxdf(const float* cases, int64_t n, float* out) {
  for (int64_t i = 0; i < n; i++) {
    const float* c = cases + i * 16;
    float* o = out + i * 14;
    for (int k = 0; k < 14; k++) o[k] = 0.0f;
    const int lobe = int(c[0]), calls = int(c[15]);
    if (lobe < 0 || lobe > BX_BSSRDF) {
      g_error = "oracle_bxdf: unknown lobe";
      return 2;
    }
    BXDF b;
    b.kind = BxdfKind(lobe);
    b.albedo = vec3(c[1], c[2], c[3]);
    b.roughness = c[4];
    b.ior = c[5];
    b.wi = vec3(c[6], c[7], c[8]);
    const vec3 wo(c[9], c[10], c[11]);
    if (calls & 1) {
      const vec3 f = b.f(wo);
      o[0] = f.x, o[1] = f.y, o[2] = f.z;
      o[3] = b.pdf(wo);
    }
    o[4] = b.is_delta() ? 1.0f : 0.0f;
    if (calls & 2) {
      Sampler sampler;  // SobolSampler(64) on a 1024 x 1024 image, as `pine_ref bxdf` starts it
      sampler.kind = SAMPLER_SOBOL;
      sampler.spp = 64;
      sampler.init(1024, 1024);
      sampler.start_pixel(int(c[12]), int(c[13]), 0);
      for (int k = 0; k < int(c[14]); k++) sampler.start_next_sample();
      BSDFSample bs;
      if (b.sample(sampler, bs)) {
        o[5] = 1.0f;
        o[6] = bs.wo.x, o[7] = bs.wo.y, o[8] = bs.wo.z;
        o[9] = bs.f.x, o[10] = bs.f.y, o[11] = bs.f.z;
        o[12] = bs.pdf;
        o[13] = bs.is_delta ? 1.0f : 0.0f;
      }
    }
  }
  return 0;
}

int oracle_light_samples(const char* pscene, const float* queries, int64_t n, float* out, int64_t capacity) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  int64_t k = 0;
  for (auto& g : scene.geometries)
    for (int64_t i = 0; i < n; i++) {
      if (k + 13 > capacity) return -1;
      const float* q = queries + i * 6;
      float* o = out + k;
      k += 13;
      for (int j = 0; j < 13; j++) o[j] = 0.0f;
      if (g.kind == S_CYLINDER) {  // the reference has no Cylinder::sample (geometry.h:148)
        o[0] = -1.0f;
        continue;
      }
      const vec3 p(q[0], q[1], q[2]);
      ShapeSample ss;
      if (!g.sample(p, vec2(q[3], q[4]), q[5], ss)) continue;
      o[0] = 1.0f;
      o[1] = ss.p.x, o[2] = ss.p.y, o[3] = ss.p.z;
      o[4] = ss.n.x, o[5] = ss.n.y, o[6] = ss.n.z;
      o[7] = ss.w.x, o[8] = ss.w.y, o[9] = ss.w.z;
      o[10] = ss.distance, o[11] = ss.pdf;
      o[12] = g.pdf(Ray(p, ss.w, 0.0f, ss.distance), ss.n);
    }
  for (auto& L : scene.lights) {  // (the environment light is the last entry)
    if (L.kind == Scene::Light::Area) continue;
    for (int64_t i = 0; i < n; i++) {
      if (k + 9 > capacity) return -1;
      const float* q = queries + i * 6;
      float* o = out + k;
      k += 9;
      for (int j = 0; j < 9; j++) o[j] = 0.0f;
      LightSample ls;
      if (!Integrator::sample_other_light(L, vec3(q[0], q[1], q[2]), vec2(q[3], q[4]), ls)) continue;
      o[0] = 1.0f;
      o[1] = ls.wo.x, o[2] = ls.wo.y, o[3] = ls.wo.z;
      o[4] = ls.distance, o[5] = ls.pdf;
      o[6] = ls.le.x, o[7] = ls.le.y, o[8] = ls.le.z;
    }
  }
  return k == capacity ? 0 : -1;
}

int oracle_node_evals(const char* pscene, const float* queries, int64_t n, float* out, int64_t capacity) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  if (capacity != int64_t(scene.materials.size()) * n * 7) return -1;
  float* o = out;
  for (const Material& m : scene.materials)
    for (int64_t i = 0; i < n; i++, o += 7) {
      const float* q = queries + i * 8;
      const NodeEvalCtx c{vec3(q[0], q[1], q[2]), vec3(q[3], q[4], q[5]), vec2(q[6], q[7])};
      for (int k = 0; k < 7; k++) o[k] = 0.0f;
      const vec3 a = m.albedo_at(c);
      o[0] = a.x, o[1] = a.y, o[2] = a.z;
      if (m.kind == M_EMISSIVE || m.kind == M_DIFFUSE) continue;
      o[3] = m.roughness_at(c);
      if (m.kind == M_UBER) o[4] = m.metallic_at(c), o[5] = m.transmission_at(c), o[6] = m.ior;
      if (m.kind == M_GLOSSY || m.kind == M_GLASS) o[6] = m.ior_at(c);
      if (m.kind == M_SUBSURFACE) o[6] = 1.4f;  // material.h:110
    }
  return 0;
}

int oracle_lobe_choice(const char* pscene, const float* cases, int64_t n, float* out) {
  Scene scene;
  if (!parse_pscene(pscene, scene)) return 2;
  for (int64_t i = 0; i < n; i++) {
    const float* c = cases + i * 16;
    float* o = out + i * 8;
    if (!(c[0] >= 0 && c[0] < float(scene.materials.size())) || scene.materials[size_t(c[0])].kind == M_EMISSIVE) {
      g_error = "oracle_lobe_choice: a case names no material that has a lobe";
      return 2;
    }
    const Material& m = scene.materials[size_t(c[0])];
    const vec3 nn(c[4], c[5], c[6]);
    const NodeEvalCtx nc{vec3(c[1], c[2], c[3]), nn, vec2(c[7], c[8])};
    Sampler sampler;  // SobolSampler(64) on a 1024 x 1024 image, as `pine_ref lobes` starts it
    sampler.kind = SAMPLER_SOBOL;
    sampler.spp = 64;
    sampler.init(1024, 1024);
    sampler.start_pixel(int(c[13]), int(c[14]), 0);
    for (int k = 0; k < int(c[15]); k++) sampler.start_next_sample();
    const BXDF b = material_sample_bxdf(m, nc, vec3(c[9], c[10], c[11]), nn, c[12] != 0.0f, sampler);
    o[0] = float(b.kind);
    o[1] = b.albedo.x, o[2] = b.albedo.y, o[3] = b.albedo.z;
    o[4] = b.kind == BX_DIFFUSE || b.kind == BX_BSSRDF ? 0.0f : b.roughness;
    o[5] = b.kind == BX_DIFFUSE || b.kind == BX_CONDUCTOR ? 0.0f : b.ior;
    o[6] = float(sampler.dimension);
    o[7] = sampler.randf();
  }
  return 0;
}

}  // extern "C"
