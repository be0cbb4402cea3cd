// pine_amd/csrc/pine_math_check.h -- the test hooks pine_gpu_test_math_eval / _compare / _sweep (include/pine_gpu.h):
// the scalar functions of pine_math.h by PINE_GPU_MATH_* code, evaluated on bit patterns and compared with their
// references.  math_eval<FN> is compiled for both sides: pine_test_hooks.hip's test_math_kernel instantiates it for the
// device with the path kernels' flags, and its host build is the device = -1 path.  Everything else here is host code
// (the references, the comparison, the chunked sweep), shared by the product library (pine_test_hooks.hip; the comparison's
// hook, pine_gpu_test_math_compare, is in pine_host.cpp) and the sanitizer build of the host code (tools/sanitize), which
// has no device half.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pine_gpu.h"
#include "pine_math.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <functional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace pine_gpu {

constexpr int math_width(int fn) { return fn == PINE_GPU_MATH_SINCOS ? 2 : 1; }
constexpr int math_arity(int fn) { return fn == PINE_GPU_MATH_CLAMP ? 3 : fn == PINE_GPU_MATH_EXP ? 1 : fn >= PINE_GPU_MATH_ATAN2 ? 2 : 1; }

// out[0] (SINCOS: out[0], out[1]) = FN(a, b, c) by the production functions.  One instantiation per function, so that
// a kernel inlines only the function under test.
template <int FN>
PINE_HD void math_eval(uint32_t ua, uint32_t ub, uint32_t uc, uint32_t* out) {
  const float a = pine_libm::asfloat(ua), b = pine_libm::asfloat(ub), c = pine_libm::asfloat(uc);
  float r = 0.0f;
  if constexpr (FN == PINE_GPU_MATH_SQRT) r = psqrt(a);
  else if constexpr (FN == PINE_GPU_MATH_RCP) r = prcp(a);
  else if constexpr (FN == PINE_GPU_MATH_SIN) r = psin(a);
  else if constexpr (FN == PINE_GPU_MATH_COS) r = pcos(a);
  else if constexpr (FN == PINE_GPU_MATH_SINCOS) {
    float s, co;
    psincos(a, s, co);
    out[1] = pine_libm::asuint(co);
    r = s;
  } else if constexpr (FN == PINE_GPU_MATH_LOG) r = plog(a);
  else if constexpr (FN == PINE_GPU_MATH_ACOS) r = pacos(a);
  else if constexpr (FN == PINE_GPU_MATH_ATAN2) r = patan2(a, b);
  else if constexpr (FN == PINE_GPU_MATH_POW) r = ppow(a, b);
  else if constexpr (FN == PINE_GPU_MATH_DIV) r = a / b;
  else if constexpr (FN == PINE_GPU_MATH_MIN) r = pmin(a, b);
  else if constexpr (FN == PINE_GPU_MATH_MAX) r = pmax(a, b);
  else if constexpr (FN == PINE_GPU_MATH_CLAMP) r = pclamp(a, b, c);
  else if constexpr (FN == PINE_GPU_MATH_EXP) r = pexp(a);
  out[0] = pine_libm::asuint(r);
}

// ---- host code ----
void set_error(const std::string& msg);

namespace math_check {

constexpr int64_t kChunk = int64_t(1) << 26;  // arguments per device launch / host pass of a sweep

// the host build, by code
template <int... FN>
constexpr std::array<void (*)(uint32_t, uint32_t, uint32_t, uint32_t*), sizeof...(FN)> host_table(
    std::integer_sequence<int, FN...>) {
  return {math_eval<FN>...};
}
inline void eval_host(int fn, uint32_t a, uint32_t b, uint32_t c, uint32_t* out) {
  static constexpr auto kTable = host_table(std::make_integer_sequence<int, PINE_GPU_MATH_COUNT>());
  kTable[size_t(fn)](a, b, c, out);
}

// the reference of output k of fn: correctly rounded host IEEE operations, the host's glibc, or the comparison expressions
inline uint32_t reference(int fn, int k, uint32_t ua, uint32_t ub, uint32_t uc) {
  const float a = pine_libm::asfloat(ua), b = pine_libm::asfloat(ub), c = pine_libm::asfloat(uc);
  float r = 0.0f;
  switch (fn) {
    case PINE_GPU_MATH_SQRT: r = ::sqrtf(a); break;
    case PINE_GPU_MATH_RCP: r = 1.0f / a; break;
    case PINE_GPU_MATH_SIN: r = ::sinf(a); break;
    case PINE_GPU_MATH_COS: r = ::cosf(a); break;
    case PINE_GPU_MATH_SINCOS: r = k ? ::cosf(a) : ::sinf(a); break;
    case PINE_GPU_MATH_LOG: r = ::logf(a); break;
    case PINE_GPU_MATH_ACOS: r = ::acosf(a); break;
    case PINE_GPU_MATH_ATAN2: r = ::atan2f(a, b); break;
    case PINE_GPU_MATH_POW: r = ::powf(a, b); break;
    case PINE_GPU_MATH_DIV: r = a / b; break;
    case PINE_GPU_MATH_MIN: r = a < b ? a : b; break;
    case PINE_GPU_MATH_MAX: r = a > b ? a : b; break;
    case PINE_GPU_MATH_CLAMP: {
      const float t = a > b ? a : b;
      r = t < c ? t : c;
      break;
    }
    case PINE_GPU_MATH_EXP: r = ::expf(a); break;
  }
  return pine_libm::asuint(r);
}

// position on the number line, -0 and +0 one apart
inline int64_t ulp_key(uint32_t u) { return (u >> 31) ? -int64_t(u & 0x7fffffffu) - 1 : int64_t(u); }

struct Tally {
  int64_t checked = 0, bad = 0, nan_payload = 0, max_ulp = 0;
  std::vector<uint32_t> examples;  // 5 words each
  void add(int cap, uint32_t a, uint32_t b, uint32_t c, uint32_t got, uint32_t want) {
    checked++;
    if (got == want) return;
    const bool got_nan = (got & 0x7fffffffu) > 0x7f800000u, want_nan = (want & 0x7fffffffu) > 0x7f800000u;
    if (got_nan && want_nan) {
      nan_payload++;
      return;
    }
    bad++;
    if (!got_nan && !want_nan) {
      const int64_t d = ulp_key(got) - ulp_key(want);
      max_ulp = std::max(max_ulp, d < 0 ? -d : d);
    }
    if (int64_t(examples.size()) < int64_t(cap) * 5) examples.insert(examples.end(), {a, b, c, got, want});
  }
  void merge(const Tally& o, int cap) {
    checked += o.checked;
    bad += o.bad;
    nan_payload += o.nan_payload;
    max_ulp = std::max(max_ulp, o.max_ulp);
    for (size_t i = 0; i < o.examples.size() && int64_t(examples.size()) < int64_t(cap) * 5; i++) examples.push_back(o.examples[i]);
  }
  void report(int64_t* stats, uint32_t* out) const {
    stats[0] = checked;
    stats[1] = bad;
    stats[2] = nan_payload;
    stats[3] = max_ulp;
    if (!examples.empty()) memcpy(out, examples.data(), examples.size() * 4);
  }
};

// host threads: min(16, $OMP_NUM_THREADS, hardware threads) -- never the hardware count alone (a shared machine's share
// is far smaller)
inline int threads() {
  int n = int(std::thread::hardware_concurrency());
  if (n < 1) n = 1;
  n = std::min(n, 16);
  if (const char* e = getenv("OMP_NUM_THREADS")) {
    const int v = atoi(e);
    if (v > 0) n = std::min(n, v);
  }
  return n;
}
// f(lo, hi, tally) on contiguous ranges of [0, n), one per thread, merged in order: the examples are the first ones
template <class F>
Tally parallel(int64_t n, int cap, F f) {
  const int nt = int(std::max<int64_t>(1, std::min<int64_t>(threads(), n / 4096)));
  std::vector<Tally> part(size_t(nt), Tally{});
  std::vector<std::thread> th;
  for (int t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * t / nt, n * (t + 1) / nt, part[size_t(t)]); });
  for (auto& x : th) x.join();
  Tally all;
  for (const Tally& t : part) all.merge(t, cap);
  return all;
}

inline bool bad_args(int fn, int64_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c) {
  if (fn < 0 || fn >= PINE_GPU_MATH_COUNT || n < 0 || !a || (math_arity(fn) > 1 && !b) || (math_arity(fn) > 2 && !c)) {
    set_error("bad argument");
    return true;
  }
  return false;
}

inline int eval_host_arrays(int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n, uint32_t* got) {
  if (bad_args(fn, n, a, b, c)) return -1;
  if (!got) {
    set_error("bad argument");
    return -1;
  }
  const int w = math_width(fn), ar = math_arity(fn);
  parallel(n, 0, [&](int64_t lo, int64_t hi, Tally&) {
    for (int64_t i = lo; i < hi; i++) eval_host(fn, a[i], ar > 1 ? b[i] : 0u, ar > 2 ? c[i] : 0u, got + i * w);
  });
  return 0;
}

inline int compare(int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* got, int64_t n,
                   int64_t* stats, uint32_t* examples, int cap) {
  if (bad_args(fn, n, a, b, c) || !got || !stats || cap < 0 || (cap > 0 && !examples)) {
    set_error("bad argument");
    return -1;
  }
  const int w = math_width(fn), ar = math_arity(fn);
  parallel(n, cap, [&](int64_t lo, int64_t hi, Tally& t) {
    for (int64_t i = lo; i < hi; i++) {
      const uint32_t ua = a[i], ub = ar > 1 ? b[i] : 0u, uc = ar > 2 ? c[i] : 0u;
      for (int k = 0; k < w; k++) t.add(cap, ua, w > 1 ? uint32_t(k) : ub, uc, got[i * w + k], reference(fn, k, ua, ub, uc));
    }
  }).report(stats, examples);
  return 0;
}

inline bool bad_sweep_args(int fn, int swept_arg, uint64_t count, int64_t* stats, uint32_t* examples, int cap) {
  if (fn < 0 || fn >= PINE_GPU_MATH_COUNT || swept_arg < 0 || swept_arg >= math_arity(fn) || count > (uint64_t(1) << 32) ||
      !stats || cap < 0 || (cap > 0 && !examples)) {
    set_error("bad argument");
    return true;
  }
  return false;
}
// fills h[0, len * width) with fn at the arguments of chunk (start, len); returns < 0 on failure (the error is set)
using ChunkEval = std::function<int(uint32_t start, int64_t len, uint32_t* h)>;
// The sweep: argument swept_arg = first + k * stride (mod 2^32) for k < count, the others fixed_bits, in chunks of
// kChunk; h holds one chunk's results.  device_chunk evaluates on the device; empty: the host build, here.
inline int sweep(int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count, uint32_t stride,
                 const ChunkEval& device_chunk, uint32_t* h, int64_t* stats, uint32_t* examples, int cap) {
  const int w = math_width(fn);
  Tally all;
  for (uint64_t k0 = 0; k0 < count; k0 += uint64_t(kChunk)) {
    const int64_t len = int64_t(std::min<uint64_t>(uint64_t(kChunk), count - k0));
    const uint32_t start = first + uint32_t(k0) * stride;  // (mod 2^32)
    if (device_chunk && device_chunk(start, len, h) < 0) return -1;
    all.merge(parallel(len, cap, [&](int64_t lo, int64_t hi, Tally& t) {
                for (int64_t i = lo; i < hi; i++) {
                  const uint32_t v = start + uint32_t(i) * stride;
                  const uint32_t ua = swept_arg == 0 ? v : fixed_bits, ub = swept_arg == 1 ? v : fixed_bits,
                                 uc = swept_arg == 2 ? v : fixed_bits;
                  if (!device_chunk) eval_host(fn, ua, ub, uc, h + i * w);
                  for (int k = 0; k < w; k++)
                    t.add(cap, ua, w > 1 ? uint32_t(k) : ub, uc, h[i * w + k], reference(fn, k, ua, ub, uc));
                }
              }),
              cap);
  }
  all.report(stats, examples);
  return 0;
}
inline int sweep_host(int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count, uint32_t stride,
                      int64_t* stats, uint32_t* examples, int cap) {
  if (bad_sweep_args(fn, swept_arg, count, stats, examples, cap)) return -1;
  std::vector<uint32_t> h(size_t(std::min<uint64_t>(count, uint64_t(kChunk))) * size_t(math_width(fn)) + 2);
  return sweep(fn, fixed_bits, swept_arg, first, count, stride, ChunkEval(), h.data(), stats, examples, cap);
}

}  // namespace math_check

}  // namespace pine_gpu
