// pine_amd/csrc/pine_test_hooks.hip -- the device unit-test hooks of the C ABI (include/pine_gpu.h): the building blocks
// of the path kernels (scalar math, samplers, RNG, traversal, shapes) run on their own and read back, for the parity
// tests.  Built with the path kernels' flags (Makefile CXXFLAGS, -ffp-contract=off): tests/test_device_math.py relies on
// it.  The host-only hooks live in pine_host.cpp.
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <type_traits>
#include <utility>

#include "pine_plan.h"
#include "pine_math_check.h"

namespace pine_gpu {

// ------------------------------------------------------------------------------------------------
// Device-side unit-test kernels (parity of the building blocks against the oracle)
// ------------------------------------------------------------------------------------------------
__global__ void test_sincos_kernel(const float* x, long long n, float* s, float* c) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    // the branch-free shared-reduction form the kernels call, cross-checked against the two single functions
    float sn, cs;
    psincos(x[i], sn, cs);
    const float s1 = psin(x[i]), c1 = pcos(x[i]);
    const bool same = __float_as_uint(s1) == __float_as_uint(sn) && __float_as_uint(c1) == __float_as_uint(cs);
    s[i] = same ? sn : __uint_as_float(0x7fc00001u);
    c[i] = same ? cs : __uint_as_float(0x7fc00001u);
  }
}
__global__ void test_powlog_kernel(const float* x, const float* y, long long n, float* p, float* l) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    p[i] = ppow(x[i], y[i]);
    l[i] = plog(x[i]);
  }
}
__global__ void test_atan_kernel(const float* y, const float* x, long long n, float* at2, float* ac) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    at2[i] = patan2(y[i], x[i]);
    ac[i] = pacos(x[i]);
  }
}
// pine_gpu_test_math_*: the scalar functions of pine_math.h on bit patterns (pine_math_check.h has math_eval<FN>).
// inputs from arrays (a != NULL; b, c as the arity needs) or generated: argument `swept` = first + i * stride, the others
// `fixed`.  out: n * math_width(FN) words.
template <int FN>
__global__ void test_math_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t fixed, int swept,
                                 uint32_t first, uint32_t stride, long long n, uint32_t* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ua, ub = fixed, uc = fixed;
  if (a) {
    ua = a[i];
    if (math_arity(FN) > 1) ub = b[i];
    if (math_arity(FN) > 2) uc = c[i];
  } else {
    const uint32_t v = first + uint32_t(i) * stride;
    ua = swept == 0 ? v : fixed;
    ub = swept == 1 ? v : fixed;
    uc = swept == 2 ? v : fixed;
  }
  math_eval<FN>(ua, ub, uc, out + i * math_width(FN));
}
__constant__ int kTestPixels[6][2] = {{0, 0}, {1, 0}, {3, 5}, {127, 127}, {128, 5}, {639, 639}};
__global__ void test_sampler_kernel(DTables T, int spp, float* out) {
  // one thread per (pixel, pass); layout identical to oracle_sampler_stream
  const int pix = blockIdx.x;
  if (threadIdx.x != 0) return;
  float* o = out + size_t(pix) * spp * (260 + 270);
  DSampler s;
  s.px = kTestPixels[pix][0];
  s.py = kTestPixels[pix][1];
  s.dimension = 0;
  s.index = 0;
  size_t k = 0;
  for (int i = 0; i < spp; i++) {
    for (int d = 0; d < 130; d++) {
      const f2 v = sampler_get2d(T, s);
      o[k++] = v.x;
      o[k++] = v.y;
    }
    s.dimension = 0;
    s.index++;
  }
  s.index = 0;
  for (int i = 0; i < spp; i++) {
    for (int d = 0; d < 90; d++) {
      o[k++] = sampler_get1d(T, s);
      const f2 v = sampler_get2d(T, s);
      o[k++] = v.x;
      o[k++] = v.y;
    }
    s.dimension = 0;
    s.index++;
  }
}
// pine_gpu_test_sampler_draws: one case (9 ints: kind, spp, film w, film h, px, py, sample index, pattern, calls) through the
// sampler front the kernels call, started as they start it; host pass and device pass.
constexpr int kDrawCaseInts = 9, kDrawMaxCases = 65536, kDrawMaxCalls = 65536;
PINE_HD bool draw_is_get1d(int pattern, int call) { return pattern == 2 || (pattern == 1 && (call & 1) == 0); }
template <int MODE>
PINE_HD void test_draws_case(const DTables& T, const int32_t* q, float* o) {
  DSampler s;
  s.px = q[4];
  s.py = q[5];
  s.index = q[6];
  s.dimension = T.kind == 2 ? 2 : 0;  // (HaltonSampler::start_pixel / start_next_sample: dimension = 2)
  for (int i = 0; i < q[8]; i++) {
    if (draw_is_get1d(q[7], i)) {
      *o++ = sampler_get1d<MODE>(T, s);
    } else {
      const f2 v = sampler_get2d<MODE>(T, s);
      *o++ = v.x;
      *o++ = v.y;
    }
  }
}
// one thread per case; MODE & kSmLds: the launch has kLdsLaneStride threads a workgroup and every lane keeps its own pixel's slice,
// as a lane of the megakernel or of the AO kernel does for the work item it holds
template <int MODE>
__global__ void test_draws_kernel(DTables tables, const int32_t* cases, const long long* offsets, int n, float* out) {
  const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
  if constexpr ((MODE & kSmLds) != 0) {
    __shared__ int lds_sobol[kLdsSamplerDims * 256 / 4];
    __shared__ uint32_t lds_tile[kLdsTileDwords * kLdsLaneStride];
    stage_sobol_rows(lds_sobol, tables, threadIdx.x, kLdsLaneStride);
    const DTables T = lane_tables(tables, lds_sobol, lds_tile, threadIdx.x);
    if (i < n) load_lane_slice(tables, cases[i * kDrawCaseInts + 4], cases[i * kDrawCaseInts + 5], lds_tile, threadIdx.x);
    __syncthreads();
    if (i < n) test_draws_case<MODE>(T, cases + i * kDrawCaseInts, out + offsets[i]);
  } else {
    if (i < n) test_draws_case<MODE>(tables, cases + i * kDrawCaseInts, out + offsets[i]);
  }
}
__global__ void test_rng_kernel(unsigned long long* out) {
  const int pix = threadIdx.x;
  if (pix >= 6) return;
  unsigned long long* o = out + pix * 19;
  const uint64_t h = hash_pixel(kTestPixels[pix][0], kTestPixels[pix][1], 0);
  o[0] = h;
  DRng g = rng_seed(h);
  o[1] = g.s0;
  o[2] = g.s1;
  for (int i = 0; i < 16; i++) o[3 + i] = (unsigned long long)(uint32_t)as_int(rng_nextf(g));
}
// The primitives a ray's traversal tests, in order, and its result: the nested loops of the scene-in-LDS variants
// (FLAT = false: scene_traverse / mesh_traverse, pine_traverse.h) or the flat state machine of the F_LDS_TOP variants (pine_trav.h).
// One thread per ray, 64 per block; out: per ray `cap` words closest (count, words...), 4 result words (hit, geometry,
// triangle, tmax bits), `cap` words any-hit, 1 result word.
// (MODE 2: both queries in EmbreeAccel's order, PINE_GPU_FLAG_ORDER_EMBREE -- scene_traverse_embree for the closest hit,
//  scene_occluded_embree for the any-hit query; tests/test_embree_order.py compares each with the real Embree's)
template <int MODE>
__global__ void __launch_bounds__(64) test_traverse_kernel(DeviceScene S, const float* rays, long long nrays, int cap, unsigned* out) {
  constexpr bool FLAT = MODE == 1;
  constexpr unsigned F = FLAT ? (F_ALL | F_LDS_TOP) : MODE == 2 ? (F_ALL | F_EMBREE) : F_ALL;
  using StackT = typename std::conditional<FLAT, unsigned short, int>::type;
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  StackT* const stack = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  const SceneView V = scene_view_global(S);
  const long long i = blockIdx.x * 64ll + threadIdx.x;
  const bool live = i < nrays;
  const float* q = rays + (live ? i : 0) * 8;
  unsigned* o = out + (live ? i : 0) * (2ll * cap + 5);
  for (int pass = 0; pass < 2; pass++) {
    DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};
    TravLog log{o + (pass ? cap + 4 : 0) + 1, 0, cap - 1};
    bool hit = false;
    int geom = 0, prim = 0;
    if constexpr (FLAT) {
      TravState ts;
      trav_begin(V, ts);
      if (!live) ts.done = 1;
      const DRayOct oct = make_oct(ray);
      if (pass == 0) trav_trips<false, F, 64>(V, ray, oct, ts, stack, 0, 1 << 30, nullptr, &log);
      else trav_trips<true, F, 64>(V, ray, oct, ts, stack, 0, 1 << 30, nullptr, &log);
      hit = ts.hit_geom >= 0;
      geom = ts.hit_geom, prim = ts.hit_prim;
    } else if (live) {
      hit = pass == 0 ? scene_traverse<false, F, 64>(V, ray, stack, geom, prim, &log) : scene_traverse<true, F, 64>(V, ray, stack, geom, prim, &log);
    }
    if (live) {
      o[pass ? cap + 4 : 0] = unsigned(log.n);
      if (pass == 0) {
        o[cap] = hit ? 1u : 0u;
        o[cap + 1] = hit ? unsigned(geom & kPrimIndexMask) : 0u;
        // (a mesh hit reports the triangle's index within its mesh, as the reference does; elsewhere the word is unused: 0)
        const bool on_mesh = hit && (geom >> kPrimKindShift) == SHAPE_MESH;
        o[cap + 2] = on_mesh ? unsigned(prim - S.bvhs[as_int(S.shapes[geom & kPrimIndexMask].f[2])].prim_base) : 0u;
        o[cap + 3] = __float_as_uint(ray.tmax);
      } else {
        o[2 * cap + 4] = hit ? 1u : 0u;
      }
    }
  }
}
__global__ void test_shapes_kernel(const DShape* shapes, int num_shapes, const float* rays, long long nrays,
                                   float* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nrays * num_shapes) return;
  const int g = int(i / nrays);
  const long long r = i % nrays;
  const float* q = rays + r * 8;
  DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};
  float* o = out + i * 11;
  const DShape* S = &shapes[g];
  o[0] = shape_hit(S, ray) ? 1.0f : 0.0f;
  DRay r2 = ray;
  const bool h = shape_intersect(S, r2);
  o[1] = h ? 1.0f : 0.0f;
  o[2] = r2.tmax;
  DSurface it;
  it.p = it.n = mk3(0.0f);
  it.uv = f2{0, 0};
  if (h) shape_surface_info(S, ray_at(r2, r2.tmax), it);
  o[3] = it.p.x, o[4] = it.p.y, o[5] = it.p.z;
  o[6] = it.n.x, o[7] = it.n.y, o[8] = it.n.z;
  o[9] = it.uv.x, o[10] = it.uv.y;
}
// pine_gpu_test_bxdf: one BSDF lobe call per case (16 floats in, 14 out: the layout of `pine_ref bxdf`, include/pine_gpu.h).
// The same body runs on the host (device = -1) and as a kernel; F is the path kernels' feature mask.
constexpr unsigned kBxdfNarrow[6] = {0u, F_UBER, F_SSS, F_UBER, F_UBER, F_SSS};  // the narrowest mask that contains each lobe
template <unsigned F>
PINE_HD void test_bxdf_case(const float* c, float* o) {
  DBxdf b;
  b.kind = int(c[0]);
  b.albedo = ld3(c + 1);
  b.albedo_over_pi = b.albedo / kPi;
  b.roughness = c[4];
  b.ior = c[5];
  b.wi = ld3(c + 6);
  const f3 wo = ld3(c + 9);
  const int calls = int(c[15]);
  for (int k = 0; k < 14; k++) o[k] = 0.0f;
  if (calls & 1) {
    const f3 f = bxdf_f<F>(b, wo);
    o[0] = f.x, o[1] = f.y, o[2] = f.z;
    o[3] = bxdf_pdf<F>(b, wo);
  }
  o[4] = bxdf_is_delta<F>(b) ? 1.0f : 0.0f;
  if (calls & 2) {
    // SobolSampler(64) on a 1024 x 1024 image, set up as a plan sets it up; in this mode nothing is read from the tables
    DTables T{};
    T.kind = 1;
    sobol_sampler_params(T, 64, 1024, 1024);
    DSampler s;
    s.px = int(c[12]);
    s.py = int(c[13]);
    s.index = int(c[14]);
    s.dimension = 0;
    DBsdfSample bs;
    if (bxdf_sample<F, kSmSobol>(b, T, s, bs)) {
      o[5] = 1.0f;
      o[6] = bs.wo.x, o[7] = bs.wo.y, o[8] = bs.wo.z;
      o[9] = bs.f.x, o[10] = bs.f.y, o[11] = bs.f.z;
      o[12] = bs.pdf;
      o[13] = bs.is_delta ? 1.0f : 0.0f;
    }
  }
}
// one thread per entry of idx (idx = NULL: per case)
template <unsigned F>
__global__ void __launch_bounds__(64) test_bxdf_kernel(const float* cases, const int* idx, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n) return;
  const long long i = idx ? idx[t] : t;
  test_bxdf_case<F>(cases + i * 16, out + i * 14);
}
// pine_gpu_test_light_samples: shape_sample + shape_pdf per (geometry, query), light_sample_other per (light, query)
PINE_HD void test_shape_sample_case(const DShape* S, const float* tri_verts, const float* q, float* o) {
  for (int k = 0; k < 13; k++) o[k] = 0.0f;
  if (S->kind == SHAPE_CYLINDER) {  // the reference has no Cylinder::sample (geometry.h:148)
    o[0] = -1.0f;
    return;
  }
  const f3 p = ld3(q);
  DShapeSample ss;
  if (!shape_sample(S, tri_verts, p, f2{q[3], q[4]}, q[5], ss)) return;
  o[0] = 1.0f;
  o[1] = ss.p.x, o[2] = ss.p.y, o[3] = ss.p.z;
  o[4] = ss.n.x, o[5] = ss.n.y, o[6] = ss.n.z;
  o[7] = ss.w.x, o[8] = ss.w.y, o[9] = ss.w.z;
  o[10] = ss.distance, o[11] = ss.pdf;
  o[12] = shape_pdf(S, DRay{p, ss.w, 0.0f, ss.distance}, ss.n);
}
PINE_HD void test_light_sample_case(const DLight* L, const float* q, float* o) {
  for (int k = 0; k < 9; k++) o[k] = 0.0f;
  f3 w, le;
  float distance, pdf;
  if (!light_sample_other(L, nullptr, ld3(q), f2{q[3], q[4]}, w, distance, pdf, le)) return;  // (ImageSky: pine_gpu_test_env_light)
  o[0] = 1.0f;
  o[1] = w.x, o[2] = w.y, o[3] = w.z;
  o[4] = distance, o[5] = pdf;
  o[6] = le.x, o[7] = le.y, o[8] = le.z;
}
__global__ void __launch_bounds__(64) test_light_samples_kernel(const DShape* shapes, int num_shapes, const float* tri_verts, const DLight* lights,
                                                               int num_lights, const float* queries, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n * (num_shapes + num_lights)) return;
  const long long k = t / n, i = t % n;
  if (k < num_shapes) test_shape_sample_case(&shapes[k], tri_verts, queries + i * 6, out + t * 13);
  else test_light_sample_case(&lights[k - num_shapes], queries + i * 6, out + n * num_shapes * 13 + (t - n * num_shapes) * 9);
}
// pine_gpu_test_env_light: ImageSky's or Atmosphere's sample(u2), then color(wo) and pdf(wo) of the query's own direction
PINE_HD void test_env_light_case(const DLight* L, const float* env, const float* q, float* o) {
  f3 w, le;
  float pdf;
  int px, py;
  const bool atmosphere = L->kind == LIGHT_ATMOSPHERE;
  if (atmosphere) atmosphere_sample(L, env, f2{q[0], q[1]}, w, pdf, le, px, py);
  else image_sky_sample(L, env, f2{q[0], q[1]}, w, pdf, le, px, py);
  o[0] = float(px), o[1] = float(py), o[2] = pdf;
  o[3] = w.x, o[4] = w.y, o[5] = w.z;
  o[6] = le.x, o[7] = le.y, o[8] = le.z;
  const f3 wo = ld3(q + 2);
  const f3 c = atmosphere ? atmosphere_sky_color(L, wo) : image_sky_color(L, env, wo);
  o[9] = c.x, o[10] = c.y, o[11] = c.z;
  o[12] = image_sky_pdf(L, env, wo);
}
// pine_gpu_test_atmosphere_color: atmosphere_color(direction, sun_dir, 8, flag) of a query of 7 floats
PINE_HD void test_atmosphere_color_case(const float* q, float* o) {
  const f3 c = atmosphere_color_of(ld3(q), ld3(q + 3), q[6] != 0.0f);
  o[0] = c.x, o[1] = c.y, o[2] = c.z;
}
__global__ void __launch_bounds__(64) test_atmosphere_color_kernel(const float* queries, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n) return;
  test_atmosphere_color_case(queries + t * 7, out + t * 3);
}
// pine_gpu_test_env_light_sample: the light sampler's own call for the environment light -- light_sample_other with the plan's
// env buffer -- as pine_gpu_test_light_samples' 9-float record
PINE_HD void test_env_light_sample_case(const DLight* L, const float* env, const float* q, float* o) {
  for (int k = 0; k < 9; k++) o[k] = 0.0f;
  f3 w, le;
  float distance, pdf;
  if (!light_sample_other(L, env, ld3(q), f2{q[3], q[4]}, w, distance, pdf, le)) return;
  o[0] = 1.0f;
  o[1] = w.x, o[2] = w.y, o[3] = w.z;
  o[4] = distance, o[5] = pdf;
  o[6] = le.x, o[7] = le.y, o[8] = le.z;
}
__global__ void __launch_bounds__(64) test_env_light_sample_kernel(DLight L, const float* env, const float* queries, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n) return;
  test_env_light_sample_case(&L, env, queries + t * 5, out + t * 9);
}
__global__ void __launch_bounds__(64) test_env_light_kernel(DLight L, const float* env, const float* queries, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n) return;
  test_env_light_case(&L, env, queries + t * 5, out + t * 13);
}
// pine_gpu_test_material_params: material_params<F_ALL> of one material at one query (p, n, uv) -> 10 floats
PINE_HD void test_material_params_case(const DMaterial* m, const DNodeOp* ops, const float* tex, const float* q, float* o) {
  const MatParams mp = material_params<F_ALL>(m, ops, tex, ld3(q), ld3(q + 3), f2{q[6], q[7]});
  o[0] = mp.albedo.x, o[1] = mp.albedo.y, o[2] = mp.albedo.z;
  o[3] = mp.albedo_over_pi.x, o[4] = mp.albedo_over_pi.y, o[5] = mp.albedo_over_pi.z;
  o[6] = mp.roughness, o[7] = mp.metallic, o[8] = mp.transmission, o[9] = mp.ior;
}
__global__ void __launch_bounds__(64) test_material_params_kernel(const DMaterial* mats, int num_mats, const DNodeOp* ops, const float* tex, const float* queries,
                                                                 long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= n * num_mats) return;
  test_material_params_case(&mats[t / n], ops, tex, queries + (t % n) * 8, out + t * 10);
}
// pine_gpu_test_choose_lobe: material_params, then choose_lobe as the path kernels call it, one thread per (after_walk, case).
// The pixel's RNG lives in a local; the sampler is SobolSampler(64) on a 1024 x 1024 image, as in test_bxdf_case.  A slot the
// chosen lobe does not have (bxdf.h:38-138: no roughness in Diffuse / BSSRDF, no ior in Diffuse / Conductor) is written as 0.
__global__ void __launch_bounds__(64) test_choose_lobe_kernel(const DMaterial* mats, const DNodeOp* ops, const float* tex, const float* cases, long long n, float* out) {
  const long long t = blockIdx.x * 64ll + threadIdx.x;
  if (t >= 2 * n) return;
  const float* c = cases + (t % n) * 16;
  float* o = out + t * 8;
  const DMaterial* mat = &mats[int(c[0])];  // (checked against the material count on the host)
  const f3 nn = ld3(c + 4);
  DTables T{};
  T.kind = 1;
  sobol_sampler_params(T, 64, 1024, 1024);
  DSampler s;
  s.px = int(c[13]);
  s.py = int(c[14]);
  s.index = int(c[15]);
  s.dimension = 0;
  DRng g = rng_seed(hash_pixel(s.px, s.py, 0));  // Sampler::start_pixel(p, 0): path.cpp:32
  const MatParams mp = material_params<F_ALL>(mat, ops, tex, ld3(c + 1), nn, f2{c[7], c[8]});
  DBxdf bx;
  choose_lobe<F_ALL, kSmSobol>(mat, mp, ld3(c + 9), nn, c[12] != 0.0f, t >= n, [&]() -> DRng { return g; }, [&](const DRng& x) { g = x; }, T, s, bx);
  o[0] = float(bx.kind);
  o[1] = mp.albedo.x, o[2] = mp.albedo.y, o[3] = mp.albedo.z;
  o[4] = bx.kind == BX_DIFFUSE || bx.kind == BX_BSSRDF ? 0.0f : bx.roughness;
  o[5] = bx.kind == BX_DIFFUSE || bx.kind == BX_CONDUCTOR ? 0.0f : bx.ior;
  o[6] = float(s.dimension);
  o[7] = rng_nextf(g);
}
}  // namespace pine_gpu

using namespace pine_gpu;

extern "C" {

int pine_gpu_plan_test_traverse_baked(pine_gpu_plan* p, const float* rays, int64_t nrays, uint32_t* out) {
  if (!p || !rays || !out || nrays <= 0) {
    set_error("null argument");
    return -1;
  }
  const hipModule_t baked = p->scene_kernel.baked_module();
  if (!baked) {
    set_error("the plan has no baked scene (PINE_GPU_FLAG_SPECIALIZE, a scene that qualifies)");
    return -1;
  }
  HIP_OK(hipSetDevice(p->device));
  hipFunction_t fn;
  HIP_OK(hipModuleGetFunction(&fn, baked, "pine_baked_traverse_test"));
  DeviceBuffer<float> dr;
  DeviceBuffer<unsigned> dout;
  if (dr.upload(rays, size_t(nrays) * 8, __func__) || dout.alloc(size_t(nrays) * 4, __func__)) return -1;
  float* rays_dev = dr;
  unsigned* out_dev = dout;
  long long n = nrays;
  void* args[] = {&rays_dev, &n, &out_dev};
  if (const hipError_t e = hipModuleLaunchKernel(fn, unsigned((nrays + 63) / 64), 1, 1, 64, 1, 1, 0, nullptr, args, nullptr)) return hip_error(__func__, e);
  return dout.download(out, size_t(nrays) * 4, __func__);
}

// ---- device unit-test hooks -------------------------------------------------------------------
// Every hook below reads: validate the arguments, build the inputs, upload them, allocate the outputs, launch, check the launch,
// download.  Its buffers are locals (pine_device_buffer.h); the first failing HIP call is reported under the hook's own name.
int pine_gpu_test_sincos(int device, const float* x, int64_t n, float* s, float* c) {
  if (need_device(device)) return -1;
  DeviceBuffer<float> dx, ds, dc;
  if (dx.upload(x, n, __func__) || ds.alloc(n, __func__) || dc.alloc(n, __func__)) return -1;
  if (n > 0) hipLaunchKernelGGL(test_sincos_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dx.get(), (long long)n, ds.get(), dc.get());
  return hip_launch_check(__func__) || ds.download(s, n, __func__) || dc.download(c, n, __func__) ? -1 : 0;
}
int pine_gpu_test_powlog(int device, const float* x, const float* y, int64_t n, float* pw, float* lg) {
  if (need_device(device)) return -1;
  DeviceBuffer<float> dx, dy, dp, dl;
  if (dx.upload(x, n, __func__) || dy.upload(y, n, __func__) || dp.alloc(n, __func__) || dl.alloc(n, __func__)) return -1;
  if (n > 0) hipLaunchKernelGGL(test_powlog_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dx.get(), dy.get(), (long long)n, dp.get(), dl.get());
  return hip_launch_check(__func__) || dp.download(pw, n, __func__) || dl.download(lg, n, __func__) ? -1 : 0;
}
int pine_gpu_test_atan(int device, const float* y, const float* x, int64_t n, float* at2, float* ac) {
  if (need_device(device)) return -1;
  DeviceBuffer<float> dy, dx, da, dc;
  if (dy.upload(y, n, __func__) || dx.upload(x, n, __func__) || da.alloc(n, __func__) || dc.alloc(n, __func__)) return -1;
  if (n > 0) hipLaunchKernelGGL(test_atan_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dy.get(), dx.get(), (long long)n, da.get(), dc.get());
  return hip_launch_check(__func__) || da.download(at2, n, __func__) || dc.download(ac, n, __func__) ? -1 : 0;
}

// ---- pine_gpu_test_math_*: the scalar functions over bit patterns against their references (pine_math_check.h) -----
extern "C++" {
namespace {
template <int FN>
void math_launch(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t fixed, int swept, uint32_t first,
                 uint32_t stride, long long n, uint32_t* out) {
  hipLaunchKernelGGL(test_math_kernel<FN>, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, a, b, c, fixed, swept, first,
                     stride, n, out);
}
using MathLaunch = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, int, uint32_t, uint32_t, long long,
                            uint32_t*);
template <int... FN>
constexpr std::array<MathLaunch, sizeof...(FN)> math_launch_table(std::integer_sequence<int, FN...>) {
  return {math_launch<FN>...};
}
constexpr std::array<MathLaunch, PINE_GPU_MATH_COUNT> kMathLaunch =
    math_launch_table(std::make_integer_sequence<int, PINE_GPU_MATH_COUNT>());
}  // namespace
}  // extern "C++"

int pine_gpu_test_math_eval(int device, int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n, uint32_t* got) {
  if (device < 0) return math_check::eval_host_arrays(fn, a, b, c, n, got);
  if (math_check::bad_args(fn, n, a, b, c)) return -1;
  if (!got) {
    set_error("bad argument");
    return -1;
  }
  if (need_device(device)) return -1;
  const int w = math_width(fn), ar = math_arity(fn);
  const int64_t m = std::max<int64_t>(1, std::min(n, math_check::kChunk));
  DeviceBuffer<uint32_t> d[4];  // a, b, c as the arity needs; the results
  for (int k = 0; k < 4; k++)
    if ((k < ar || k == 3) && d[k].alloc(size_t(m) * (k == 3 ? w : 1), __func__)) return -1;
  const uint32_t* src[3] = {a, b, c};
  for (int64_t i0 = 0; i0 < n; i0 += m) {
    const int64_t len = std::min(m, n - i0);
    for (int k = 0; k < ar; k++)
      if (d[k].write(src[k] + i0, size_t(len), __func__)) return -1;
    kMathLaunch[size_t(fn)](d[0], d[1], d[2], 0u, 0, 0u, 0u, (long long)len, d[3]);
    if (hip_launch_check(__func__) || d[3].download(got + i0 * w, size_t(len) * w, __func__)) return -1;
  }
  return 0;
}

int pine_gpu_test_math_sweep(int device, int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count, uint32_t stride,
                             int64_t* stats, uint32_t* examples, int cap) {
  if (device < 0) return math_check::sweep_host(fn, fixed_bits, swept_arg, first, count, stride, stats, examples, cap);
  if (math_check::bad_sweep_args(fn, swept_arg, count, stats, examples, cap) || need_device(device)) return -1;
  const int w = math_width(fn);
  const int64_t m = std::max<int64_t>(1, std::min<int64_t>(int64_t(count), math_check::kChunk));
  PinnedOwner<uint32_t> h;  // one chunk's results, pinned for the copies
  DeviceBuffer<uint32_t> d;
  if (alloc_pinned(h, size_t(m) * w, hipHostMallocDefault, __func__) || d.alloc(size_t(m) * w, __func__)) return -1;
  const char* const me = __func__;
  const math_check::ChunkEval on_device = [&](uint32_t start, int64_t len, uint32_t* out) {
    kMathLaunch[size_t(fn)](nullptr, nullptr, nullptr, fixed_bits, swept_arg, start, stride, (long long)len, d);
    return hip_launch_check(me) || d.download(out, size_t(len) * w, me) ? -1 : 0;
  };
  return math_check::sweep(fn, fixed_bits, swept_arg, first, count, stride, on_device, h.get(), stats, examples, cap);
}

int pine_gpu_test_sampler(int device, int spp_req, float* out, int64_t capacity) {
  if (need_device(device)) return -1;
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  const std::vector<uint8_t>& g_tables = *tables_blob;
  const int spp = effective_spp(spp_req);
  const int64_t need = int64_t(6) * spp * (260 + 270);
  if (capacity < need) {
    set_error("capacity too small");
    return -1;
  }
  int k = 0;
  while ((1 << k) < spp) k++;
  DeviceBuffer<uint8_t> dt;
  DeviceBuffer<float> dout;
  if (dt.alloc(65536 + 262144, __func__) || dt.write(transposed_sobol(g_tables).data(), 65536, __func__) || dout.alloc(size_t(need), __func__)) return -1;
  if (const hipError_t e = hipMemcpy(dt + 65536, g_tables.data() + 65536 + size_t(k) * 262144, 262144, hipMemcpyHostToDevice)) return hip_error(__func__, e);
  DTables T{dt, dt + 65536, dt + 65536 + 131072, nullptr, nullptr, 0};
  hipLaunchKernelGGL(test_sampler_kernel, dim3(6), dim3(64), 0, 0, T, spp, dout.get());
  return hip_launch_check(__func__) || dout.download(out, size_t(need), __func__) ? -1 : 0;
}
int64_t pine_gpu_test_sampler_draws(int device, int kind, int spp, int w, int h, int mode, const int32_t* cases, int64_t n, float* out,
                                    int64_t capacity) {
  const auto refuse = [](const char* why) {
    set_error(std::string("pine_gpu_test_sampler_draws: ") + why);
    return int64_t(-1);
  };
  if (!cases || !out || n < 0 || n > kDrawMaxCases || kind < 0 || kind > 2 || (mode != 0 && mode != 1)) return refuse("bad argument");
  if (spp <= 0) return refuse("samples per pixel must be positive");
  if (spp > kMaxDeviceSpp) return refuse("at most 4096 samples per pixel");
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return refuse("a film side is 1 .. 65535 pixels");
  if (device < 0 && mode != 0) return refuse("the LDS form runs on the device only");
  const int sampler_spp = kind == 0 ? effective_spp(spp) : spp;  // (as check_params hands it to a plan)
  std::vector<long long> offsets(size_t(n) + 1, 0);
  for (int64_t i = 0; i < n; i++) {
    const int32_t* q = cases + i * kDrawCaseInts;
    if (q[0] != kind || q[1] != spp || q[2] != w || q[3] != h) return refuse("a case names another sampler or film than the call");
    if (q[4] < 0 || q[4] >= w || q[5] < 0 || q[5] >= h) return refuse("a case's pixel lies outside the film");
    if (q[6] < 0 || q[6] >= sampler_spp) return refuse("a case's sample index lies outside the pixel's samples");
    if (q[7] < 0 || q[7] > 2 || q[8] < 0 || q[8] > kDrawMaxCalls) return refuse("a case's pattern is 0, 1 or 2, its calls at most 65536");
    int floats = 0;
    for (int c = 0; c < q[8]; c++) floats += draw_is_get1d(q[7], c) ? 1 : 2;
    offsets[size_t(i) + 1] = offsets[size_t(i)] + floats;
  }
  const long long total = offsets[size_t(n)];
  if (capacity < total) return refuse("capacity too small");
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  DTables T{};
  DeviceBuffer<uint8_t> d_tables, d_halton;
  if (device < 0) {
    std::vector<uint8_t> host_tables;
    if (fill_sampler_tables(*tables_blob, kind, sampler_spp, w, h, T, d_tables, d_halton, &host_tables)) return -1;
    for (int64_t i = 0; i < n; i++) {
      if (kind == 0) test_draws_case<0>(T, cases + i * kDrawCaseInts, out + offsets[size_t(i)]);
      else test_draws_case<kSmSobol>(T, cases + i * kDrawCaseInts, out + offsets[size_t(i)]);
    }
    return total;
  }
  if (need_device(device)) return -1;
  if (n == 0) return 0;
  DeviceBuffer<int32_t> dc;
  DeviceBuffer<long long> doff;
  DeviceBuffer<float> dout;
  if (fill_sampler_tables(*tables_blob, kind, sampler_spp, w, h, T, d_tables, d_halton) || dc.upload(cases, size_t(n) * kDrawCaseInts, __func__) ||
      doff.upload(offsets.data(), size_t(n), __func__) || dout.alloc(size_t(std::max(total, 1ll)), __func__))
    return -1;
  const dim3 block(mode ? kLdsLaneStride : 64), grid(unsigned((n + block.x - 1) / block.x));
  const int m = (mode ? kSmLds : 0) | (kind ? kSmSobol : 0);
  if (m == 0) hipLaunchKernelGGL(test_draws_kernel<0>, grid, block, 0, 0, T, dc.get(), doff.get(), int(n), dout.get());
  else if (m == kSmLds) hipLaunchKernelGGL(test_draws_kernel<kSmLds>, grid, block, 0, 0, T, dc.get(), doff.get(), int(n), dout.get());
  else if (m == kSmSobol) hipLaunchKernelGGL(test_draws_kernel<kSmSobol>, grid, block, 0, 0, T, dc.get(), doff.get(), int(n), dout.get());
  else hipLaunchKernelGGL(test_draws_kernel<(kSmLds | kSmSobol)>, grid, block, 0, 0, T, dc.get(), doff.get(), int(n), dout.get());
  return hip_launch_check(__func__) || dout.download(out, size_t(total), __func__) ? -1 : total;
}
int pine_gpu_test_rng(int device, uint64_t* out, int64_t capacity) {
  if (need_device(device)) return -1;
  if (capacity < 6 * 19) {
    set_error("capacity too small");
    return -1;
  }
  DeviceBuffer<unsigned long long> d;
  if (d.alloc(6 * 19, __func__)) return -1;
  hipLaunchKernelGGL(test_rng_kernel, dim3(1), dim3(64), 0, 0, d.get());
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the stream is read back in place");
  return hip_launch_check(__func__) || d.download(reinterpret_cast<unsigned long long*>(out), 6 * 19, __func__) ? -1 : 0;
}
int pine_gpu_test_traverse(pine_gpu_scene* scene, int device, const float* rays, int64_t nrays, int flat, int cap, uint32_t* out) {
  if (!scene || !rays || !out || cap < 2 || nrays < 0) {
    set_error("bad argument");
    return -1;
  }
  if (need_device(device)) return -1;
  // the scene as the kernels see it: a plan's device records (nothing is rendered)
  pine_gpu_render_params prm{};
  prm.spp = 1, prm.max_path_length = 2, prm.device = device, prm.shard_rank = 0, prm.shard_world = 1;
  prm.flags = PINE_GPU_FLAG_NO_SPECIALIZE | (flat == 2 ? PINE_GPU_FLAG_ORDER_EMBREE : 0);
  const PlanOwner p(pine_gpu_plan_create(scene, &prm));
  if (!p) return -1;
  if (flat == 1 && p->S.stack_total > 0 && scene_host(scene).accel.nodes.size() > 65535) {
    set_error("the flat traversal keeps 16-bit node ids");
    return -1;
  }
  const size_t words = size_t(nrays) * (2 * size_t(cap) + 5);
  DeviceBuffer<float> dr;
  DeviceBuffer<unsigned> dout;
  if (dr.upload(rays, size_t(nrays) * 8, __func__) || dout.alloc(std::max<size_t>(words, 1), __func__)) return -1;
  if (const hipError_t e = hipMemset(dout, 0, std::max<size_t>(words, 1) * 4)) return hip_error(__func__, e);
  const size_t lds = size_t(std::max(1, p->S.stack_total)) * 64 * (flat == 1 ? sizeof(unsigned short) : sizeof(int));
  if (nrays > 0) {
    if (flat == 1) hipLaunchKernelGGL(test_traverse_kernel<1>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr.get(), (long long)nrays, cap, dout.get());
    else if (flat == 2) hipLaunchKernelGGL(test_traverse_kernel<2>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr.get(), (long long)nrays, cap, dout.get());
    else hipLaunchKernelGGL(test_traverse_kernel<0>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr.get(), (long long)nrays, cap, dout.get());
  }
  return hip_launch_check(__func__) || dout.download(out, words, __func__) ? -1 : 0;
}

int pine_gpu_test_shapes(pine_gpu_scene* scene, int device, const float* rays, int64_t nrays, float* out,
                         int64_t capacity) {
  if (!scene || !rays || !out) {
    set_error("null argument");
    return -1;
  }
  if (need_device(device)) return -1;
  SceneHost& H = scene_host(scene);
  std::vector<DShape> shapes;
  for (auto& g : H.geometries)
    if (g.shape.kind != SHAPE_MESH) shapes.push_back(g.shape);
  const int64_t need = int64_t(shapes.size()) * nrays * 11;
  if (capacity < need) {
    set_error("capacity too small");
    return -1;
  }
  DeviceBuffer<DShape> ds;
  DeviceBuffer<float> dr, dout;
  if (ds.upload(shapes, __func__) || dr.upload(rays, size_t(nrays) * 8, __func__) || dout.alloc(size_t(std::max<int64_t>(need, 1)), __func__)) return -1;
  const long long total = (long long)shapes.size() * nrays;
  if (total > 0)
    hipLaunchKernelGGL(test_shapes_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, 0, ds.get(), int(shapes.size()), dr.get(), (long long)nrays, dout.get());
  return hip_launch_check(__func__) || dout.download(out, size_t(need), __func__) ? -1 : 0;
}

// pine_gpu_test_box_slabs: the host build of box_slabs and of box_slabs_lean (pine_device.h) on caller-given boxes and rays
int pine_gpu_test_box_slabs(const float* boxes, const float* rays, int64_t n, uint32_t* out) {
  if (!boxes || !rays || !out || n < 0) {
    set_error("pine_gpu_test_box_slabs: bad argument");
    return -1;
  }
  for (int64_t i = 0; i < n; i++) {
    const float *b = boxes + i * 6, *q = rays + i * 8;
    const f3 lo = ld3(b), hi = ld3(b + 3), o = ld3(q), d = ld3(q + 3);
    for (int lean = 0; lean < 2; lean++) {
      float tmin = q[6], tmax = q[7];
      const bool hit = lean ? box_slabs_lean(lo, hi, o, d, tmin, tmax) : box_slabs(lo, hi, o, d, tmin, tmax);
      uint32_t* r = out + i * 6 + lean * 3;
      r[0] = hit ? 1u : 0u;
      memcpy(r + 1, &tmin, 4);
      memcpy(r + 2, &tmax, 4);
    }
  }
  return 0;
}

// pine_gpu_test_short_div: the baked traversal's short division (kind 0: the window test, pdiv_short over prcp_core, plain
// division outside the window) and short normalisation (kind 1: local_direction_lean -- the direction and the reciprocals of
// its components) beside the compiler's n / d and normalize() + prcp(), compared bit by bit on the device.
__device__ __forceinline__ uint32_t short_div_word(uint64_t& x, uint32_t elo, uint32_t ehi) {  // splitmix64; a float's bits with a biased exponent in [elo, ehi]
  x += 0x9e3779b97f4a7c15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  const uint32_t w = uint32_t(z), e = elo + uint32_t((uint64_t(uint32_t(z >> 32)) * (ehi - elo + 1)) >> 32);
  return (w & 0x807fffffu) | (e << 23);
}
__device__ __forceinline__ bool bits_within(uint32_t u, float lo, float hi) {  // |value| in [lo, hi], asked of the bits
  u &= 0x7fffffffu;
  return u >= __float_as_uint(lo) && u <= __float_as_uint(hi);
}
__global__ void __launch_bounds__(256) test_short_div_kernel(const uint32_t* in, int kind, int gen, uint32_t p0, uint32_t p1, uint32_t p2, long long n,
                                                             unsigned long long* stats, uint32_t* ex, int cap) {
  unsigned long long taken = 0, outside = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
    uint32_t u[3] = {0, 0, 0};
    const int arity = kind == 0 ? 2 : 3;
    if (gen == 0) {
      for (int k = 0; k < arity; k++) u[k] = in[i * arity + k];
    } else if (gen == 1) {  // numerator p1 over the denominators p0 + i
      u[0] = p1, u[1] = p0 + uint32_t(i);
    } else {
      uint64_t x = (uint64_t(p0) << 32) ^ (uint64_t(i) * 3u);
      for (int k = 0; k < arity; k++) u[k] = short_div_word(x, p1, p2);
    }
    uint32_t want[6], got[6];
    int words;
    bool took, inside;
    if (kind == 0) {
      const float num = __uint_as_float(u[0]), den = __uint_as_float(u[1]);
      took = div_ordinary(num) && div_ordinary(den);
      float q = pdiv_short(num, den, prcp_core(den));
      if (!took) q = num / den;
      want[0] = __float_as_uint(num / den), got[0] = __float_as_uint(q), words = 1;
      inside = bits_within(u[0], kDivLo, kDivHi) && bits_within(u[1], kDivLo, kDivHi);
    } else {
      const f3 v = f3{__uint_as_float(u[0]), __uint_as_float(u[1]), __uint_as_float(u[2])};
      f3 d, inv;
      took = local_direction_lean(v, d, inv);
      const f3 wd = normalize(v), winv = f3{prcp(wd.x), prcp(wd.y), prcp(wd.z)};
      const float w6[6] = {wd.x, wd.y, wd.z, winv.x, winv.y, winv.z}, g6[6] = {d.x, d.y, d.z, inv.x, inv.y, inv.z};
      for (int k = 0; k < 6; k++) want[k] = __float_as_uint(w6[k]), got[k] = __float_as_uint(g6[k]);
      words = 6;
      inside = bits_within(u[0], kRayLo, kRayHi) && bits_within(u[1], kRayLo, kRayHi) && bits_within(u[2], kRayLo, kRayHi);
    }
    taken += took ? 1 : 0;
    outside += took && !inside ? 1 : 0;
    int bad = -1;
    for (int k = words - 1; k >= 0; k--)
      if (want[k] != got[k]) bad = k;
    if (bad >= 0) {
      const unsigned long long slot = atomicAdd(&stats[1], 1ull);
      if (slot < (unsigned long long)cap) {
        uint32_t* e = ex + slot * 8;
        e[0] = u[0], e[1] = u[1], e[2] = u[2], e[3] = uint32_t(bad), e[4] = want[bad], e[5] = got[bad], e[6] = took ? 1u : 0u, e[7] = 0u;
      }
    }
  }
  if (taken) atomicAdd(&stats[2], taken);
  if (outside) atomicAdd(&stats[3], outside);
}
int pine_gpu_test_short_div(int device, int kind, int gen, const uint32_t* in, uint32_t p0, uint32_t p1, uint32_t p2, int64_t n, int64_t* stats,
                            uint32_t* examples, int cap) {
  if (kind < 0 || kind > 1 || gen < 0 || gen > 2 || (gen == 0) != (in != nullptr) || n < 0 || !stats || cap < 0 || (cap > 0 && !examples) ||
      (gen == 1 && (kind != 0 || uint64_t(p0) + uint64_t(n) > 0x100000000ull)) || (gen == 2 && (p1 > p2 || p2 > 255u))) {
    set_error("pine_gpu_test_short_div: bad argument");
    return -1;
  }
  if (need_device(device)) return -1;
  const size_t arity = kind == 0 ? 2 : 3;
  DeviceBuffer<uint32_t> din, dex;
  DeviceBuffer<unsigned long long> dstats;
  if ((in && din.upload(in, size_t(n) * arity, __func__)) || dex.alloc(std::max<size_t>(size_t(cap) * 8, 1), __func__) || dstats.alloc(4, __func__)) return -1;
  if (const hipError_t e = hipMemset(dstats, 0, 4 * sizeof(unsigned long long))) return hip_error(__func__, e);
  if (const hipError_t e = hipMemset(dex, 0, std::max<size_t>(size_t(cap) * 8, 1) * 4)) return hip_error(__func__, e);
  if (n > 0) {
    const unsigned blocks = unsigned(std::min<int64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(test_short_div_kernel, dim3(blocks), dim3(256), 0, 0, in ? din.get() : nullptr, kind, gen, p0, p1, p2, (long long)n, dstats.get(), dex.get(), cap);
  }
  unsigned long long h[4] = {};
  if (hip_launch_check(__func__) || dstats.download(h, 4, __func__) || (cap > 0 && dex.download(examples, size_t(cap) * 8, __func__))) return -1;
  stats[0] = n;
  for (int k = 1; k < 4; k++) stats[k] = int64_t(h[k]);
  return 0;
}

// pine_gpu_test_frame_table: the table as plan creation builds it (device < 0: here, on the host) or as a plan's kernels read it
// (device >= 0: copied back from the plan's scene blob).  `generic`: per entry what the per-hit code computes at a point of that
// face; `faces`: the face shape_surface_info reports for caller-given rays.
static f3 point_on_face(const DShape& sh, int face) {
  const float* f = sh.f;
  if (sh.kind == SHAPE_RECT) return ld3(f);
  const f3 lo = ld3(f), hi = ld3(f + 3);
  f3 p = (lo + hi) / 2.0f;
  set(p, face >> 1, (face & 1) ? get(lo, face >> 1) : get(hi, face >> 1));
  return sh.kind == SHAPE_OBB ? mul_point(ld34(f + 6), p) : p;
}
int64_t pine_gpu_test_frame_table(pine_gpu_scene* scene, pine_gpu_plan* plan, int device, float* entries, float* generic, int64_t cap_entries,
                                  int32_t* base, int64_t cap_shapes, const float* rays, int64_t nrays, int32_t* faces) {
  if (!scene || (device >= 0) != (plan != nullptr) || (faces && !rays) || nrays < 0) {
    set_error("pine_gpu_test_frame_table: bad argument (device >= 0 reads a plan's table, device < 0 builds the scene's)");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  std::vector<DShape> shapes;
  for (auto& g : H.geometries) shapes.push_back(g.shape);
  std::vector<float> table;
  std::vector<int> first;
  if (plan) {
    const DeviceScene& S = plan->S;
    if (size_t(S.num_shapes) != shapes.size()) {
      set_error("pine_gpu_test_frame_table: the plan is not one of this scene");
      return -1;
    }
    first.assign(shapes.size(), -1);
    if (S.off_frames != 0) {
      HIP_OK(hipSetDevice(plan->device));
      table.resize(size_t(S.off_frame_base - S.off_frames) / sizeof(float));
      HIP_OK(hipMemcpy(table.data(), plan->d_blob + S.off_frames, table.size() * sizeof(float), hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(first.data(), plan->d_blob + S.off_frame_base, first.size() * sizeof(int), hipMemcpyDeviceToHost));
      int n = 0;
      for (const DShape& sh : shapes) n += frame_faces(sh.kind);
      table.resize(size_t(n) * kFrameFloats);  // (without the section's padding)
    }
  } else build_frame_table(shapes, table, first);
  const int64_t n = int64_t(table.size() / kFrameFloats);
  if (n > cap_entries || int64_t(shapes.size()) > cap_shapes || !entries || !base) {
    set_error("pine_gpu_test_frame_table: capacity too small");
    return -1;
  }
  memcpy(entries, table.data(), table.size() * sizeof(float));
  for (size_t g = 0; g < shapes.size(); g++) base[g] = first[g];
  if (generic)
    for (size_t g = 0; g < shapes.size(); g++) {
      if (first[g] < 0) continue;
      for (int face = 0; face < frame_faces(shapes[g].kind); face++) {
        DSurface it;
        it.p = it.n = mk3(0.0f);
        it.uv = f2{0, 0};
        if (shape_surface_info(&shapes[g], point_on_face(shapes[g], face), it) != face) {
          set_error("pine_gpu_test_frame_table: a point of a face is not reported on that face");
          return -1;
        }
        const m3 m = coordinate_system(it.n);
        float* e = generic + (size_t(first[g]) + size_t(face)) * kFrameFloats;
        e[0] = it.n.x, e[1] = it.n.y, e[2] = it.n.z, e[3] = 0.0f;
        e[4] = m.x.x, e[5] = m.x.y, e[6] = m.x.z, e[7] = 0.0f;
        e[8] = m.y.x, e[9] = m.y.y, e[10] = m.y.z, e[11] = 0.0f;
      }
    }
  if (faces) {  // (the records' order of pine_gpu_test_shapes: every shape that is no mesh, every ray)
    int32_t* o = faces;
    for (const DShape& sh : shapes) {
      if (sh.kind == SHAPE_MESH) continue;
      for (int64_t r = 0; r < nrays; r++) {
        const float* q = rays + r * 8;
        DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};
        DSurface it;
        *o++ = shape_intersect(&sh, ray) ? shape_surface_info(&sh, ray_at(ray, ray.tmax), it) : -1;
      }
    }
  }
  return n;
}

int pine_gpu_test_bxdf(int device, const float* cases, int64_t n, float* out) {
  if (!cases || !out || n < 0 || n > (1 << 24)) {
    set_error("bad argument");
    return -1;
  }
  // the cases of each narrow mask, found here: a lobe its mask excludes never reaches a kernel built without it
  std::vector<int> idx[3];  // 0: no optional lobe, 1: F_UBER, 2: F_SSS
  for (int64_t i = 0; i < n; i++) {
    const float lobe = cases[i * 16];
    if (!(lobe >= 0 && lobe <= 5 && lobe == float(int(lobe)))) {
      set_error("pine_gpu_test_bxdf: unknown lobe");
      return -1;
    }
    const unsigned m = kBxdfNarrow[int(lobe)];
    idx[m == 0 ? 0 : m == F_UBER ? 1 : 2].push_back(int(i));
  }
  float* const narrow = out + n * 14;
  if (device < 0) {
    for (int64_t i = 0; i < n; i++) test_bxdf_case<F_ALL>(cases + i * 16, out + i * 14);
    for (int i : idx[0]) test_bxdf_case<0u>(cases + size_t(i) * 16, narrow + size_t(i) * 14);
    for (int i : idx[1]) test_bxdf_case<F_UBER>(cases + size_t(i) * 16, narrow + size_t(i) * 14);
    for (int i : idx[2]) test_bxdf_case<F_SSS>(cases + size_t(i) * 16, narrow + size_t(i) * 14);
    return 0;
  }
  if (n == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<float> dc, dout;
  DeviceBuffer<int> didx;
  std::vector<int> order;  // the three groups one after the other
  for (const std::vector<int>& g : idx) order.insert(order.end(), g.begin(), g.end());
  if (dc.upload(cases, size_t(n) * 16, __func__) || dout.alloc(size_t(n) * 2 * 14, __func__) || didx.upload(order, __func__)) return -1;
  if (const hipError_t e = hipMemset(dout, 0, size_t(n) * 2 * 56)) return hip_error(__func__, e);
  const auto blocks = [](size_t m) { return dim3(unsigned((m + 63) / 64)); };
  hipLaunchKernelGGL(test_bxdf_kernel<F_ALL>, blocks(size_t(n)), dim3(64), 0, 0, dc.get(), (const int*)nullptr, (long long)n, dout.get());
  float* const dnarrow = dout + n * 14;
  const int* di = didx;
  if (!idx[0].empty()) hipLaunchKernelGGL(test_bxdf_kernel<0u>, blocks(idx[0].size()), dim3(64), 0, 0, dc.get(), di, (long long)idx[0].size(), dnarrow);
  di += idx[0].size();
  if (!idx[1].empty()) hipLaunchKernelGGL(test_bxdf_kernel<F_UBER>, blocks(idx[1].size()), dim3(64), 0, 0, dc.get(), di, (long long)idx[1].size(), dnarrow);
  di += idx[1].size();
  if (!idx[2].empty()) hipLaunchKernelGGL(test_bxdf_kernel<F_SSS>, blocks(idx[2].size()), dim3(64), 0, 0, dc.get(), di, (long long)idx[2].size(), dnarrow);
  return hip_launch_check(__func__) || dout.download(out, size_t(n) * 2 * 14, __func__) ? -1 : 0;
}

int pine_gpu_test_light_samples(pine_gpu_scene* scene, int device, const float* queries, int64_t n, float* out) {
  if (!scene || !queries || !out || n < 0 || n > (1 << 20)) {
    set_error("bad argument");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  if (!H.accel.built) H.build_accel();  // (a mesh's first triangle and triangle count are written into its record there)
  std::vector<DShape> shapes;
  for (auto& g : H.geometries) shapes.push_back(g.shape);
  std::vector<DLight> lights;
  for (auto& l : H.lights)
    if (l.kind != LIGHT_AREA) lights.push_back(l);
  if (H.has_env) lights.push_back(H.env);
  const int ns = int(shapes.size()), nl = int(lights.size());
  const size_t words = size_t(n) * (size_t(ns) * 13 + size_t(nl) * 9);
  if (device < 0) {
    float* o = out;
    for (int k = 0; k < ns; k++)
      for (int64_t i = 0; i < n; i++, o += 13) test_shape_sample_case(&shapes[size_t(k)], H.accel.tri_verts.data(), queries + i * 6, o);
    for (int k = 0; k < nl; k++)
      for (int64_t i = 0; i < n; i++, o += 9) test_light_sample_case(&lights[size_t(k)], queries + i * 6, o);
    return 0;
  }
  if (words == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<DShape> ds;
  DeviceBuffer<DLight> dl;
  DeviceBuffer<float> dt, dq, dout;
  if (ds.upload(shapes, __func__) || dl.upload(lights, __func__) || dt.upload(H.accel.tri_verts, __func__) || dq.upload(queries, size_t(n) * 6, __func__) ||
      dout.alloc(words, __func__))
    return -1;
  const long long total = (long long)n * (ns + nl);
  hipLaunchKernelGGL(test_light_samples_kernel, dim3(unsigned((total + 63) / 64)), dim3(64), 0, 0, ds.get(), ns, dt.get(), dl.get(), nl, dq.get(), (long long)n, dout.get());
  return hip_launch_check(__func__) || dout.download(out, words, __func__) ? -1 : 0;
}

// pine_gpu_test_env_light and pine_gpu_test_env_light_sample: per query of 5 floats a record of `rec` floats, from `host_case`
// (device < 0) or from `kernel`
static int env_light_hook(const char* me, pine_gpu_scene* scene, int device, const float* queries, int64_t n, float* out, int rec,
                          void (*host_case)(const DLight*, const float*, const float*, float*), void (*kernel)(DLight, const float*, const float*, long long, float*)) {
  if (!scene || !queries || !out || n < 0 || n > (1 << 20)) {
    set_error("bad argument");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  if (!H.has_env || (H.env.kind != LIGHT_IMAGE_SKY && H.env.kind != LIGHT_ATMOSPHERE) || !env_image_valid(H.env, H.env_words)) {
    set_error(std::string(me) + ": the scene's environment light is no ImageSky and no Atmosphere");
    return -1;
  }
  if (device < 0) {
    for (int64_t i = 0; i < n; i++) host_case(&H.env, H.env_words.data(), queries + i * 5, out + i * rec);
    return 0;
  }
  if (n == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<float> de, dq, dout;
  if (de.upload(H.env_words, me) || dq.upload(queries, size_t(n) * 5, me) || dout.alloc(size_t(n) * rec, me)) return -1;
  hipLaunchKernelGGL(kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, 0, H.env, de.get(), dq.get(), (long long)n, dout.get());
  return hip_launch_check(me) || dout.download(out, size_t(n) * rec, me) ? -1 : 0;
}
int pine_gpu_test_env_light(pine_gpu_scene* scene, int device, const float* queries, int64_t n, float* out) {
  return env_light_hook(__func__, scene, device, queries, n, out, 13, test_env_light_case, test_env_light_kernel);
}
int pine_gpu_test_env_light_sample(pine_gpu_scene* scene, int device, const float* queries, int64_t n, float* out) {
  return env_light_hook(__func__, scene, device, queries, n, out, 9, test_env_light_sample_case, test_env_light_sample_kernel);
}

int pine_gpu_test_atmosphere_color(int device, const float* queries, int64_t n, float* out) {
  if (!queries || !out || n < 0 || n > (1 << 20)) {
    set_error("bad argument");
    return -1;
  }
  if (device < 0) {
    for (int64_t i = 0; i < n; i++) test_atmosphere_color_case(queries + i * 7, out + i * 3);
    return 0;
  }
  if (n == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<float> dq, dout;
  if (dq.upload(queries, size_t(n) * 7, __func__) || dout.alloc(size_t(n) * 3, __func__)) return -1;
  hipLaunchKernelGGL(test_atmosphere_color_kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, 0, dq.get(), (long long)n, dout.get());
  return hip_launch_check(__func__) || dout.download(out, size_t(n) * 3, __func__) ? -1 : 0;
}

int64_t pine_gpu_test_env_table(pine_gpu_scene* scene, float* out, int64_t capacity) {
  if (!scene) {
    set_error("null argument");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  if (!H.has_env || H.env.kind != LIGHT_ATMOSPHERE || !env_image_valid(H.env, H.env_words)) {
    set_error("pine_gpu_test_env_table: the scene's environment light is no Atmosphere");
    return -1;
  }
  const int w = H.env.pad[1], h = H.env.pad[2];
  const int64_t n = int64_t(w) * h, grid = int64_t(w + 1) * (h + 1), floats = n + grid * 3;
  if (!out || capacity < floats) return floats;
  // The scene keeps the colours (they are part of the light's buffer) and not the densities, which only the tree build read:
  // they are computed again here, where the light's own were (H.env_table_device), and the colours that come with them must be
  // the ones the light holds.
  std::vector<float> colors(size_t(grid) * 3), density(static_cast<size_t>(n));
  if (atmosphere_tables(H.env_table_device, H.env.direction, w, h, colors.data(), density.data()) < 0) return -1;
  const float* held = H.env_words.data() + (H.env_words.size() - size_t(grid) * 3);
  if (memcmp(colors.data(), held, size_t(grid) * 12) != 0) {
    set_error("pine_gpu_test_env_table: the tables computed again differ from the light's");
    return -1;
  }
  memcpy(out, density.data(), size_t(n) * 4);
  memcpy(out + n, held, size_t(grid) * 12);
  return floats;
}

int64_t pine_gpu_test_env_tree(pine_gpu_scene* scene, int32_t* out, int64_t capacity_words) {
  if (!scene) {
    set_error("null argument");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  if (!H.has_env || (H.env.kind != LIGHT_IMAGE_SKY && H.env.kind != LIGHT_ATMOSPHERE) || !env_image_valid(H.env, H.env_words)) {
    set_error("pine_gpu_test_env_tree: the scene's environment light is no ImageSky and no Atmosphere");
    return -1;
  }
  const int64_t words = int64_t(H.env.geom) * 7;
  if (!out || capacity_words < words) return words;
  const int32_t* base = reinterpret_cast<const int32_t*>(H.env_words.data()) + kEnvHeaderWords;
  std::vector<int> todo{0};  // pre-order: a node, its left subtree, its right subtree
  int32_t* o = out;
  while (!todo.empty()) {
    const int k = todo.back();
    todo.pop_back();
    const int32_t* nd = base + int64_t(k) * kEnvNodeWords;
    *o++ = nd[0];
    *o++ = (nd[3] & kEnvSplitX) ? 1 : 0;
    *o++ = nd[4], *o++ = nd[5], *o++ = nd[6], *o++ = nd[7];
    *o++ = (nd[3] & kEnvLeaf) ? 1 : 0;
    if (!(nd[3] & kEnvLeaf)) todo.push_back(nd[2] + 1), todo.push_back(nd[2]);
  }
  return words;
}

int64_t pine_gpu_test_node_programs(pine_gpu_scene* scene, int32_t* out, int64_t capacity_words) {
  if (!scene) {
    set_error("null argument");
    return -1;
  }
  std::vector<DMaterial> mats;
  std::vector<DNodeOp> ops;
  std::vector<float> tex;
  if (!scene_host(scene).compile_node_programs(mats, ops, tex) || !tex_ops_valid(ops, tex.size())) return -1;
  const int64_t words = 2 + 4 * int64_t(mats.size()) + 4 * int64_t(ops.size());
  if (out && capacity_words >= words) {
    int32_t* o = out;
    *o++ = int32_t(mats.size());
    *o++ = int32_t(ops.size());
    for (const DMaterial& m : mats)
      for (int k = 0; k < 4; k++) *o++ = m.prog[k];
    if (!ops.empty()) memcpy(o, ops.data(), ops.size() * sizeof(DNodeOp));
  }
  return words;
}

int64_t pine_gpu_test_tex_words(pine_gpu_scene* scene) {
  if (!scene) {
    set_error("null argument");
    return -1;
  }
  std::vector<DMaterial> mats;
  std::vector<DNodeOp> ops;
  std::vector<float> tex;
  if (!scene_host(scene).compile_node_programs(mats, ops, tex) || !tex_ops_valid(ops, tex.size())) return -1;
  return int64_t(tex.size());
}

int pine_gpu_test_material_params(pine_gpu_scene* scene, int device, const float* queries, int64_t n, float* out) {
  if (!scene || !queries || !out || n < 0 || n > (1 << 20)) {
    set_error("bad argument");
    return -1;
  }
  std::vector<DMaterial> mats;
  std::vector<DNodeOp> ops;
  std::vector<float> tex;
  if (!scene_host(scene).compile_node_programs(mats, ops, tex) || !tex_ops_valid(ops, tex.size())) return -1;
  const int nm = int(mats.size());
  if (device < 0) {
    for (int k = 0; k < nm; k++)
      for (int64_t i = 0; i < n; i++) test_material_params_case(&mats[size_t(k)], ops.data(), tex.data(), queries + i * 8, out + (k * n + i) * 10);
    return 0;
  }
  if (n == 0 || nm == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<DMaterial> dm;
  DeviceBuffer<DNodeOp> dops;
  DeviceBuffer<float> dq, dout, dtex;
  const size_t words = size_t(n) * size_t(nm) * 10;
  if (dm.upload(mats, __func__) || dops.upload(ops, __func__) || dtex.upload(tex, __func__) || dq.upload(queries, size_t(n) * 8, __func__) || dout.alloc(words, __func__)) return -1;
  const long long total = (long long)n * nm;
  hipLaunchKernelGGL(test_material_params_kernel, dim3(unsigned((total + 63) / 64)), dim3(64), 0, 0, dm.get(), nm, dops.get(), dtex.get(), dq.get(), (long long)n, dout.get());
  return hip_launch_check(__func__) || dout.download(out, words, __func__) ? -1 : 0;
}

int pine_gpu_test_choose_lobe(pine_gpu_scene* scene, int device, const float* cases, int64_t n, float* out) {
  if (!scene || !cases || !out || n < 0 || n > (1 << 20)) {
    set_error("bad argument");
    return -1;
  }
  if (device < 0) {
    set_error("pine_gpu_test_choose_lobe: choose_lobe is device code only");
    return -1;
  }
  std::vector<DMaterial> mats;
  std::vector<DNodeOp> ops;
  std::vector<float> tex;
  if (!scene_host(scene).compile_node_programs(mats, ops, tex) || !tex_ops_valid(ops, tex.size())) return -1;
  for (int64_t i = 0; i < n; i++) {
    const float* c = cases + i * 16;
    const bool whole = c[0] >= 0 && c[0] < float(mats.size()) && c[0] == float(int(c[0]));
    if (!whole || mats[size_t(c[0])].kind == MAT_EMISSIVE) {  // EmissiveMaterial::sample_bxdf is unreachable (material.h:20)
      set_error("pine_gpu_test_choose_lobe: a case names no material that has a lobe");
      return -1;
    }
    if (!(c[13] >= 0 && c[13] < 1024 && c[14] >= 0 && c[14] < 1024 && c[15] >= 0 && c[15] < 64)) {
      set_error("pine_gpu_test_choose_lobe: pixel or sample index out of range");
      return -1;
    }
  }
  if (n == 0) return 0;
  if (need_device(device)) return -1;
  DeviceBuffer<DMaterial> dm;
  DeviceBuffer<DNodeOp> dops;
  DeviceBuffer<float> dc, dout, dtex;
  if (dm.upload(mats, __func__) || dops.upload(ops, __func__) || dtex.upload(tex, __func__) || dc.upload(cases, size_t(n) * 16, __func__) || dout.alloc(size_t(n) * 16, __func__)) return -1;
  hipLaunchKernelGGL(test_choose_lobe_kernel, dim3(unsigned((2 * n + 63) / 64)), dim3(64), 0, 0, dm.get(), dops.get(), dtex.get(), dc.get(), (long long)n, dout.get());
  return hip_launch_check(__func__) || dout.download(out, size_t(n) * 16, __func__) ? -1 : 0;
}

// The handles the owners of pine_device_buffer.h hold right now (device blocks, pinned memory, events, streams: those of live plans
// and of calls in flight) and the blocks the pool keeps for the next plan.  Reads two counters; launches nothing.
int pine_gpu_test_live_device_blocks(int64_t out[2]) {
  if (!out) {
    set_error("null argument");
    return -1;
  }
  out[0] = g_live_handles.load();
  std::lock_guard<std::mutex> lock(DevicePool::get().mu);
  out[1] = int64_t(DevicePool::get().free_blocks.size());
  return 0;
}

// PINE_GPU_TEST_POISON (pine_device_buffer.h): the blocks and bytes this process has poisoned so far, device and pinned ones
// together.  Reads two counters; launches nothing.
int pine_gpu_test_poison_stats(int64_t out[2]) {
  if (!out) {
    set_error("null argument");
    return -1;
  }
  out[0] = g_poisoned_blocks.load(), out[1] = g_poisoned_bytes.load();
  return 0;
}

// One block of `bytes` bytes on `device`, from the pool (from_pool != 0) or from hipMalloc, as DeviceBuffer hands it out: nothing
// is written to it, its first `bytes` bytes are downloaded to out_words ((bytes + 3) / 4 words; the bytes behind `bytes` in the
// last word are left as they were).  Launches nothing.
int pine_gpu_test_poison_probe(int device, int from_pool, int64_t bytes, uint32_t* out_words) {
  if (!out_words || bytes <= 0) {
    set_error("pine_gpu_test_poison_probe: null argument or no bytes");
    return -1;
  }
  if (const hipError_t e = hipSetDevice(device)) return hip_error(__func__, e);
  DeviceBuffer<uint8_t> d(from_pool ? kFromPool : kFromMalloc);
  return d.alloc_bytes(size_t(bytes), __func__) || d.download(reinterpret_cast<uint8_t*>(out_words), size_t(bytes), __func__) ? -1 : 0;
}

}  // extern "C"
