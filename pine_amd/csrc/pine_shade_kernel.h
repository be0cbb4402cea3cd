// pine_amd/csrc/pine_shade_kernel.h -- Shader: ONE vertex of PathIntegrator::radiance() (src/pine/impl/integrator/path.cpp:42-123,
// without the medium lines) for N paths in caller-owned device buffers, batched as Accel's ray queries are (pine_accel_kernel.h).
// With Accel, `begin -> intersect -> vertex -> hit -> intersect -> vertex -> ... -> fold -> resolve` is a complete path tracer
// written by the caller, who sees every ray, hit and vertex record on the way.  Lane = path, 256 threads, 64-bit offsets; no
// atomics, no waits between lanes, no persistent loop, no device state that a query writes.  Every step is the path kernels'
// (pine_radiance.h: camera_sample, terminal_radiance, choose_lobe, sample_direct, clamp_radiance, fold_level; pine_device.h:
// material_params, bxdf_sample, spawn_ray): the same bits.  What the path kernels do inline between those calls is restated in
// shade_vertex_kernel below, in their order.  There is no BSSRDF walk (a Subsurface scene is refused by the host): every kernel
// ends after a bounded amount of work.
//
// The order of draws of one vertex: Uber's lobe choice from the pixel's RNG (0-2 floats, choose_lobe); unless the lobe is a delta
// one, the light sampler's get2d then get1d (sample_direct); the lobe's own draws (bxdf_sample).  A sample starts with four RNG
// floats (camera_sample, lens first).  The RNG is serial over a pixel's samples: it travels in the state, and a caller renders a
// pixel's samples in order.
//
// One ray is Accel's: 8 floats, o[3] d[3] tmin tmax.  The null ray -- written where a record has no shadow or next ray -- is
// o = 0, d = (0, 0, 1), tmin = 0, tmax = -1: finite, answered at once, its answer never read.
//
// The path state: 8 words, two 16-byte loads / stores.
//   0-3   u64 x 2  the pixel's RNG (xoroshiro s0, s1)
//   4     u32      PackedState: sample index (bits 0-11), Vertex::length (21-26), diffuse_length > 0 (27), is_delta (28)
//   5     u32      px | py << 16
//   6     i32      the sampler's dimension counter
//   7     u32      0: the path is live; 1: done (shade_vertex_kernel leaves such a state byte for byte as it was)
//
// The vertex record: 16 words, four 16-byte stores.
//   0     i32  kind: -1 none (the path was done before this level), 0 the ray left the scene, 1 it met an emissive surface, 2 the
//              path-length limit, 3 a shaded vertex -- the kinds of the per-vertex log
//   1     i32  Vertex::length of the vertex
//   2     u32  flags: bit 0 has_shadow_ray, bit 1 has_next_ray, bit 2 the light pdf is there
//   3     f32  kinds 0 and 1: the pdf of having picked the vertex by light sampling; -1: none (the bounce before was a delta one)
//   4-6   f32  kinds 0 and 1: the returned Lo; else 0                     7   f32  cosine
//   8-10  f32  kind 3: the direct term, UNSHADOWED (shade_fold_kernel clears it where the shadow ray was occluded); else 0
//   11    f32  bs.pdf
//   12-14 f32  bs.f                                                       15  f32  bs.is_delta (0 or 1)
// (words 7 and 11-15 are 0 unless has_next_ray.)
//
// The log shade_fold_kernel writes: 16 floats per vertex, the words of pine_gpu_plan_vertex_log --
//   kind | length | direct term after visibility (3) | bs.f (3) | cosine | bs.pdf | is_delta | mis | returned light pdf (-1: none) | returned Lo (3)
#pragma once
#include "pine_accel_kernel.h"

namespace pine_gpu {

constexpr int kShadeStateWords = 8, kShadeRecordWords = 16;
constexpr int kShadeNone = -1, kShadeMiss = 0, kShadeEmissive = 1, kShadeLimit = 2, kShadeShaded = 3;
constexpr unsigned kShadeHasShadowRay = 1u, kShadeHasNextRay = 2u, kShadeHasLightPdf = 4u;

__device__ __forceinline__ void shade_store_ray(float4* __restrict__ rays, long long i, const DRay& r) {
  rays[2 * i] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
  rays[2 * i + 1] = make_float4(r.d.y, r.d.z, r.tmin, r.tmax);
}
__device__ __forceinline__ DRay shade_null_ray() { return DRay{mk3(0.0f), f3{0.0f, 0.0f, 1.0f}, 0.0f, -1.0f}; }

struct ShadeState {
  DRng g;
  PackedState st;
  unsigned pxy;
  int dimension;
  unsigned done;
};
__device__ __forceinline__ ShadeState shade_load_state(const float4* states, long long i) {
  const float4 a = states[2 * i], b = states[2 * i + 1];
  ShadeState s;
  s.g.s0 = uint64_t(__float_as_uint(a.x)) | (uint64_t(__float_as_uint(a.y)) << 32);
  s.g.s1 = uint64_t(__float_as_uint(a.z)) | (uint64_t(__float_as_uint(a.w)) << 32);
  s.st.v = __float_as_uint(b.x);
  s.pxy = __float_as_uint(b.y);
  s.dimension = __float_as_int(b.z);
  s.done = __float_as_uint(b.w);
  return s;
}
__device__ __forceinline__ void shade_store_state(float4* states, long long i, const ShadeState& s) {
  states[2 * i] = make_float4(__uint_as_float(uint32_t(s.g.s0)), __uint_as_float(uint32_t(s.g.s0 >> 32)), __uint_as_float(uint32_t(s.g.s1)),
                              __uint_as_float(uint32_t(s.g.s1 >> 32)));
  states[2 * i + 1] = make_float4(__uint_as_float(s.st.v), __uint_as_float(s.pxy), __int_as_float(s.dimension), __uint_as_float(s.done));
}

// Sample `sample` of every pixel starts (path.cpp:34-36): Sampler::start_pixel's seed for sample 0 -- later samples go on from the
// RNG the state holds --, sampler index `sample`, dimension 0 (HaltonSampler: 2), Vertex::first_vertex(), the camera ray.
// (This kernel, the fold and the resolve read no scene record: templates only so that pine_shade_kernels.hip alone emits them, F = 0.)
template <unsigned F>
__global__ void __launch_bounds__(kBlock) shade_begin_kernel(DCamera cam, int sampler_kind, int sample, float4* states, float4* __restrict__ rays) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)cam.W * cam.H) return;
  const int px = int(i % cam.W), py = int(i / cam.W);
  ShadeState s;
  if (sample == 0) s.g = rng_seed(hash_pixel(px, py, 0));
  else s.g = shade_load_state(states, i).g;
  const DRay r = camera_sample(cam, px, py, s.g);
  s.st.start_sample(sample);
  s.pxy = unsigned(px) | (unsigned(py) << 16);
  s.dimension = sampler_kind == 2 ? 2 : 0;
  s.done = 0u;
  shade_store_state(states, i, s);
  shade_store_ray(rays, i, DRay{r.o, r.d, 0.0f, r.tmax});  // (every ray of a path has tmin == 0)
}

// One radiance() invocation per lane.  rays[i] is the ray that led here, hits[i] Accel's 12-word answer for it.
// LDS (F_LDS_SCENE only): the scene blob.
template <unsigned F>
__global__ void __launch_bounds__(kBlock) shade_vertex_kernel(DeviceScene S, const float4* __restrict__ rays, const float4* __restrict__ hits, long long n,
                                                              float4* states, float4* __restrict__ records, float4* __restrict__ shadow_rays,
                                                              float4* __restrict__ next_rays) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  constexpr int kSM = (F & F_SOBOL) ? kSmSobol : 0;  // (the sampler's tables are read from global memory: a block's lanes are arbitrary pixels)
  const unsigned tid = threadIdx.x;
  SceneView V;
  if constexpr (F & F_LDS_SCENE) V = scene_view_staged(S, reinterpret_cast<uint4*>(lds_raw), tid, kBlock);
  else V = scene_view_global(S);
  __syncthreads();  // (the scene staged above; every lane arrives, the ones past the last path too: nothing returns before this)
  const long long i = (long long)blockIdx.x * kBlock + tid;
  if (i >= n) return;
  const DTables& T = S.tables;
  ShadeState ps = shade_load_state(states, i);

  int kind = kShadeNone, length = 0;
  unsigned flags = 0;
  float light_pdf = -1.0f, cosine = 0.0f, pdf = 0.0f, delta = 0.0f;
  f3 Lo = mk3(0.0f), direct = mk3(0.0f), f = mk3(0.0f);
  DRay shadow_ray = shade_null_ray(), next_ray = shade_null_ray();

  if (ps.done == 0u) {
    const DRay ray = accel_load_ray(rays, i);
    const float4 h0 = hits[3 * i], h1 = hits[3 * i + 1], h2 = hits[3 * i + 2];
    const float tmax = h0.x;
    const int geom = __float_as_int(h0.y);
    const bool hit = geom >= 0 && geom < S.num_shapes;  // (an index from the caller's buffer: nothing outside the scene's records is read)
    DSurface it;
    it.p = f3{h1.x, h1.y, h1.z};
    it.n = f3{h1.w, h2.x, h2.y};
    it.uv = f2{h2.z, h2.w};
    DSampler sampler;
    sampler.px = int(ps.pxy & 0xffffu), sampler.py = int(ps.pxy >> 16);
    sampler.index = ps.st.s_cur();
    sampler.dimension = ps.dimension;
    const int pv_length = ps.st.length();
    length = pv_length;
    bool terminal = false, has_light_pdf = false;
    float lp = 0.0f;
    const DShape* shape = nullptr;
    const DMaterial* mat = nullptr;
    if (!hit) {
      terminal = true;
      kind = kShadeMiss;
      Lo = terminal_radiance<F>(V, S.env_light, S.num_lights, false, shape, it, ray.o, ray.d, tmax, ps.st.is_delta(), has_light_pdf, lp);
    } else {
      shape = &V.shapes[geom];
      mat = &V.materials[shape->material];
      if (mat->kind == MAT_EMISSIVE) {
        Lo = terminal_radiance<F>(V, S.env_light, S.num_lights, true, shape, it, ray.o, ray.d, tmax, ps.st.is_delta(), has_light_pdf, lp);
        terminal = true;
        kind = kShadeEmissive;
      } else if (pv_length + 1 >= S.max_path_length) {  // path.cpp:89
        terminal = true;
        kind = kShadeLimit;
      }
    }
    if (has_light_pdf) {
      flags |= kShadeHasLightPdf;
      light_pdf = lp;
    }
    if (!terminal) {
      kind = kShadeShaded;
      const f3 wi = -ray.d;
      const m3 l2w = surface_frame(V, -1, it.n);  // (the generic per-hit frame: the hit record carries no frame-table entry)
      const m3 w2l = transpose(l2w);
      const MatParams mp = material_params<F>(mat, V.node_ops, V.tex, it.p, it.n, it.uv);
      DBxdf bx;
      auto rng_load = [&]() -> DRng { return ps.g; };
      auto rng_store = [&](const DRng& g) { ps.g = g; };
      choose_lobe<F, kSM>(mat, mp, wi, it.n, ps.st.diffuse_length() > 0, false, rng_load, rng_store, T, sampler, bx);
      bx.wi = mul(w2l, wi);  // material.h:119
      // next-event estimation (path.cpp:98-113): the trace is the caller's -- the ray is recorded, the term kept as if visible
      if (!bxdf_is_delta<F>(bx)) {
        unsigned shadow_count = 0;
        direct = sample_direct<F, kSM>(V, S.num_lights, it, w2l, bx, mp, T, sampler, shadow_count, [&](const DRay& sr) -> bool {
          shadow_ray = sr;
          flags |= kShadeHasShadowRay;
          return false;
        });
      }
      // BSDF sampling + continuation (path.cpp:114-120)
      bx.albedo = mp.albedo;
      bx.albedo_over_pi = mp.albedo_over_pi;
      DBsdfSample bs;
      if (bxdf_sample<F, kSM>(bx, T, sampler, bs)) {
        const f3 wo_world = mul(l2w, bs.wo);
        cosine = absdot(wo_world, it.n);
        f = bs.f;
        pdf = bs.pdf;
        delta = bs.is_delta ? 1.0f : 0.0f;
        next_ray = spawn_ray(it.p, it.n, wo_world, kFloatMax);
        flags |= kShadeHasNextRay;
        ps.st.next_vertex(bs.is_delta);
      } else {
        terminal = true;  // no continuation: the vertex resolves with lo = its direct term (path.cpp:121); the fold clamps it
      }
    }
    ps.dimension = sampler.dimension;
    ps.done = terminal ? 1u : 0u;
    shade_store_state(states, i, ps);
  }
  float4* o = records + 4 * i;
  o[0] = make_float4(__int_as_float(kind), __int_as_float(length), __uint_as_float(flags), light_pdf);
  o[1] = make_float4(Lo.x, Lo.y, Lo.z, cosine);
  o[2] = make_float4(direct.x, direct.y, direct.z, pdf);
  o[3] = make_float4(f.x, f.y, f.z, delta);
  shade_store_ray(shadow_rays, i, shadow_ray);
  shade_store_ray(next_rays, i, next_ray);
}

// The backward fold of one sample of n paths (path.cpp:114-121): records and occlusion bytes are [level][path].  A path ends at
// its first record without a next ray; levels behind it are not read.  A path still live at the last level given (the caller
// stopped early) folds with nothing from below.  sum[i]: xyz the running sum in sample order (sample 0 starts it), w the samples
// summed.  log (or null): [level][path][16], zeros behind the path's end.
template <unsigned F>
__global__ void __launch_bounds__(kBlock) shade_fold_kernel(const float4* __restrict__ records, const unsigned char* __restrict__ occluded, int levels,
                                                                   long long n, int sample, float4* sum, float4* __restrict__ log) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int last = -1;  // the deepest level that holds a vertex of this path
  bool ended = false;
  for (int l = 0; l < levels; l++) {
    const float4 r0 = records[4 * ((long long)l * n + i)];
    if (__float_as_int(r0.x) < 0) break;
    last = l;
    if (!(__float_as_uint(r0.z) & kShadeHasNextRay)) {
      ended = true;
      break;
    }
  }
  f3 Li = mk3(0.0f);
  bool lp_valid = false;
  float lp = 0.0f;
  for (int l = levels - 1; l >= 0; l--) {
    const long long at = (long long)l * n + i;
    float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g1 = g0, g2 = g0, g3 = g0;
    if (l <= last) {
      const float4 *r = records + 4 * at, r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
      const int kind = __float_as_int(r0.x);
      const unsigned flags = __float_as_uint(r0.z);
      f3 nee{r2.x, r2.y, r2.z};
      if ((flags & kShadeHasShadowRay) && occluded[at] != 0) nee = mk3(0.0f);
      g0 = make_float4(float(kind), float(__float_as_int(r0.y)), nee.x, nee.y);
      if (l == last && ended) {
        if (kind == kShadeShaded) {
          Li = clamp_radiance(0, nee);
        } else {
          Li = f3{r1.x, r1.y, r1.z};
          lp_valid = (flags & kShadeHasLightPdf) != 0;
          lp = r0.w;
        }
        g1 = make_float4(nee.z, 0.0f, 0.0f, 0.0f);
        g3 = make_float4(lp_valid ? lp : -1.0f, Li.x, Li.y, Li.z);
      } else {
        const float e[8] = {nee.x, nee.y, nee.z, r3.x, r3.y, r3.z, r1.w / r2.w, r2.w};
        const float mis = fold_level<F>(e, 0ull, l, Li, lp_valid, lp);
        g1 = make_float4(nee.z, r3.x, r3.y, r3.z);
        g2 = make_float4(r1.w, r2.w, r3.w, mis);
        g3 = make_float4(-1.0f, Li.x, Li.y, Li.z);
      }
    }
    if (log) {
      float4* g = log + 4 * at;
      g[0] = g0, g[1] = g1, g[2] = g2, g[3] = g3;
    }
  }
  f3 L = mk3(0.0f);
  if (sample != 0) {
    const float4 a = sum[i];
    L = f3{a.x, a.y, a.z};
  }
  L = L + Li;
  sum[i] = make_float4(L.x, L.y, L.z, float(sample + 1));
}

// film[i] = (sum / spp, 1): the division of the path kernels' resolve (resolve_tile, pine_kernels_device.h).
template <unsigned F>
__global__ void __launch_bounds__(kBlock) shade_resolve_kernel(const float4* __restrict__ sum, long long n, int spp, float4* __restrict__ film) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 a = sum[i];
  const f3 m = f3{a.x, a.y, a.z} / float(spp);
  film[i] = make_float4(m.x, m.y, m.z, 1.0f);
}

// The precompiled variants, first fit: the Cornell box's class -- Diffuse and Emissive on analytic shapes, area lights only, no
// node programs, BlueSampler, the scene in LDS --, then everything a scene may hold except Subsurface.
struct PineShadeVariant {
  unsigned features;
  const void* vertex;
  const char* name;
};
constexpr unsigned kFShadeNarrow = kFAccelAnalytic | F_LDS_SCENE;
constexpr unsigned kFShadeAll = kFAccelShapes | F_UBER | F_NODES | F_LIGHTS | F_SOBOL;
const PineShadeVariant* pine_gpu_shade_variant_table(int* count);  // pine_shade_kernels.hip
const void* pine_gpu_shade_begin_fn();
const void* pine_gpu_shade_fold_fn();
const void* pine_gpu_shade_resolve_fn();

}  // namespace pine_gpu
