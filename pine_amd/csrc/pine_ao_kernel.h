// pine_amd/csrc/pine_ao_kernel.h -- AOIntegrator (src/pine/impl/integrator/ao.h, ao.cpp) on gfx950.
//
// One camera sample is one closest-hit ray and, where it hits, EIGHT independent any-hit rays of length `radius` around
// one random frame -- no materials, no lights, no fold, no recursion.  A sample's value is k / 8, k the rays that met
// nothing, so a pixel's sum is exact in any order and the kernel counts unoccluded rays per pixel as INTEGERS with plain
// atomics; ao_film_kernel turns the counts into the film, (count * 0.125f) / spp.  Every building block is the path
// kernels' (the prologue of pine_radiance.h -- scene view, LDS staging, sampler slices --, camera_sample, pine_traverse.h's scene_traverse
// in pine-BVH order, hit_surface, the samplers, spawn_ray): the same bits.
//
// Two schedules of the same arithmetic (template parameter REGROUP):
//   false  lane = camera sample, a loop over its eight occlusion rays ($PINE_GPU_AO_KERNEL=serial, the default: the faster
//          one on cbox and on 10 000 cones);
//   true   ($PINE_GPU_AO_KERNEL=regroup) phase A as above; then the wave compacts the lanes that hit (ballot + prefix rank) into a per-wave LDS slab
//          of records (p, flipped n, the three columns of the frame, the pixel) and works them off eight at a time:
//          lane l traces direction l & 7 of record l >> 3, a ballot's bytes give each record's k.  64 lanes carry 64
//          any-hit rays whatever the fraction of camera rays that hit.
// The kernel has no wait of any kind (work is handed out by one atomic per wave and 64 items; waves never depend on one
// another), so nothing in it can run out; the bail-out record of Counters is raised by the test hook only.
#pragma once
#include "pine_kernels_device.h"

namespace pine_gpu {

struct AoParams {
  float radius;   // min_value(scene.get_aabb().diagonal()) / 2 (ao.h:12)
  float dir[24];  // directions[8] (ao.cpp:6-9), host libm
  int spp;        // AO samples per pixel: max(sampler.spp() / 8, 1) (ao.cpp:13)
};

// LDS layout (dword offsets): sampler slices [12][256] | Sobol rows 40 x 256 bytes | (REGROUP) record slabs, 16 x 64 per wave |
// traversal stack [stack_total][256] | (F_LDS_SCENE) the scene blob
constexpr int kAoOffTile = 0;
constexpr int kAoOffSobol = kLdsTileDwords * kBlock;
constexpr int kAoOffSlab = kAoOffSobol + kLdsSamplerDims * 256 / 4;
constexpr int kAoSlabDwords = 16 * 64;
constexpr int ao_off_stack(bool regroup) { return kAoOffSlab + (regroup ? (kBlock / 64) * kAoSlabDwords : 0); }

template <unsigned F, bool REGROUP>
__global__ void __launch_bounds__(kBlock) ao_kernel(DeviceScene S, WorkParams W, AoParams A, const ulonglong2* __restrict__ ckpt,
                                                   unsigned* __restrict__ counts, Counters* __restrict__ counters) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  constexpr int kSM = kSmLds | ((F & F_SOBOL) ? kSmSobol : 0);
  constexpr int kOffStack = ao_off_stack(REGROUP);
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  if (W.debug_force_bail) {  // test hook: the launch must FAIL through the bail-out record
    if (tid == 0 && blockIdx.x == 0) {
      counters->bail_code = 7;
      atomicAdd(&counters->bail_count, 1ull);
    }
    return;
  }
  float* const lds_f = reinterpret_cast<float*>(lds_raw);
  uint32_t* const lds_u = reinterpret_cast<uint32_t*>(lds_raw);
  int* const stack = lds_raw + kOffStack + tid;
  stage_sobol_rows(lds_raw + kAoOffSobol, S.tables, tid, kBlock);
  const DTables T = lane_tables(S.tables, lds_raw + kAoOffSobol, lds_u + kAoOffTile, tid);
  SceneView V;
  if constexpr (F & F_LDS_SCENE) V = scene_view_staged(S, reinterpret_cast<uint4*>(lds_raw + kOffStack + S.stack_total * kBlock), tid, kBlock);
  else V = scene_view_global(S);
  __syncthreads();  // Sobol rows (and the scene) staged above
  const int film_w = S.cam.W;
  const int kspi = W.samples_per_item;
  const f3 my_dir = ld3(A.dir + 3 * int(lane & 7u));  // REGROUP: this lane's entry of directions[8]
  (void)my_dir;
  float* const slab = lds_f + kAoOffSlab + int(tid >> 6) * kAoSlabDwords;  // REGROUP: this wave's records, [field][rank]
  (void)slab;
  unsigned long long hits = 0, rays = 0;  // (wave totals, kept by every lane alike)

  while (true) {
    // 64 consecutive items = one 8x8 tile at one sample range: one atomic per wave
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&counters->next_item, 64ull);
    base = __shfl(base, 0);
    if (base >= W.total_items) break;
    if (lane == 0) post_progress(W, base, 6);
    const unsigned long long item = base + lane;
    ItemInfo it{};
    bool valid = item < W.total_items;
    if (valid) {
      it = decode_item(W, S.cam.W, S.cam.H, A.spp, item);
      valid = it.valid;
    }
    DRng g{0, 0};
    if (valid) {
      load_lane_slice(S.tables, it.px, it.py, lds_u + kAoOffTile, tid);
      // radiance() draws nothing from the pixel's RNG: the state at sample s is the seed advanced 4 s steps (checkpoints)
      if (W.items_per_pixel == 1) {
        g = rng_seed(hash_pixel(it.px, it.py, 0));
      } else {
        const ulonglong2 c = ckpt[it.ckpt_index];
        g = DRng{c.x, c.y};
      }
    }
    const unsigned pixel = unsigned(it.py) * unsigned(film_w) + unsigned(it.px);
    for (int j = 0; j < kspi; j++) {
      // ---- phase A, lane = camera sample: closest hit, surface, the sample's one get2d, the frame ----
      bool hit = false;
      f3 p = mk3(0.0f), n = mk3(0.0f);
      m3 tbn{mk3(0.0f), mk3(0.0f), mk3(0.0f)};
      if (valid) {
        DRay r = camera_sample(S.cam, it.px, it.py, g);
        int geom = -1, prim = 0;
        hit = scene_traverse<false, F>(V, r, stack, geom, prim);
        if (hit) {
          DSurface su;
          hit_surface<F>(V, &V.shapes[geom & kPrimIndexMask], prim, r.o, r.d, r.tmax, su);
          p = su.p;
          n = face_same_hemisphere(su.n, -r.d);
          DSampler sampler{it.px, it.py, it.chunk * kspi + j, 0};
          if constexpr (F & F_SOBOL)
            if (S.tables.kind == 2) sampler.dimension = 2;  // HaltonSampler::start_pixel / start_next_sample
          tbn = coordinate_system(uniform_sphere(sampler_get2d<kSM>(T, sampler)));
        }
      }
      const unsigned long long hit_mask = __ballot(hit);
      const int nrec = __popcll(hit_mask);
      hits += unsigned(nrec);
      rays += 8u * unsigned(nrec);
      if constexpr (!REGROUP) {
        if (hit) {
          unsigned k = 0;
          for (int i = 0; i < 8; i++) {
            DRay sr = spawn_ray(p, n, face_same_hemisphere(mul(tbn, ld3(A.dir + 3 * i)), n), A.radius);
            int g2, p2;
            if (!scene_traverse<true, F>(V, sr, stack, g2, p2)) k++;
          }
          if (k) atomicAdd(&counts[pixel], k);
        }
      } else if (nrec > 0) {
        // ---- regroup: the lanes that hit, compacted; records handed out eight at a time ----
        if (hit) {
          const int rank = __popcll(hit_mask & ((1ull << lane) - 1ull));
          const float rec[15] = {p.x, p.y, p.z, n.x, n.y, n.z, tbn.x.x, tbn.x.y, tbn.x.z, tbn.y.x, tbn.y.y, tbn.y.z, tbn.z.x, tbn.z.y, tbn.z.z};
#pragma unroll
          for (int f = 0; f < 15; f++) slab[f * 64 + rank] = rec[f];
          reinterpret_cast<unsigned*>(slab)[15 * 64 + rank] = pixel;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        for (int first = 0; first < nrec; first += 8) {
          // ---- phase B, lane = one occlusion ray ----
          const int rec = first + int(lane >> 3);
          const bool active = rec < nrec;
          bool clear = false;
          if (active) {
            float q[15];
#pragma unroll
            for (int f = 0; f < 15; f++) q[f] = slab[f * 64 + rec];
            const f3 rn = ld3(q + 3);
            const m3 frame{ld3(q + 6), ld3(q + 9), ld3(q + 12)};
            DRay sr = spawn_ray(ld3(q), rn, face_same_hemisphere(mul(frame, my_dir), rn), A.radius);
            int g2, p2;
            clear = !scene_traverse<true, F>(V, sr, stack, g2, p2);
          }
          const unsigned long long clear_mask = __ballot(clear);
          if (active && (lane & 7u) == 0u) {
            const unsigned k = __popc(unsigned(clear_mask >> lane) & 0xffu);
            if (k) atomicAdd(&counts[reinterpret_cast<const unsigned*>(slab)[15 * 64 + rec]], k);
          }
        }
        // (the next sample's records overwrite the slab: every read above comes first)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (lane == 0 && hits) {
    atomicAdd(&counters->vertices, hits);
    atomicAdd(&counters->shadow_rays, rays);
  }
}

// film[p] = vec4(L / spp, 1) (integrator.cpp:96) with L = count / 8, exact: one thread per pixel of the shard's tiles.
static __global__ void __launch_bounds__(kBlock) ao_film_kernel(WorkParams W, int film_w, int film_h, int spp, const unsigned* __restrict__ counts,
                                                               float4* __restrict__ film) {
  const unsigned long long t = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  const int ltile = int(t >> 6);
  if (ltile >= W.num_local_tiles) return;
  const int q = int(t & 63);
  const int tile = film_tile_of(W, ltile);
  const int px = (tile % W.tiles_x) * kTile + (q & 7), py = (tile / W.tiles_x) * kTile + (q >> 3);
  if (px >= film_w || py >= film_h) return;
  const size_t at = size_t(py) * film_w + px;
  const float v = (float(counts[at]) * 0.125f) / float(spp);
  film[at] = make_float4(v, v, v, 1.0f);
}

// The precompiled variants: {analytic shapes with the scene in LDS, every shape kind from global memory} x {BlueSampler, all
// three samplers}, each in both schedules.  The host takes the first that covers the scene.
struct PineAoVariant {
  unsigned features;
  const void* regrouped;
  const void* serial;
  const char* name;
};
constexpr unsigned kFAoAnalytic = F_AABB | F_OBB | F_SPHERE | F_DISK | F_CONE;
constexpr unsigned kFAoShapes = kFAoAnalytic | F_MESH | F_XSHAPES;
const PineAoVariant* pine_gpu_ao_variants(int* count);  // pine_ao_kernels.hip

}  // namespace pine_gpu
