// pine_amd/csrc/pine_accel_kernel.h -- Accel's ray queries (src/pine/core/accel.h:10-25: intersect(ray, it), hit(ray)) on gfx950,
// batched: N rays in device memory in, N answers in device memory out.  What RTIntegrator::intersect / hit hand to a
// CustomRayIntegrator's radiance() (core/integrator.h:31-38, :61-74), for callers that write their own integrator over ray queries.
// No sampler, no RNG, no atomics, no waits between lanes and no persistent loop: lane = ray.  Every building block is the path
// kernels' (scene view and LDS staging of pine_radiance.h, scene_traverse in pine-BVH order or -- F_EMBREE -- in EmbreeAccel's,
// hit_surface, camera_gen_ray): the same bits.  The traversal stack is the guide kernel's ([slot][thread] in LDS, 32-bit entries
// whatever the node count); an F_EMBREE variant's BVH8 stack is scene_traverse_embree's own.
//
// One ray is 8 floats, o[3] d[3] tmin tmax: two 16-byte loads.  The direction is used as given (not normalised: t is in units of
// d) and tmin is honoured.  A ray with non-finite words or a zero direction is answered without a fault -- every box and shape test
// is a comparison that fails on NaN, a stack never grows past the tree's depth (pine_traverse.h bvh2_walk: one push per inner node
// on the way down; scene_traverse_embree: the host checked the hierarchy against kEmbreeStackEntries) and every index comes from
// the tree, not from the ray -- but WHAT is answered is unspecified.
#pragma once
#include "pine_kernels_device.h"

namespace pine_gpu {

// One answer of accel_intersect_kernel: 12 words, three 16-byte stores.  On a miss: the ray's tmax as it came, -1 -1 -1, zeros.
//   0     f32  ray.tmax after the query
//   1     i32  geometry index (scene.add order)
//   2     i32  triangle index within its mesh; -1 for every other shape
//   3     i32  material index
//   4-6   f32  it.p        7-9  f32  it.n (not turned towards the ray)        10-11  f32  it.uv
constexpr int kAccelRayFloats = 8, kAccelHitWords = 12;

__device__ __forceinline__ DRay accel_load_ray(const float4* __restrict__ rays, long long i) {
  const float4 a = rays[2 * i], b = rays[2 * i + 1];
  return DRay{f3{a.x, a.y, a.z}, f3{a.w, b.x, b.y}, b.z, b.w};
}

// LDS layout (dwords): traversal stack [stack_total][256] | (F_LDS_SCENE) the scene blob
template <unsigned F>
__device__ __forceinline__ SceneView accel_scene_view(const DeviceScene& S, int* lds_raw, unsigned tid) {
  SceneView V;
  if constexpr (F & F_LDS_SCENE) V = scene_view_staged(S, reinterpret_cast<uint4*>(lds_raw + S.stack_total * kBlock), tid, kBlock);
  else V = scene_view_global(S);
  __syncthreads();  // (the scene staged above; every lane arrives, the ones past the last ray too: nothing returns before this)
  return V;
}

template <unsigned F>
__global__ void __launch_bounds__(kBlock) accel_intersect_kernel(DeviceScene S, const float4* __restrict__ rays, long long n, float4* __restrict__ hits) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  const unsigned tid = threadIdx.x;
  int* const stack = lds_raw + tid;
  const SceneView V = accel_scene_view<F>(S, lds_raw, tid);
  const long long i = (long long)blockIdx.x * kBlock + tid;
  if (i >= n) return;
  DRay r = accel_load_ray(rays, i);
  DSurface it;
  it.p = it.n = mk3(0.0f);
  it.uv = f2{0.0f, 0.0f};
  int geom = -1, prim = 0, index = -1, tri = -1, material = -1;
  if (scene_traverse<false, F>(V, r, stack, geom, prim)) {
    index = geom & kPrimIndexMask;
    const DShape* shape = &V.shapes[index];
    hit_surface<F>(V, shape, prim, r.o, r.d, r.tmax, it);
    material = shape->material;
    if constexpr (F & F_MESH)
      if ((geom >> kPrimKindShift) == SHAPE_MESH) tri = prim - V.bvhs[as_int(shape->f[2])].prim_base;
  }
  float4* o = hits + 3 * i;
  o[0] = make_float4(r.tmax, __int_as_float(index), __int_as_float(tri), __int_as_float(material));
  o[1] = make_float4(it.p.x, it.p.y, it.p.z, it.n.x);
  o[2] = make_float4(it.n.y, it.n.z, it.uv.x, it.uv.y);
}

template <unsigned F>
__global__ void __launch_bounds__(kBlock) accel_hit_kernel(DeviceScene S, const float4* __restrict__ rays, long long n, unsigned char* __restrict__ occluded) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  const unsigned tid = threadIdx.x;
  int* const stack = lds_raw + tid;
  const SceneView V = accel_scene_view<F>(S, lds_raw, tid);
  const long long i = (long long)blockIdx.x * kBlock + tid;
  if (i >= n) return;
  DRay r = accel_load_ray(rays, i);
  int geom = -1, prim = 0;
  occluded[i] = scene_traverse<true, F>(V, r, stack, geom, prim) ? 1 : 0;
}

// The precompiled variants: {analytic shapes with the scene in LDS, every shape kind from global memory} x {pine-BVH order,
// EmbreeAccel's order}.  No material is evaluated: no F_NODES.  The host takes the first that covers the scene.
struct PineAccelVariant {
  unsigned features;
  const void* intersect;
  const void* hit;
  const char* name;
};
constexpr unsigned kFAccelAnalytic = F_AABB | F_OBB | F_SPHERE | F_DISK | F_CONE;
constexpr unsigned kFAccelShapes = kFAccelAnalytic | F_MESH | F_XSHAPES;
const PineAccelVariant* pine_gpu_accel_variant_table(int* count);  // pine_accel_kernels.hip
const void* pine_gpu_accel_camera_rays_fn();  // accel_camera_rays_kernel(DCamera, float4* rays), pine_accel_kernels.hip

}  // namespace pine_gpu
