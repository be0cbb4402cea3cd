// pine_amd/csrc/pine_guides_kernel.h -- the guide images of DenoiseIntegrator (src/pine/impl/integrator/denoiser.cpp:13-23) on
// gfx950: per pixel ONE closest-hit ray through the pixel centre, camera.gen_ray((p + 0.5) / film_size, (0.5, 0.5)); where it
// hits, albedo[p] = material.albedo({it, it.n}) (material.h:125-130: an Emissive's colour, every other material's albedo node at
// the surface's p, n, uv) and normal[p] = it.n, as the interaction carries it -- not turned towards the camera; zeros on a miss.
// No sampler, no RNG, no checkpoints, no atomics and no waits: lane = pixel, a wave = one 8x8 tile (the path kernels' tiles, for
// the same coherence of the traversal).  Every building block is the path kernels' (scene view and LDS staging of
// pine_radiance.h, camera_gen_ray, scene_traverse in pine-BVH order, hit_surface, material_params): the same bits.
#pragma once
#include "pine_kernels_device.h"

namespace pine_gpu {

// LDS layout (dwords): traversal stack [stack_total][256] | (F_LDS_SCENE) the scene blob
template <unsigned F>
__global__ void __launch_bounds__(kBlock) guides_kernel(DeviceScene S, int tiles_x, int num_tiles, float* __restrict__ albedo, float* __restrict__ normal) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  int* const stack = lds_raw + tid;
  SceneView V;
  if constexpr (F & F_LDS_SCENE) V = scene_view_staged(S, reinterpret_cast<uint4*>(lds_raw + S.stack_total * kBlock), tid, kBlock);
  else V = scene_view_global(S);
  __syncthreads();  // (the scene staged above; every lane arrives: nothing returns before this)
  const int tile = int(blockIdx.x) * (kBlock / 64) + int(tid >> 6);
  if (tile >= num_tiles) return;
  const int px = (tile % tiles_x) * kTile + int(lane & 7u), py = (tile / tiles_x) * kTile + int(lane >> 3);
  if (px >= S.cam.W || py >= S.cam.H) return;
  DRay r = camera_gen_ray(S.cam, f2{(float(px) + 0.5f) / float(S.cam.W), (float(py) + 0.5f) / float(S.cam.H)}, f2{0.5f, 0.5f});
  f3 a = mk3(0.0f), n = mk3(0.0f);
  int geom = -1, prim = 0;
  if (scene_traverse<false, F>(V, r, stack, geom, prim)) {
    const DShape* shape = &V.shapes[geom & kPrimIndexMask];
    DSurface it;
    hit_surface<F>(V, shape, prim, r.o, r.d, r.tmax, it);
    a = material_params<F>(&V.materials[shape->material], V.node_ops, V.tex, it.p, it.n, it.uv).albedo;
    n = it.n;
  }
  const size_t at = (size_t(py) * size_t(S.cam.W) + size_t(px)) * 3;
  albedo[at] = a.x, albedo[at + 1] = a.y, albedo[at + 2] = a.z;
  normal[at] = n.x, normal[at + 1] = n.y, normal[at + 2] = n.z;
}

// The precompiled variants: {analytic shapes with the scene in LDS, every shape kind from global memory} x {literal albedos,
// node programs}.  The host takes the first that covers the scene.
struct PineGuidesVariant {
  unsigned features;
  const void* fn;
  const char* name;
};
constexpr unsigned kFGuidesAnalytic = F_AABB | F_OBB | F_SPHERE | F_DISK | F_CONE;
constexpr unsigned kFGuidesShapes = kFGuidesAnalytic | F_MESH | F_XSHAPES;
const PineGuidesVariant* pine_gpu_guides_variant_table(int* count);  // pine_guides_kernels.hip

}  // namespace pine_gpu
