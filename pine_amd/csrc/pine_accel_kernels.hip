// pine_amd/csrc/pine_accel_kernels.hip -- the precompiled ray-query kernels of Accel (pine_accel_kernel.h): four feature sets, an
// intersect and a hit kernel each, and the camera-ray kernel.  Exports one plain-typed table; pine_kernels.hip chooses from it
// (pine_accel_host.h).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "pine_accel_kernel.h"

namespace pine_gpu {

// The rays DenoiseIntegrator's guide images use (denoiser.cpp:13-23): camera.gen_ray((p + 0.5) / film_size, (0.5, 0.5)) for every
// pixel, row-major, tmin = 0 and tmax = FLT_MAX (ray.h:10-11).  One thread per pixel.
static __global__ void __launch_bounds__(kBlock) accel_camera_rays_kernel(DCamera cam, float4* __restrict__ rays) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= (long long)cam.W * cam.H) return;
  const int px = int(i % cam.W), py = int(i / cam.W);
  const DRay r = camera_gen_ray(cam, f2{(float(px) + 0.5f) / float(cam.W), (float(py) + 0.5f) / float(cam.H)}, f2{0.5f, 0.5f});
  rays[2 * i] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
  rays[2 * i + 1] = make_float4(r.d.y, r.d.z, r.tmin, r.tmax);
}

#define PINE_ACCEL_ENTRY(F, NAME) PineAccelVariant{F, (const void*)accel_intersect_kernel<F>, (const void*)accel_hit_kernel<F>, NAME}
static const PineAccelVariant kAccelVariants[] = {
    PINE_ACCEL_ENTRY(kFAccelAnalytic | F_LDS_SCENE, "accel: analytic shapes, scene in LDS, pine-BVH order"),
    PINE_ACCEL_ENTRY(kFAccelAnalytic | F_LDS_SCENE | F_EMBREE, "accel: analytic shapes, scene in LDS, EmbreeAccel's order"),
    PINE_ACCEL_ENTRY(kFAccelShapes, "accel: every shape kind, pine-BVH order"),
    PINE_ACCEL_ENTRY(kFAccelShapes | F_EMBREE, "accel: every shape kind, EmbreeAccel's order"),
};

const PineAccelVariant* pine_gpu_accel_variant_table(int* count) {
  *count = int(sizeof(kAccelVariants) / sizeof(kAccelVariants[0]));
  return kAccelVariants;
}
const void* pine_gpu_accel_camera_rays_fn() { return (const void*)accel_camera_rays_kernel; }

}  // namespace pine_gpu
