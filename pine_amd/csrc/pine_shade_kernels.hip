// pine_amd/csrc/pine_shade_kernels.hip -- the precompiled kernels of Shader (pine_shade_kernel.h): the vertex kernel's feature
// sets, and the begin, fold and resolve kernels, which no scene feature touches.  Exports one plain-typed table;
// pine_kernels.hip chooses from it (pine_shade_host.h).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "pine_shade_kernel.h"

namespace pine_gpu {

#define PINE_SHADE_ENTRY(F, NAME) PineShadeVariant{F, (const void*)shade_vertex_kernel<F>, NAME}
static const PineShadeVariant kShadeVariants[] = {
    PINE_SHADE_ENTRY(kFShadeNarrow, "shade: Diffuse and Emissive on analytic shapes, area lights, BlueSampler, scene in LDS"),
    PINE_SHADE_ENTRY(kFShadeAll, "shade: every shape, material, light and sampler kind but Subsurface"),
};

const PineShadeVariant* pine_gpu_shade_variant_table(int* count) {
  *count = int(sizeof(kShadeVariants) / sizeof(kShadeVariants[0]));
  return kShadeVariants;
}
const void* pine_gpu_shade_begin_fn() { return (const void*)shade_begin_kernel<0u>; }
const void* pine_gpu_shade_fold_fn() { return (const void*)shade_fold_kernel<0u>; }
const void* pine_gpu_shade_resolve_fn() { return (const void*)shade_resolve_kernel<0u>; }

}  // namespace pine_gpu
