// pine_amd/csrc/pine_guides_kernels.hip -- the precompiled guide-image kernels of DenoiseIntegrator (pine_guides_kernel.h): four
// feature sets.  Exports one plain-typed table; pine_kernels.hip chooses from it (pine_guides_host.h).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "pine_guides_kernel.h"

namespace pine_gpu {

#define PINE_GUIDES_ENTRY(F, NAME) PineGuidesVariant{F, (const void*)guides_kernel<F>, NAME}
static const PineGuidesVariant kGuidesVariants[] = {
    PINE_GUIDES_ENTRY(kFGuidesAnalytic | F_LDS_SCENE, "guides: analytic shapes, scene in LDS, literal albedos"),
    PINE_GUIDES_ENTRY(kFGuidesAnalytic | F_LDS_SCENE | F_NODES, "guides: analytic shapes, scene in LDS, node programs"),
    PINE_GUIDES_ENTRY(kFGuidesShapes, "guides: every shape kind, literal albedos"),
    PINE_GUIDES_ENTRY(kFGuidesShapes | F_NODES, "guides: every shape kind, node programs"),
};

const PineGuidesVariant* pine_gpu_guides_variant_table(int* count) {
  *count = int(sizeof(kGuidesVariants) / sizeof(kGuidesVariants[0]));
  return kGuidesVariants;
}

}  // namespace pine_gpu
