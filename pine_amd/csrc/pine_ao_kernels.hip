// pine_amd/csrc/pine_ao_kernels.hip -- the precompiled AOIntegrator kernels (pine_ao_kernel.h): four feature sets, each as
// the regrouped kernel and as its plain twin.  Exports one plain-typed table; pine_kernels.hip chooses from it.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "pine_ao_kernel.h"

namespace pine_gpu {

#define PINE_AO_ENTRY(F, NAME) PineAoVariant{F, (const void*)ao_kernel<F, true>, (const void*)ao_kernel<F, false>, NAME}
static const PineAoVariant kAoVariants[] = {
    PINE_AO_ENTRY(kFAoAnalytic | F_LDS_SCENE, "ao: analytic shapes, scene in LDS, BlueSampler"),
    PINE_AO_ENTRY(kFAoAnalytic | F_LDS_SCENE | F_SOBOL, "ao: analytic shapes, scene in LDS, all samplers"),
    PINE_AO_ENTRY(kFAoShapes, "ao: every shape kind, BlueSampler"),
    PINE_AO_ENTRY(kFAoShapes | F_SOBOL, "ao: every shape kind, all samplers"),
};

const PineAoVariant* pine_gpu_ao_variants(int* count) {
  *count = int(sizeof(kAoVariants) / sizeof(kAoVariants[0]));
  return kAoVariants;
}

}  // namespace pine_gpu
