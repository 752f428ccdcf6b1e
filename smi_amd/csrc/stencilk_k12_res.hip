// stencilk_k12_res.hip -- sweepk_res_kernel<12>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_RES_INSTANCE(12)
