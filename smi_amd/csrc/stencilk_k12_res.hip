// stencilk_k12_res.hip -- sweepk_res_kernel<12>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(12, Res)
