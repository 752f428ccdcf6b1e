// stencilk_k5_res.hip -- sweepk_res_kernel<5>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(5, Res)
