// stencilk_k6_res.hip -- sweepk_res_kernel<6>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(6, Res)
