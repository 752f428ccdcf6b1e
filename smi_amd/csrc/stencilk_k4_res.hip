// stencilk_k4_res.hip -- sweepk_res_kernel<4>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(4, Res)
