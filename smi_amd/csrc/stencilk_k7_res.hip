// stencilk_k7_res.hip -- sweepk_res_kernel<7>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(7, Res)
