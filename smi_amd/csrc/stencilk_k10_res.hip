// stencilk_k10_res.hip -- sweepk_res_kernel<10>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(10, Res)
