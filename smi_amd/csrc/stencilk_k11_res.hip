// stencilk_k11_res.hip -- sweepk_res_kernel<11>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(11, Res)
