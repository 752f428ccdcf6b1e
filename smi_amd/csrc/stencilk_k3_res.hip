// stencilk_k3_res.hip -- sweepk_res_kernel<3>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(3, Res)
