// stencilk_k8_res.hip -- sweepk_res_kernel<8>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(8, Res)
