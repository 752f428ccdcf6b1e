// stencilk_k9_res.hip -- sweepk_res_kernel<9>, the residual instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(9, Res)
