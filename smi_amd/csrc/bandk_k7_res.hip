// bandk_k7_res.hip -- bandk_res_kernel<7>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(7, Res)
