// bandk_k5_res.hip -- bandk_res_kernel<5>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(5, Res)
