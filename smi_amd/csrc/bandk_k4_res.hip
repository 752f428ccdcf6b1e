// bandk_k4_res.hip -- bandk_res_kernel<4>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(4, Res)
