// bandk_k6_res.hip -- bandk_res_kernel<6>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(6, Res)
