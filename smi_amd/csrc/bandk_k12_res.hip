// bandk_k12_res.hip -- bandk_res_kernel<12>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(12, Res)
