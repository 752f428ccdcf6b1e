// bandk_k10_res.hip -- bandk_res_kernel<10>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(10, Res)
