// bandk_k11_res.hip -- bandk_res_kernel<11>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(11, Res)
