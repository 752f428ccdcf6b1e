// bandk_k3_res.hip -- bandk_res_kernel<3>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(3, Res)
