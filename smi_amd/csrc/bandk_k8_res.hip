// bandk_k8_res.hip -- bandk_res_kernel<8>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(8, Res)
