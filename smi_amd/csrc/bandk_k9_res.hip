// bandk_k9_res.hip -- bandk_res_kernel<9>, the residual instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(9, Res)
