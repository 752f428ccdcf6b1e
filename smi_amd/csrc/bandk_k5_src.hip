// bandk_k5_src.hip -- bandk_src_kernel<5>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(5, Src)
