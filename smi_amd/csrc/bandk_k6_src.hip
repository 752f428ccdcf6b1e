// bandk_k6_src.hip -- bandk_src_kernel<6>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(6, Src)
