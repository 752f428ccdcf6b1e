// bandk_k4_src.hip -- bandk_src_kernel<4>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(4, Src)
