// bandk_k7_src.hip -- bandk_src_kernel<7>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(7, Src)
