// bandk_k9_src.hip -- bandk_src_kernel<9>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(9, Src)
