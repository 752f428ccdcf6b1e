// bandk_k3_src.hip -- bandk_src_kernel<3>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(3, Src)
