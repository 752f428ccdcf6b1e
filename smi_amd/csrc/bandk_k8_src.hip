// bandk_k8_src.hip -- bandk_src_kernel<8>, the source instantiation (stencil_bandk.h)
#include "stencil_bandk.h"
SMI_BANDK_INSTANCE(8, Src)
