// stencilk_k8_src.hip -- sweepk_src_kernel<8>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(8, Src)
