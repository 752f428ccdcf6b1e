// stencilk_k3_src.hip -- sweepk_src_kernel<3>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(3, Src)
