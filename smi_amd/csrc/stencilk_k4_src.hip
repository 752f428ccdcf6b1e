// stencilk_k4_src.hip -- sweepk_src_kernel<4>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(4, Src)
