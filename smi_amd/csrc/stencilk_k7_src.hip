// stencilk_k7_src.hip -- sweepk_src_kernel<7>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(7, Src)
