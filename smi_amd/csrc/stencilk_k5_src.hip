// stencilk_k5_src.hip -- sweepk_src_kernel<5>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(5, Src)
