// stencilk_k6_src.hip -- sweepk_src_kernel<6>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(6, Src)
