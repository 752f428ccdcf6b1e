// stencilk_k9_src.hip -- sweepk_src_kernel<9>, the source instantiation (stencilk.h)
#include "stencilk.h"
SMI_SWEEPK_INSTANCE(9, Src)
