// translation unit of the split HIP build (core.h FV3LM_LINK): the bulk of a2b_ord4 as one LDS-tiled launch, nonlinear / tangent / adjoint
#define FV3LM_IMPL_A2B
#include "a2b.h"
