// translation unit of the split HIP build (core.h FV3LM_LINK): the del-6 damping increment of w and of the interface heights as one LDS-tiled
// launch, nonlinear / tangent / adjoint
#define FV3LM_IMPL_DEL6
#include "del6.h"
