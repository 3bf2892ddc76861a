// translation unit of the split HIP build (core.h FV3LM_LINK): the bulk of c_sw's d2a2c_vect as one LDS-tiled launch, nonlinear / tangent / adjoint
#define FV3LM_IMPL_D2A2C
#include "d2a2c.h"
