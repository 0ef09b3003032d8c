// combine_t_half.hip -- the fold kernels for IEEE binary16 elements (combine_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "combine_kernels.h"

MI355_COMBINE_TYPE(mi355::f16, half)
