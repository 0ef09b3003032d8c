// prefix_t_half.hip -- the prefix-fold kernels for half elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(mi355::f16, half)
