// prefix_t_int.hip -- the prefix-fold kernels for int elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(int32_t, int)
