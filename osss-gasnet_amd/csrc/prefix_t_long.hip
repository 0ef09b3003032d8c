// prefix_t_long.hip -- the prefix-fold kernels for long elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(int64_t, long)
