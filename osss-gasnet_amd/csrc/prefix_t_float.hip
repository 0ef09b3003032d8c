// prefix_t_float.hip -- the prefix-fold kernels for float elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(float, float)
