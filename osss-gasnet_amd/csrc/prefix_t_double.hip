// prefix_t_double.hip -- the prefix-fold kernels for double elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(double, double)
