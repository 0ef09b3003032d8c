// prefix_t_longdouble.hip -- the prefix-fold kernels for long double elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(x80, longdouble)
