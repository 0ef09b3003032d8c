// prefix_t_short.hip -- the prefix-fold kernels for short elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(int16_t, short)
