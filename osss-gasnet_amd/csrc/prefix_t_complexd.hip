// prefix_t_complexd.hip -- the prefix-fold kernels for double complex elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(cplxd, complexd)
