// prefix_t_complexf.hip -- the prefix-fold kernels for float complex elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(cplxf, complexf)
