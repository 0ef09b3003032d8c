// prefix_t_bfloat16.hip -- the prefix-fold kernels for bfloat16 elements (prefix_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "prefix_kernels.h"

MI355_PREFIX_TYPE(mi355::bf16, bfloat16)
