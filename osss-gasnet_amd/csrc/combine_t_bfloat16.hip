// combine_t_bfloat16.hip -- the fold kernels for bfloat16 elements (combine_kernels.h), one
// translation unit per element type so the instantiations compile in parallel.
#include "combine_kernels.h"

MI355_COMBINE_TYPE(mi355::bf16, bfloat16)
