// decode_prior_kernels.hip — decode_prior_kernel (decoder_kernels.hip: the
// generic LDS kernel's body with a per-half-shot mask over the variables and
// two priors) instantiated in a translation unit of its own,
// so the objects of every other kernel are built exactly as without it.
#define QLDPC_TU_PRIOR 1
#include "decoder_kernels.hip"
