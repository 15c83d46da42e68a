// decode_prior_kernels.hip — decode_prior_kernel (decode_generic.h: the
// generic LDS kernel's body with a per-half-shot mask over the variables and
// two priors) instantiated in a translation unit of its own,
// so the objects of every other kernel are built exactly as without it.
#include "decode_generic.h"

namespace qldpc {

QLDPC_GENERIC_SELECTOR(select_prior_kernel, decode_prior_kernel)

}  // namespace qldpc
