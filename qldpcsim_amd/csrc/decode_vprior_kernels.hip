// decode_vprior_kernels.hip — decode_vprior_kernel (decode_generic.h: the
// generic LDS kernel's body with one prior per variable, a float64 row per
// code staged into LDS) instantiated in a translation unit
// of its own, so the objects of every other kernel are built exactly as
// without it.
#include "decode_generic.h"

namespace qldpc {

QLDPC_GENERIC_SELECTOR(select_vprior_kernel, decode_vprior_kernel)

}  // namespace qldpc
