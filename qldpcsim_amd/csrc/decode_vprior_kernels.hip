// decode_vprior_kernels.hip — decode_vprior_kernel (decoder_kernels.hip: the
// generic LDS kernel's body with one prior per variable, a float64 row per
// code staged into LDS) instantiated in a translation unit
// of its own, so the objects of every other kernel are built exactly as
// without it.
#define QLDPC_TU_VPRIOR 1
#include "decoder_kernels.hip"
