// gemm_mxa8_bf16.hip -- instantiates the MXFP4 x MXFP8 scaled-MFMA kernels (gemm_mxa8.h) for one activation dtype.
#include "gemm_mxa8.h"
namespace lkm {
LKM_DEFINE_MXA8_LAUNCHERS(mxa8_bf16, LKM_DT_BF16)
}  // namespace lkm
