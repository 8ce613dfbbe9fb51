// gemm_mxa4_bf16.hip -- instantiates the MXFP4 x MXFP4 scaled-MFMA kernels (gemm_mxa4.h) for one activation dtype.
#include "gemm_mxa4.h"
namespace lkm {
LKM_DEFINE_MXA4_LAUNCHERS(mxa4_bf16, LKM_DT_BF16)
}  // namespace lkm
