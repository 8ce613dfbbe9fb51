// gemm_mxa4_f16.hip -- instantiates the MXFP4 x MXFP4 scaled-MFMA kernels (gemm_mxa4.h) for one activation dtype.
#include "gemm_mxa4.h"
namespace lkm {
LKM_DEFINE_MXA4_LAUNCHERS(mxa4_f16, LKM_DT_F16)
}  // namespace lkm
