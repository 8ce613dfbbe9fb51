// gemm_i8a8_f16.hip -- instantiates the int8 x int8 integer-MFMA kernels (gemm_i8a8.h) for one activation dtype.
#include "gemm_i8a8.h"
namespace lkm {
LKM_DEFINE_I8A8_LAUNCHERS(i8a8_f16, LKM_DT_F16)
}  // namespace lkm
