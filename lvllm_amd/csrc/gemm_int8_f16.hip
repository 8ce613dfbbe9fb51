// gemm_int8_f16.hip -- skinny grouped-GEMM kernels (gemm_skinny.h) for weight-only uint8 experts (LKM_W_INT8: uint8b128 or
// uint8 + zero points), decoded to T((q - zp) * s) in registers.
#include "gemm_skinny.h"
namespace lkm {
LKM_DEFINE_GEMM_LAUNCHERS(int8_f16, LKM_W_INT8, LKM_DT_F16)
}  // namespace lkm
