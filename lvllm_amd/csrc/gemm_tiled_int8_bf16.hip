// gemm_tiled_int8_bf16.hip -- LDS-staged tiled grouped GEMMs (gemm_tiled.h: 32 / 64 / 128-row tiles) for weight-only uint8
// experts (LKM_W_INT8).  No 256-row variant: gemm_prefill.h does not decode the format.
#include "gemm_tiled.h"
namespace lkm {
LKM_DEFINE_TILED_LAUNCHERS(int8_bf16, LKM_W_INT8, LKM_DT_BF16)
}  // namespace lkm
