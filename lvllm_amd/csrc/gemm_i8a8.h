// gemm_i8a8.h -- int8 weights (one fp32 scale per weight row) x per-token int8 activations (W8A8-int8, the reference's
// int8_w8a8_moe_quant_config with per_act_token_quant) on v_mfma_i32_16x16x64_i8.  The K loop holds no scale arithmetic and
// no decode: the sums are exact int32 (128 * 127 * K < 2^31 for K <= 131072), both scales meet the accumulator once:
//
//   out[m][n] = float(sum_k x_q[m][k] w_q[n][k]) * sx[m] * sw[n]                        (the reference's As * C * Bs)
//
// Operands (lane l = g * 16 + i, g = l / 16):
//   * A = weights: the fp8 W8A8 image byte for byte (repack.hip, RepackDims::a8) -- [tile][unit][pair][lane][16 B], lane (g, i)
//     holds row tile*16 + i, k = unit*128 + pair*64 + g*16 + 0..15: one wave-wide 16-byte load is the A operand of one MFMA,
//     straight HBM -> VGPR.  Scale image: plain fp32 [expert][tiles * 16] (padded rows 0): one 16-byte load per lane and tile
//     fetches the scales of rows 4g .. 4g + 3, the lane's rows of D.
//   * B = tokens: lane (g, j) holds the SAME 16 k of token block*16 + j (an MFMA sums over its k: any assignment that A and B
//     share is valid, lkm_common.h).  The quantiser (dispatch.hip quant_int8_rows_kernel) writes rows padded to whole units
//     with zero bytes and one fp32 scale per row; the workgroup's token tile goes through LDS once per unit (rows gathered
//     through the sort's sorted_slot list, 16-byte pieces XOR-swizzled as in gemm_mxa8.h) -- and nothing else does: there is
//     no per-unit scale traffic.  The token scale is fetched once per lane, in the epilogue, through the same gather.
//   * D: lane (g, j) holds rows tile*16 + 4g .. + 3 of token j: the epilogues of gemm_skinny.h apply unchanged.
//
// Work split: a workgroup = 4 waves = one (expert, token tile of TBW*16 rows) item of the sort's list x four 16-row weight tiles
// (GEMM1 gated: four gate + the four matching up tiles).  A wave owns its tile (pair) over all of K (a K slab of whole units
// in GEMM2's split-K) and multiplies it against every token block of the tile.  Weights: two register stages, the next unit's
// 2 x 16 bytes in flight across the barrier; tokens: registers -> LDS double buffer, one s_barrier per unit.  The loop runs two
// units per trip (the stage index is static) with every load unconditional; an odd last unit runs once more on stage 0.
#pragma once
#include "gemm_tiled.h"

namespace lkm {

typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ i32x4 mfma_i8(const u32x4& a, const u32x4& b, const i32x4& c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
}

// resident workgroups per CU asked of the register allocator: the decode heights are HBM-latency bound (resident waves hide it)
constexpr int i8a8_min_blocks(int tbw) { return tbw <= 2 ? 4 : (tbw <= 4 ? 3 : (tbw <= 8 ? 2 : 1)); }

// NTL: nontemporal weight loads -- the host's GemmParams::stream_nt (an expert's rows fit one token tile: weights are read once)
template <int ADT, bool GATED, bool IS_G1, int TBW, bool NTL>
__global__ __launch_bounds__(256, i8a8_min_blocks(TBW)) void gemm_i8a8_kernel(GemmParams p) {
    constexpr int NTT = (IS_G1 && GATED) ? 2 : 1;
    constexpr int TM = TBW * 16, THREADS = 256, ROWB = 128;
    constexpr int BUFB = TM * ROWB;                       // one unit of the token tile
    constexpr int PIECES = TM * 8 / THREADS;              // 16-byte staging pieces per thread and unit
    static_assert(PIECES >= 1, "staging split");
    extern __shared__ __attribute__((aligned(16))) char xlds[];   // [2][BUFB]

    const int ti = blockIdx.y;
    if (ti >= p.meta[3]) return;
    const int e = p.tile_e[ti], r0 = p.tile_r0[ti];
    const int m_e = p.counts[e], off_e = p.offsets[e];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int tile0 = blockIdx.x * 4 + wave;              // (T_half % 4 == 0: every wave has a tile)
    const int T_all = p.T_half * p.halves;

    // split-K (GEMM2, blockIdx.z = slab) in whole units
    const int sk = IS_G1 ? 0 : blockIdx.z;
    const int u0 = IS_G1 ? 0 : (int)((long long)sk * p.U / p.SK), u1 = IS_G1 ? p.U : (int)((long long)(sk + 1) * p.U / p.SK);

    const u32x4* wp[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
        const int tile = t ? p.T_half + tile0 : tile0;
        wp[t] = (const u32x4*)p.w + (size_t)e * p.w_estride + (size_t)tile * p.w_tstride + lane;
    }

    // the token row behind row `row` of the tile; rows past the expert's count re-read the tile's first row (their D columns
    // are never stored), so no load is conditional
    auto src_row_of = [&](int row) __attribute__((always_inline)) {
        const int r = r0 + row, rr = r < m_e ? r : r0;
        return IS_G1 ? (size_t)(p.sorted_slot[off_e + rr] / p.top_k) : (size_t)(off_e + rr);
    };
    // staging assignment: piece pc = q * 256 + tid -> (row pc / 8, 16-byte chunk pc % 8)
    const unsigned char* xrow[PIECES];
    int xdst[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const int pc = q * THREADS + tid;
        const int row = pc >> 3, chunk = pc & 7;
        xrow[q] = (const unsigned char*)p.x + src_row_of(row) * p.ldx + chunk * 16;
        xdst[q] = row * ROWB + ((chunk ^ x_swizzle<ROWB>(row)) * 16);
    }

    i32x4 acc[NTT][TBW];
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int b = 0; b < TBW; ++b) acc[t][b] = i32x4{0, 0, 0, 0};

    // the loop is specialised on the number of 16-token blocks that hold rows (workgroup-uniform, chosen once)
    auto run = [&](auto NBC) __attribute__((always_inline)) {
        constexpr int NB = decltype(NBC)::v;
        u32x4 ws[2][NTT][2];
        u32x4 xs[PIECES];
        auto load_x = [&](int u) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) xs[q] = *(const u32x4*)(xrow[q] + (size_t)u * ROWB);
        };
        auto load_w = [&](u32x4 (&s)[NTT][2], int u) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < NTT; ++t)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const u32x4* a = wp[t] + (size_t)u * p.w_ustride + h * 64;
                    s[t][h] = NTL ? __builtin_nontemporal_load(a) : *a;
                }
        };
        auto store_x = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) *(u32x4*)(xlds + buf * BUFB + xdst[q]) = xs[q];
        };
        auto compute = [&](const u32x4 (&s)[NTT][2], int buf) __attribute__((always_inline)) {
            const char* xb = xlds + buf * BUFB;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int row = b * 16 + j, sw = x_swizzle<ROWB>(row);
#pragma unroll
                for (int h = 0; h < 2; ++h) {             // k = h * 64 + 16 g .. + 15: the 16-byte piece 4 h + g of the row's unit
                    const u32x4 xv = *(const u32x4*)(xb + row * ROWB + (((4 * h + g) ^ sw) * 16));
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t][b] = mfma_i8(s[t][h], xv, acc[t][b]);
                }
            }
        };
        if (u0 >= u1) return;
        const int ulast = u1 - 1;
        load_x(u0);
        load_w(ws[0], u0);
        store_x(0);
        __syncthreads();
        // one unit: the look-ahead loads (clamped to the K range, so unconditional), the MFMAs, the LDS hand-over
        auto unit = [&](int uu, auto JC) __attribute__((always_inline)) {
            constexpr int J = decltype(JC)::v;
            const int un = uu < ulast ? uu + 1 : ulast;
            load_x(un);
            load_w(ws[J ^ 1], un);
            __builtin_amdgcn_sched_barrier(0);            // loads are issued before the MFMAs
            compute(ws[J], J);
            __builtin_amdgcn_sched_barrier(0);            // ... and the MFMAs before the hand-over
            store_x(J ^ 1);
            __syncthreads();
        };
        int u = u0;
        for (; u + 1 < u1; u += 2) {
            unit(u, IC<0>{});
            unit(u + 1, IC<1>{});
        }
        if (u < u1) unit(u, IC<0>{});
    };
    {
        const int rows_here = m_e - r0 < TM ? m_e - r0 : TM;
        const int nb = (rows_here + 15) >> 4;
        if constexpr (TBW == 2) {
            if (nb <= 1) run(IC<1>{});
            else run(IC<2>{});
        } else {
            if (nb <= TBW / 4) run(IC<TBW / 4>{});
            else if (nb <= TBW / 2) run(IC<TBW / 2>{});
            else run(IC<TBW>{});
        }
    }

    // epilogue: (float(acc) * sx[token]) * sw[row], then gemm_skinny.h -- GEMM1 rounds, applies the activation and rounds once
    // more (round_gemm1 semantics); GEMM2 writes the fp32 partial rows of its split-K slab.  The token factor goes through
    // splat2_opaque (lkm_common.h: no packed multiply with a mixed operand swizzle), the row factors are a plain vector.
    f32x4 wsc[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
        const int tile = t ? p.T_half + tile0 : tile0;
        wsc[t] = *((const f32x4*)((const float*)p.s + ((size_t)e * T_all + tile) * 16) + g);
    }
    auto scaled = [&](const i32x4& a, const f32x2& sx, const f32x4& sw) __attribute__((always_inline)) {
        return scale4(f32x4{(float)a.x, (float)a.y, (float)a.z, (float)a.w}, sx) * sw;
    };
    static_for<TBW>([&](auto BC) __attribute__((always_inline)) {
        constexpr int b = decltype(BC)::v;
        const int r_tok = r0 + b * 16 + j;
        if (r_tok < m_e) {
            const int n = tile0 * 16 + g * 4;
            if (n < p.n_real) {
                const f32x2 sx = splat2_opaque(p.xscale[src_row_of(b * 16 + j)]);
                if constexpr (IS_G1)
                    store_gemm1_frag<ADT, GATED>(p, scaled(acc[0][b], sx, wsc[0]), scaled(acc[NTT - 1][b], sx, wsc[NTT - 1]), (size_t)(off_e + r_tok), n);
                else
                    store_gemm2_frag(p, scaled(acc[0][b], sx, wsc[0]), sk, (size_t)(off_e + r_tok), n);
            }
        }
    });
}

template <int ADT, bool GATED, bool IS_G1, int TBW>
static int launch_i8a8_t(hipStream_t st, const GemmParams& p, int max_tiles) {
    constexpr size_t lds = (size_t)2 * TBW * 16 * 128;
    dim3 grid(p.T_half / 4, max_tiles, IS_G1 ? 1 : p.SK), block(256);
    auto kern = p.stream_nt ? gemm_i8a8_kernel<ADT, GATED, IS_G1, TBW, true> : gemm_i8a8_kernel<ADT, GATED, IS_G1, TBW, false>;
    if (lds > 64 * 1024) LKM_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LKM_LAUNCH_GEMM(kern, grid, block, lds, st, p);
    LKM_HIP_CHECK(hipGetLastError());
    return LKM_OK;
}

template <int ADT, bool GATED, bool IS_G1>
static int launch_i8a8(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {
    LKM_REQUIRE(p.T_half % 4 == 0 && p.SK >= 1 && p.SK <= p.U && p.w_ustride == 128, "gemm_i8a8: T_half=%d SK=%d U=%d", p.T_half, p.SK, p.U);
    switch (cfg.tiled) {
    case 32: return launch_i8a8_t<ADT, GATED, IS_G1, 2>(st, p, max_tiles);
    case 64: return launch_i8a8_t<ADT, GATED, IS_G1, 4>(st, p, max_tiles);
    case 128: return launch_i8a8_t<ADT, GATED, IS_G1, 8>(st, p, max_tiles);
    case 256: return launch_i8a8_t<ADT, GATED, IS_G1, 16>(st, p, max_tiles);
    }
    set_error("gemm_i8a8: token-tile height %d not built (32, 64, 128, 256)", cfg.tiled);
    return LKM_E_INVALID;
}

#define LKM_DEFINE_I8A8_LAUNCHERS(SUFFIX, ADT)                                                                               \
    int launch_gemm1_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, bool gated, int max_tiles) {  \
        return gated ? launch_i8a8<ADT, true, true>(st, cfg, p, max_tiles) : launch_i8a8<ADT, false, true>(st, cfg, p, max_tiles); \
    }                                                                                                                        \
    int launch_gemm2_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {              \
        return launch_i8a8<ADT, false, false>(st, cfg, p, max_tiles);                                                        \
    }

}  // namespace lkm
