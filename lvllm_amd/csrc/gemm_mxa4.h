// gemm_mxa4.h -- MXFP4 weights x MXFP4 activations (W4A4) on v_mfma_scale_f32_16x16x128_f8f6f4 with BOTH operands fp4 (cbsz = 4,
// blgp = 4): the form of the instruction that runs at the fp4 rate, and the one in which a token's 128-k unit is 64 bytes.
//
//   acc += sum_k w_q[n][k] x_q[m][k] 2^(sw[n][k/32] - 127) 2^(sx[m][k/32] - 127)       (products exact, fp32 sums)
//
// Operands (lane l = g * 16 + i, g = l / 16):
//   * A = weights: the image and the scale image of gemm_mxa8.h, unchanged (repack.hip repack_w_mxa8_kernel /
//     repack_s_mxa8_kernel): lane (g, i) holds row tile*16 + i, k = unit*128 + g*32 + 0..31 as 16 bytes, its E8M0 bytes as one dword
//     per four units, the byte picked by op_sel.
//   * B = tokens, fp4: lane (g, i) holds token block*16 + i, k = unit*128 + g*32 + 0..31 as 16 bytes in the low four dwords of the
//     operand (even k in the low nibble) -- the SAME contiguous 32 k as the A side, unlike the two 64-k halves of an 8-bit
//     operand -- and its scale is the E8M0 byte of (token, 32-block unit*4 + g), the byte of the scale register picked by the B
//     side's op_sel.  Measured (tools/probe_mfma_mx.hip, fp4 B case, one run on MI355X):
//         A (group, nibble) -> B (group, nibble): (g, n) -> (g, n) for all 128 positions
//         fp4 B data in lane group d, scale 2.0 in lane group 0..3: 64 at group d, 32 elsewhere (d = 0..3)
//         fp4 B scale register bytes 1, 2, 4, 8 (x 128 products), op_sel 0..3: 128 256 512 1024
//   * D: lane (g, i) holds rows tile*16 + 4g .. + 3 of token i: the epilogues of gemm_skinny.h apply unchanged.
//
// Token image (dispatch.hip quant_mxfp4_rows_kernel, PAD form): rows padded to whole STAGES of two units (256 k):
// [row][S * 128] value bytes and [row][S] scale pairs of dwords, S = ceil(K / 256).  The eight scale bytes of a stage are stored
// [g][h] (h = unit of the stage), so the two scales of a lane are ONE aligned 16-bit word: one ds_read_u16 per (token block,
// stage), the unit's byte picked by op_sel.  The pad unit of an odd K is value 0 with scale byte 127 and is never multiplied.
//
// Work split: as gemm_mxa8.h -- a workgroup = 4 waves = one (expert, token tile of TBW*16 rows) item of the sort's list x four
// 16-row weight tiles (GEMM1 gated: four gate + the four matching up tiles); a wave owns its tile (pair) over all of K (a K slab
// in GEMM2's split-K, whole groups of four units).  What differs is the K loop: an LDS stage carries TWO units of the token tile
// (TM x 128 B, the footprint of one MXFP8 unit), so there is one s_barrier and one global -> LDS hand-over per 256 k, and a
// fragment is ONE ds_read_b128 per (token block, unit): chunk h*4 + g of the row's 128 bytes.  The XOR swizzle is over the eight
// 16-byte chunks of the stage row with (row >> 1) & 7: rows j and j + 1 are 128 B apart (the two halves of a 256-byte bank row),
// so the 16 rows of a block reading chunk c hit 16 different bank groups, for both units of the stage.  Weights: two register
// stages of two units each, the next stage's 2 x 16 bytes in flight across the barrier.  The steady loop runs one group of four
// units (two stages, op_sel is an immediate) per trip with every load unconditional; the last group runs in the drain.
#pragma once
#include "gemm_tiled.h"

namespace lkm {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// one scaled MFMA, both operands fp4: A scale = byte OA of `sa`, B scale = byte OB of `sb`
template <int OA, int OB>
__device__ __forceinline__ f32x4 mfma_mx4(const u32x4& a, const u32x4& b, const f32x4& c, int sa, int sb) {
    const i32x8 av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const i32x8 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 4, OA, sa, OB, sb);
}

// resident workgroups per CU asked of the register allocator (the decode heights are HBM-latency bound)
constexpr int mxa4_min_blocks(int tbw) { return tbw <= 2 ? 4 : (tbw <= 4 ? 3 : (tbw <= 8 ? 2 : 1)); }

// NTL: nontemporal weight loads -- the host's GemmParams::stream_nt
template <int ADT, bool GATED, bool IS_G1, int TBW, bool NTL>
__global__ __launch_bounds__(256, mxa4_min_blocks(TBW)) void gemm_mxa4_kernel(GemmParams p) {
    constexpr int NTT = (IS_G1 && GATED) ? 2 : 1;
    constexpr int TM = TBW * 16, THREADS = 256, ROWB = 128;      // ROWB: one STAGE (two units) of a token row
    constexpr int BUFB = TM * ROWB + THREADS * 8;         // one stage of the token tile: values + one scale dword pair per THREAD
                                                          // (rows first; the store is unconditional, as in gemm_mxa8.h)
    constexpr int PIECES = TM * 8 / THREADS;              // 16-byte staging pieces per thread and stage
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
    const int U4 = (p.U + 3) >> 2;                        // groups of four units (the scale image's granule)

    // split-K (GEMM2, blockIdx.z = slab) in whole groups of four units = two stages
    const int sk = IS_G1 ? 0 : blockIdx.z;
    const int q0 = IS_G1 ? 0 : (int)((long long)sk * U4 / p.SK), q1 = IS_G1 ? U4 : (int)((long long)(sk + 1) * U4 / p.SK);
    const int u1 = q1 * 4 < p.U ? q1 * 4 : p.U;           // units [q0 * 4, u1)

    const u32x4* wp[NTT];
    const int* sp[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
        const int tile = t ? p.T_half + tile0 : tile0;
        wp[t] = (const u32x4*)p.w + (size_t)e * p.w_estride + (size_t)tile * p.w_tstride + lane;
        sp[t] = (const int*)p.s + ((size_t)e * T_all + tile) * U4 * 64 + lane;
    }

    // staging assignment: piece pc = q * 256 + tid -> (row pc / 8, 16-byte chunk pc % 8 of the stage: unit chunk / 4, lane group
    // chunk % 4); rows past the expert's count read a valid row of the tile (their D columns are never stored)
    const unsigned char* xrow[PIECES];
    int xdst[PIECES];
#pragma unroll
    for (int q = 0; q < PIECES; ++q) {
        const int pc = q * THREADS + tid;
        const int row = pc >> 3, chunk = pc & 7;
        const int r = r0 + row, rr = r < m_e ? r : r0;
        const size_t src_row = IS_G1 ? (size_t)(p.sorted_slot[off_e + rr] / p.top_k) : (size_t)(off_e + rr);
        xrow[q] = (const unsigned char*)p.x + src_row * p.ldx + chunk * 16;
        xdst[q] = row * ROWB + ((chunk ^ x_swizzle<ROWB>(row)) * 16);
    }
    const u32x2* xsrow;
    {
        const int row = tid < TM ? tid : TM - 1;          // (threads past the tile fetch its last row's scales and drop them)
        const int r = r0 + row, rr = r < m_e ? r : r0;
        const size_t src_row = IS_G1 ? (size_t)(p.sorted_slot[off_e + rr] / p.top_k) : (size_t)(off_e + rr);
        xsrow = (const u32x2*)((const unsigned*)p.xscale + src_row * p.ld_xscale);
    }

    f32x4 acc[NTT][TBW];
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int b = 0; b < TBW; ++b) acc[t][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the loop is specialised on the number of 16-token blocks that hold rows (workgroup-uniform, chosen once)
    auto run = [&](auto NBC) __attribute__((always_inline)) {
        constexpr int NB = decltype(NBC)::v;
        u32x4 ws[2][2][NTT];                              // [register stage][unit of the stage][tile]
        u32x4 xs[PIECES];
        u32x2 xsv = {0u, 0u};
        int wsc[NTT], wsc_next[NTT];
        if (q0 >= q1) return;
        const int ulast = u1 - 1, slast = ulast >> 1, qlast = q1 - 1;
        auto load_x = [&](int s) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) xs[q] = *(const u32x4*)(xrow[q] + (size_t)s * ROWB);
            xsv = xsrow[s];
        };
        auto load_w = [&](u32x4 (&st)[2][NTT], int s) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // (the image has no unit past the last: an odd K range loads its last unit twice and multiplies it once)
                const int u = 2 * s + h < ulast ? 2 * s + h : ulast;
#pragma unroll
                for (int t = 0; t < NTT; ++t) {
                    const u32x4* a = wp[t] + (size_t)u * 64;
                    st[h][t] = NTL ? __builtin_nontemporal_load(a) : *a;
                }
            }
        };
        auto store_x = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) *(u32x4*)(xlds + buf * BUFB + xdst[q]) = xs[q];
            *(u32x2*)(xlds + buf * BUFB + TM * ROWB + tid * 8) = xsv;
        };
        // the MFMAs of one stage: J = stage of the group (the weights' op_sel is 2 J + h), UNITS = 2, or 1 in the drain of an odd range
        auto compute = [&](const u32x4 (&st)[2][NTT], int buf, auto JC, auto UC) __attribute__((always_inline)) {
            constexpr int J = decltype(JC)::v, UNITS = decltype(UC)::v;
            const char* xb = xlds + buf * BUFB;
            // At the prefill height (one workgroup per CU, one wave per SIMD) nothing else hides the LDS latency, and a read that is
            // waited for right before its MFMAs exposes it 2 NB times a stage: there the fragment reads run PD token blocks
            // ahead of their MFMAs.  The lower heights keep several waves per SIMD and have no registers to spare for it.
            constexpr int PD = TBW == 16 ? (NB < 4 ? NB : 4) : 0;
            u32x4 x0[NB], x1[NB];
            int sx[NB];
            auto read = [&](auto BC) __attribute__((always_inline)) {
                constexpr int b = decltype(BC)::v;
                const int row = b * 16 + j, sw = x_swizzle<ROWB>(row);
                sx[b] = *(const unsigned short*)(xb + TM * ROWB + row * 8 + g * 2);             // bytes: unit 0, unit 1 of the stage
                x0[b] = *(const u32x4*)(xb + row * ROWB + ((g ^ sw) * 16));                    // k = stage*256 + 32 g .. + 31
                if constexpr (UNITS == 2) x1[b] = *(const u32x4*)(xb + row * ROWB + (((4 + g) ^ sw) * 16));      // ... + 128
            };
            static_for<PD>([&](auto BC) __attribute__((always_inline)) { read(BC); });
            static_for<NB>([&](auto BC) __attribute__((always_inline)) {
                constexpr int b = decltype(BC)::v;
                if constexpr (PD == 0) read(BC);
                else if constexpr (b + PD < NB) read(IC<b + PD>{});
                if constexpr (PD > 0) __builtin_amdgcn_sched_barrier(0);      // (pins the order: the scheduler otherwise sinks each read to its use)
#pragma unroll
                for (int t = 0; t < NTT; ++t) acc[t][b] = mfma_mx4<2 * J, 0>(st[0][t], x0[b], acc[t][b], wsc[t], sx[b]);
                if constexpr (UNITS == 2) {
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t][b] = mfma_mx4<2 * J + 1, 1>(st[1][t], x1[b], acc[t][b], wsc[t], sx[b]);
                }
                if constexpr (PD > 0) __builtin_amdgcn_sched_barrier(0);
            });
        };
        // one stage: the look-ahead loads (clamped to the K range, so unconditional), the MFMAs, the LDS hand-over
        auto stage = [&](int s, auto JC, auto UC) __attribute__((always_inline)) {
            constexpr int J = decltype(JC)::v;
            const int sn = s + 1 < slast ? s + 1 : slast;
            load_x(sn);
            load_w(ws[(J + 1) & 1], sn);
            __builtin_amdgcn_sched_barrier(0);            // loads are issued before the MFMAs
            compute(ws[J & 1], J & 1, JC, UC);
            __builtin_amdgcn_sched_barrier(0);            // ... and the MFMAs before the hand-over
            store_x((J + 1) & 1);
            __syncthreads();
        };
        load_x(q0 * 2);
        load_w(ws[0], q0 * 2);
#pragma unroll
        for (int t = 0; t < NTT; ++t) wsc[t] = sp[t][(size_t)q0 * 64];
        store_x(0);
        __syncthreads();
        int q = q0;
        for (; q < qlast; ++q) {                          // steady: whole groups of two stages, look-ahead inside the range
#pragma unroll
            for (int t = 0; t < NTT; ++t) wsc_next[t] = sp[t][(size_t)(q + 1) * 64];
            stage(q * 2, IC<0>{}, IC<2>{});
            stage(q * 2 + 1, IC<1>{}, IC<2>{});
#pragma unroll
            for (int t = 0; t < NTT; ++t) wsc[t] = wsc_next[t];
        }
        const int left = u1 - q * 4;                      // drain: the last group holds 1 .. 4 units (workgroup-uniform)
        if (left >= 2) stage(q * 2, IC<0>{}, IC<2>{});
        else stage(q * 2, IC<0>{}, IC<1>{});
        if (left >= 4) stage(q * 2 + 1, IC<1>{}, IC<2>{});
        else if (left == 3) stage(q * 2 + 1, IC<1>{}, IC<1>{});
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

    // epilogue (gemm_skinny.h): GEMM1 rounds the accumulators, applies the activation and rounds once more (round_gemm1
    // semantics); GEMM2 writes the fp32 partial rows of its split-K slab
    static_for<TBW>([&](auto BC) __attribute__((always_inline)) {
        constexpr int b = decltype(BC)::v;
        const int r_tok = r0 + b * 16 + j;
        if (r_tok < m_e) {
            const int n = tile0 * 16 + g * 4;
            if (n < p.n_real) {
                if constexpr (IS_G1) store_gemm1_frag<ADT, GATED>(p, acc[0][b], acc[NTT - 1][b], (size_t)(off_e + r_tok), n);
                else store_gemm2_frag(p, acc[0][b], sk, (size_t)(off_e + r_tok), n);
            }
        }
    });
}

template <int ADT, bool GATED, bool IS_G1, int TBW>
static int launch_mxa4_t(hipStream_t st, const GemmParams& p, int max_tiles) {
    constexpr size_t lds = (size_t)2 * (TBW * 16 * 128 + 256 * 8);
    dim3 grid(p.T_half / 4, max_tiles, IS_G1 ? 1 : p.SK), block(256);
    auto kern = p.stream_nt ? gemm_mxa4_kernel<ADT, GATED, IS_G1, TBW, true> : gemm_mxa4_kernel<ADT, GATED, IS_G1, TBW, false>;
    if (lds > 64 * 1024) LKM_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LKM_LAUNCH_GEMM(kern, grid, block, lds, st, p);
    LKM_HIP_CHECK(hipGetLastError());
    return LKM_OK;
}

template <int ADT, bool GATED, bool IS_G1>
static int launch_mxa4(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {
    LKM_REQUIRE(p.T_half % 4 == 0 && p.SK >= 1 && p.SK <= (p.U + 3) / 4, "gemm_mxa4: T_half=%d SK=%d U=%d", p.T_half, p.SK, p.U);
    // a token row is whole stages: (U + 1) / 2 * 128 value bytes and as many scale dword pairs
    LKM_REQUIRE(p.ldx >= (p.U + 1) / 2 * 128 && p.ld_xscale >= (p.U + 1) / 2 * 2 && p.ldx % 16 == 0 && p.ld_xscale % 2 == 0,
                "gemm_mxa4: token rows of %d bytes / %d scale dwords for U=%d", (int)p.ldx, (int)p.ld_xscale, p.U);
    switch (cfg.tiled) {
    case 32: return launch_mxa4_t<ADT, GATED, IS_G1, 2>(st, p, max_tiles);
    case 64: return launch_mxa4_t<ADT, GATED, IS_G1, 4>(st, p, max_tiles);
    case 128: return launch_mxa4_t<ADT, GATED, IS_G1, 8>(st, p, max_tiles);
    case 256: return launch_mxa4_t<ADT, GATED, IS_G1, 16>(st, p, max_tiles);
    }
    set_error("gemm_mxa4: token-tile height %d not built (32, 64, 128, 256)", cfg.tiled);
    return LKM_E_INVALID;
}

#define LKM_DEFINE_MXA4_LAUNCHERS(SUFFIX, ADT)                                                                               \
    int launch_gemm1_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, bool gated, int max_tiles) {  \
        return gated ? launch_mxa4<ADT, true, true>(st, cfg, p, max_tiles) : launch_mxa4<ADT, false, true>(st, cfg, p, max_tiles); \
    }                                                                                                                        \
    int launch_gemm2_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {              \
        return launch_mxa4<ADT, false, false>(st, cfg, p, max_tiles);                                                        \
    }

}  // namespace lkm
