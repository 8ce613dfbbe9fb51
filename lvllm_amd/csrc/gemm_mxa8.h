// gemm_mxa8.h -- MXFP4 weights x MXFP8 activations (W4A8) on v_mfma_scale_f32_16x16x128_f8f6f4: the one weight format whose
// 1 x 32 E8M0 block scales ARE the instruction's per-lane scales, so a 128-k unit is ONE instruction per (16-row weight tile,
// 16-token block) and the kernel holds no decode or scale arithmetic at all.
//
//   acc += sum_k w_q[n][k] x_q[m][k] 2^(sw[n][k/32] - 127) 2^(sx[m][k/32] - 127)       (products exact, fp32 sums)
//
// Operands (lane l = g * 16 + i, g = l / 16):
//   * A = weights, cbsz = fp4: lane (g, i) holds row tile*16 + i, k = unit*128 + g*32 + 0..31 as 16 bytes (two E2M1 per byte,
//     even k in the low nibble); its scale is the E8M0 byte of (row, 32-block unit*4 + g).  Image (repack.hip
//     repack_w_mxa8_kernel): [expert][tile][unit][lane][16 B] -- one wave-wide 16-byte load per (tile, unit), 1 KiB contiguous,
//     straight HBM -> VGPR.  Scale image: [expert][tile][unit / 4][lane] dwords, byte j = the lane's scale in unit 4 q + j:
//     one dword load per FOUR units, the byte picked by the instruction's op_sel (no per-lane extraction in the K loop).
//   * B = tokens, blgp = fp8 e4m3: lane (g, i) holds token block*16 + i as 32 bytes, but NOT the same 32 k: an 8-bit operand of
//     this instruction is two 64-k halves -- bytes 0..15 are k = unit*128 + 16 g + 0..15, bytes 16..31 are k = unit*128 + 64 + 16 g
//     + 0..15 (the 16-byte pieces g and 4 + g of the row's unit) -- while the SCALE register of lane (g, i) still belongs to
//     (token, 32-block unit*4 + g), the block of k = 32 g .. + 31.  Measured: tools/probe_mfma_mx.hip (also: op_sel j = byte j of
//     the scale register, the fp4 operand is the contiguous 32 k of its lane).  The quantiser (dispatch.hip quant_mxfp8_rows_kernel) writes rows padded to whole units --
//     [row][U*128] value bytes, [row][U] scale dwords -- so a unit of a row is 128 B + one aligned dword; the workgroup's token
//     tile goes through LDS once per unit (rows gathered through the sort's sorted_slot list as gemm_tiled.h does, 16-byte
//     pieces XOR-swizzled so that the ds_read_b128 of 16 rows hit 16 bank groups), the scale byte of a lane is a ds_read_u8.
//   * D: lane (g, i) holds rows tile*16 + 4g .. + 3 of token i: the epilogues of gemm_skinny.h apply unchanged.
//
// Work split: a workgroup = 4 waves = one (expert, token tile of TBW*16 rows) item of the sort's list x four 16-row weight tiles
// (GEMM1 gated: four gate + the four matching up tiles).  A wave owns its tile (pair) over all of K (a K slab in GEMM2's
// split-K) and multiplies it against every token block of the tile.  Weights: two register stages, the next unit's 16 bytes in
// flight across the barrier; tokens: registers -> LDS double buffer, one s_barrier per unit.  The steady loop runs four units
// per trip (op_sel is an immediate) with every load unconditional; the last group of a K range runs in the drain loop.
#pragma once
#include "gemm_tiled.h"

namespace lkm {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// one scaled MFMA: A fp4 (cbsz 4) with scale byte OPSEL of `sa`, B fp8 e4m3 (blgp 0) with scale byte 0 of `sb`
template <int OPSEL>
__device__ __forceinline__ f32x4 mfma_mx(const u32x4& a, const u32x4& blo, const u32x4& bhi, const f32x4& c, int sa, int sb) {
    const i32x8 av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
    const i32x8 bv = {(int)blo.x, (int)blo.y, (int)blo.z, (int)blo.w, (int)bhi.x, (int)bhi.y, (int)bhi.z, (int)bhi.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 0, OPSEL, sa, 0, sb);
}

// resident workgroups per CU asked of the register allocator: the decode heights are HBM-latency bound (resident waves hide it)
constexpr int mxa8_min_blocks(int tbw) { return tbw <= 2 ? 4 : (tbw <= 4 ? 3 : (tbw <= 8 ? 2 : 1)); }

// NTL: nontemporal weight loads -- the host's GemmParams::stream_nt (an expert's rows fit one token tile: weights are read once)
template <int ADT, bool GATED, bool IS_G1, int TBW, bool NTL>
__global__ __launch_bounds__(256, mxa8_min_blocks(TBW)) void gemm_mxa8_kernel(GemmParams p) {
    constexpr int NTT = (IS_G1 && GATED) ? 2 : 1;
    constexpr int TM = TBW * 16, THREADS = 256, ROWB = 128;
    constexpr int BUFB = TM * ROWB + THREADS * 4;         // one unit of the token tile: values + one scale dword per THREAD (rows
                                                          // first; the store is unconditional: a branch per unit splits the loop
                                                          // body into blocks and the MFMAs sink through them to their uses)
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
    const int U4 = (p.U + 3) >> 2;                        // groups of four units (the scale image's granule)

    // split-K (GEMM2, blockIdx.z = slab) in whole groups of four units
    const int sk = IS_G1 ? 0 : blockIdx.z;
    const int q0 = IS_G1 ? 0 : (int)((long long)sk * U4 / p.SK), q1 = IS_G1 ? U4 : (int)((long long)(sk + 1) * U4 / p.SK);
    const int u0 = q0 * 4, u1 = q1 * 4 < p.U ? q1 * 4 : p.U;

    const u32x4* wp[NTT];
    const int* sp[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t) {
        const int tile = t ? p.T_half + tile0 : tile0;
        wp[t] = (const u32x4*)p.w + (size_t)e * p.w_estride + (size_t)tile * p.w_tstride + lane;
        sp[t] = (const int*)p.s + ((size_t)e * T_all + tile) * U4 * 64 + lane;
    }

    // staging assignment: piece pc = q * 256 + tid -> (row pc / 8, 16-byte chunk pc % 8); rows past the expert's count read a
    // valid row of the tile (their D columns are never stored), so no load is conditional
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
    const unsigned* xsrow;
    {
        const int row = tid < TM ? tid : TM - 1;          // (threads past the tile fetch its last row's scales and drop them)
        const int r = r0 + row, rr = r < m_e ? r : r0;
        const size_t src_row = IS_G1 ? (size_t)(p.sorted_slot[off_e + rr] / p.top_k) : (size_t)(off_e + rr);
        xsrow = (const unsigned*)p.xscale + src_row * p.ld_xscale;
    }

    f32x4 acc[NTT][TBW];
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int b = 0; b < TBW; ++b) acc[t][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the loop is specialised on the number of 16-token blocks that hold rows (workgroup-uniform, chosen once)
    auto run = [&](auto NBC) __attribute__((always_inline)) {
        constexpr int NB = decltype(NBC)::v;
        u32x4 ws[2][NTT];
        u32x4 xs[PIECES];
        unsigned xsv = 0;
        int wsc[NTT], wsc_next[NTT];
        auto load_x = [&](int u) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) xs[q] = *(const u32x4*)(xrow[q] + (size_t)u * ROWB);
            xsv = xsrow[u];
        };
        auto load_w = [&](u32x4 (&s)[NTT], int u) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < NTT; ++t) {
                const u32x4* a = wp[t] + (size_t)u * 64;
                s[t] = NTL ? __builtin_nontemporal_load(a) : *a;
            }
        };
        auto store_x = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < PIECES; ++q) *(u32x4*)(xlds + buf * BUFB + xdst[q]) = xs[q];
            *(unsigned*)(xlds + buf * BUFB + TM * ROWB + tid * 4) = xsv;
        };
        auto compute = [&](const u32x4 (&s)[NTT], int buf, auto JC) __attribute__((always_inline)) {
            constexpr int J = decltype(JC)::v;
            const char* xb = xlds + buf * BUFB;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int row = b * 16 + j, sw = x_swizzle<ROWB>(row);
                const u32x4 lo = *(const u32x4*)(xb + row * ROWB + ((g ^ sw) * 16));           // k = 16 g .. + 15
                const u32x4 hi = *(const u32x4*)(xb + row * ROWB + (((4 + g) ^ sw) * 16));     // k = 64 + 16 g .. + 15
                const int sx = *(const unsigned char*)(xb + TM * ROWB + row * 4 + g);
#pragma unroll
                for (int t = 0; t < NTT; ++t) acc[t][b] = mfma_mx<J>(s[t], lo, hi, acc[t][b], wsc[t], sx);
            }
        };
        if (u0 >= u1) return;
        const int ulast = u1 - 1, qlast = q1 - 1;
        load_x(u0);
        load_w(ws[0], u0);
#pragma unroll
        for (int t = 0; t < NTT; ++t) wsc[t] = sp[t][(size_t)q0 * 64];
        store_x(0);
        __syncthreads();
        // one unit: the look-ahead loads (clamped to the K range, so unconditional), the MFMAs, the LDS hand-over
        auto unit = [&](int uu, auto JC) __attribute__((always_inline)) {
            constexpr int J = decltype(JC)::v;
            const int un = uu + 1 < ulast ? uu + 1 : ulast;
            load_x(un);
            load_w(ws[(J + 1) & 1], un);
            __builtin_amdgcn_sched_barrier(0);            // loads are issued before the MFMAs
            compute(ws[J & 1], J & 1, JC);
            __builtin_amdgcn_sched_barrier(0);            // ... and the MFMAs before the hand-over (the scheduler otherwise sinks
            store_x((J + 1) & 1);                         //     four units of them behind the last barrier of the group)
            __syncthreads();
        };
        int q = q0;
        for (; q < qlast; ++q) {                          // steady: whole groups, look-ahead inside the range
#pragma unroll
            for (int t = 0; t < NTT; ++t) wsc_next[t] = sp[t][(size_t)(q + 1) * 64];
            static_for<4>([&](auto JC) __attribute__((always_inline)) { unit(q * 4 + decltype(JC)::v, JC); });
#pragma unroll
            for (int t = 0; t < NTT; ++t) wsc[t] = wsc_next[t];
        }
        static_for<4>([&](auto JC) __attribute__((always_inline)) {      // drain: the last group may hold fewer than four units
            const int uu = q * 4 + decltype(JC)::v;
            if (uu < u1) unit(uu, JC);
        });
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
static int launch_mxa8_t(hipStream_t st, const GemmParams& p, int max_tiles) {
    constexpr size_t lds = (size_t)2 * (TBW * 16 * 128 + 256 * 4);
    dim3 grid(p.T_half / 4, max_tiles, IS_G1 ? 1 : p.SK), block(256);
    auto kern = p.stream_nt ? gemm_mxa8_kernel<ADT, GATED, IS_G1, TBW, true> : gemm_mxa8_kernel<ADT, GATED, IS_G1, TBW, false>;
    if (lds > 64 * 1024) LKM_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    LKM_LAUNCH_GEMM(kern, grid, block, lds, st, p);
    LKM_HIP_CHECK(hipGetLastError());
    return LKM_OK;
}

template <int ADT, bool GATED, bool IS_G1>
static int launch_mxa8(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {
    LKM_REQUIRE(p.T_half % 4 == 0 && p.SK >= 1 && p.SK <= (p.U + 3) / 4, "gemm_mxa8: T_half=%d SK=%d U=%d", p.T_half, p.SK, p.U);
    switch (cfg.tiled) {
    case 32: return launch_mxa8_t<ADT, GATED, IS_G1, 2>(st, p, max_tiles);
    case 64: return launch_mxa8_t<ADT, GATED, IS_G1, 4>(st, p, max_tiles);
    case 128: return launch_mxa8_t<ADT, GATED, IS_G1, 8>(st, p, max_tiles);
    case 256: return launch_mxa8_t<ADT, GATED, IS_G1, 16>(st, p, max_tiles);
    }
    set_error("gemm_mxa8: token-tile height %d not built (32, 64, 128, 256)", cfg.tiled);
    return LKM_E_INVALID;
}

#define LKM_DEFINE_MXA8_LAUNCHERS(SUFFIX, ADT)                                                                               \
    int launch_gemm1_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, bool gated, int max_tiles) {  \
        return gated ? launch_mxa8<ADT, true, true>(st, cfg, p, max_tiles) : launch_mxa8<ADT, false, true>(st, cfg, p, max_tiles); \
    }                                                                                                                        \
    int launch_gemm2_tiled_##SUFFIX(hipStream_t st, const LaunchCfg& cfg, const GemmParams& p, int max_tiles) {              \
        return launch_mxa8<ADT, false, false>(st, cfg, p, max_tiles);                                                        \
    }

}  // namespace lkm
