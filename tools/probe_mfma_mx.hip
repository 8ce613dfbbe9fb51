// probe_mfma_mx.hip -- stand-alone MI355X probe: operand and scale-lane layout of v_mfma_scale_f32_16x16x128_f8f6f4 with an fp4 A
// operand (cbsz 4) against an fp8 e4m3 B operand (blgp 0), the mix gemm_mxa8.h runs, and against an fp4 B operand (blgp 4, 16 bytes
// per lane in the low four dwords), the mix gemm_mxa4.h runs.  One wavefront; prints
//   * for every A position (lane group g, nibble n) the B position (lane group g', byte n') it is multiplied with,
//   * the result with the scale doubled in one lane group at a time, for data in one lane group at a time (A and B side),
//   * which byte of the scale register each op_sel value selects,
//   * the same three for the fp4 B operand: (group, nibble) pairs, the B scale-lane table, op_sel of the B scale register.
// Build: hipcc --offload-arch=gfx950 -O2 tools/probe_mfma_mx.hip -o probe_mfma_mx
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <int OA>
__device__ float mx(const i32x8& a, const i32x8& b, int sa, int sb) {
    const f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0.f, 0.f, 0.f, 0.f}, 4, 0, OA, sa, 0, sb);
    float r = d[0];   // lane 0: D[row 0][token 0]
    asm volatile("" : "+v"(r));      // (keeps the MFMA out of the `lane == 0` blocks below: it needs the whole wavefront)
    return r;
}

template <int OB>
__device__ float mx4(const i32x8& a, const i32x8& b, int sa, int sb) {       // fp4 x fp4
    const f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0.f, 0.f, 0.f, 0.f}, 4, 4, 0, sa, OB, sb);
    float r = d[0];
    asm volatile("" : "+v"(r));
    return r;
}

// out[0..127]: B position of A position p; then floats: [136..139] op_sel 0..3, [140..155] / [156..171] the scale-lane tables of A / B
// fp4 B: out[172..299] B nibble position of A position p; floats [300..315] the B scale-lane table, [316..319] op_sel 0..3 of sb
__global__ void probe(int* out) {
    const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
    float* fout = (float*)out;
    for (int pa = 0; pa < 128; ++pa) {
        i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i == 0 && g == pa / 32) a[(pa % 32) / 8] = 0x2 << (4 * (pa % 8));          // E2M1 1.0 in nibble pa % 32 of row 0
        int found = -1;
        for (int pb = 0; pb < 128; ++pb) {
            i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
            if (i == 0 && g == pb / 32) b[(pb % 32) / 4] = 0x38 << (8 * (pb % 4));      // e4m3 1.0 in byte pb % 32 of token 0
            const float d = mx<0>(a, b, 127, 127);
            if (d != 0.f) found = pb;
        }
        if (lane == 0) out[pa] = found;
    }
    const i32x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const i32x8 ones_a = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    const i32x8 ones_b = {0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838, 0x38383838};
    for (int gd = 0; gd < 4; ++gd) {                      // data only in lane group gd; scale 2.0 only in lane group gs
        const i32x8 a = g == gd ? ones_a : zero, b = g == gd ? ones_b : zero;
        for (int gs = 0; gs < 4; ++gs) {                  // 32 products of 1.0: 32 without, 64 with the doubled scale
            const float da = mx<0>(a, ones_b, g == gs ? 128 : 127, 127);
            const float db = mx<0>(ones_a, b, 127, g == gs ? 128 : 127);
            if (lane == 0) { fout[140 + gd * 4 + gs] = da; fout[156 + gd * 4 + gs] = db; }
        }
    }
    const int sc = 127 | (128 << 8) | (129 << 16) | (130 << 24);
    const float d0 = mx<0>(ones_a, ones_b, sc, 127), d1 = mx<1>(ones_a, ones_b, sc, 127), d2 = mx<2>(ones_a, ones_b, sc, 127),
                d3 = mx<3>(ones_a, ones_b, sc, 127);
    if (lane == 0) {
        fout[136] = d0; fout[137] = d1; fout[138] = d2; fout[139] = d3;      // 128 products: 128 x 2^(byte - 127)
    }
    for (int pa = 0; pa < 128; ++pa) {                    // the fp4 B operand: the same three measurements
        i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i == 0 && g == pa / 32) a[(pa % 32) / 8] = 0x2 << (4 * (pa % 8));
        int found = -1;
        for (int pb = 0; pb < 128; ++pb) {
            i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
            if (i == 0 && g == pb / 32) b[(pb % 32) / 8] = 0x2 << (4 * (pb % 8));       // E2M1 1.0 in nibble pb % 32 of token 0
            const float d = mx4<0>(a, b, 127, 127);
            if (d != 0.f) found = pb;
        }
        if (lane == 0) out[172 + pa] = found;
    }
    for (int gd = 0; gd < 4; ++gd) {
        const i32x8 b = g == gd ? ones_a : zero;
        for (int gs = 0; gs < 4; ++gs) {
            const float db = mx4<0>(ones_a, b, 127, g == gs ? 128 : 127);
            if (lane == 0) fout[300 + gd * 4 + gs] = db;
        }
    }
    const float e0 = mx4<0>(ones_a, ones_a, 127, sc), e1 = mx4<1>(ones_a, ones_a, 127, sc), e2 = mx4<2>(ones_a, ones_a, 127, sc),
                e3 = mx4<3>(ones_a, ones_a, 127, sc);
    if (lane == 0) {
        fout[316] = e0; fout[317] = e1; fout[318] = e2; fout[319] = e3;
    }
}

int main() {
    int* d = nullptr;
    int h[320];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 1;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err != hipSuccess || hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "probe_mfma_mx: kernel did not complete: %s\n", hipGetErrorString(err));
        return 1;
    }
    printf("A (group, nibble) -> B (group, byte):\n");
    for (int p = 0; p < 128; ++p) printf("(%d,%2d)->(%d,%2d)%s", p / 32, p % 32, h[p] / 32, h[p] % 32, p % 8 == 7 ? "\n" : " ");
    const float* f = (const float*)h;
    for (int side = 0; side < 2; ++side)
        for (int gd = 0; gd < 4; ++gd) {
            printf("%c data in lane group %d, scale 2.0 in lane group 0..3:", side ? 'B' : 'A', gd);
            for (int gs = 0; gs < 4; ++gs) printf(" %g", f[140 + side * 16 + gd * 4 + gs]);
            printf("\n");
        }
    printf("scale register bytes 1, 2, 4, 8 (x 128 products), op_sel 0..3: %g %g %g %g\n", f[136], f[137], f[138], f[139]);
    printf("fp4 B operand.  A (group, nibble) -> B (group, nibble):\n");
    for (int p = 0; p < 128; ++p) printf("(%d,%2d)->(%d,%2d)%s", p / 32, p % 32, h[172 + p] / 32, h[172 + p] % 32, p % 8 == 7 ? "\n" : " ");
    for (int gd = 0; gd < 4; ++gd) {
        printf("fp4 B data in lane group %d, scale 2.0 in lane group 0..3:", gd);
        for (int gs = 0; gs < 4; ++gs) printf(" %g", f[300 + gd * 4 + gs]);
        printf("\n");
    }
    printf("fp4 B scale register bytes 1, 2, 4, 8 (x 128 products), op_sel 0..3: %g %g %g %g\n", f[316], f[317], f[318], f[319]);
    (void)hipFree(d);
    return 0;
}
