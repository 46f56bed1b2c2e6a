// Micro-benchmark: what does the MFMA pipe sustain on THIS chip with real operand data, and does the MFMA SHAPE matter?
// Loops of independent v_mfma_f32_32x32x16_{f16,bf16} or v_mfma_f32_16x16x32_{f16,bf16} over the same 128 x 64 output tile per wave,
// 2 waves per SIMD (32x32x16: also 3), in two forms:
//   reg: operands stay in registers (no memory traffic);
//   lds: both operands are re-read from LDS by ds_read_b128 every k-step, at the fused vocoder kernels' fragment pattern (rows at an
//        odd number of 16-byte slots; a lane reads 16 bytes of row lane & 31 [lane & 15] at byte 16 * (lane >> 5) [16 * (lane >> 4)]).
// with (a) all-zero operands and (b, c) random operands of the magnitudes the vocoder sees.  Prints TFLOP/s and, from the wall time, the
// fraction of the 2.5 PFLOP/s dense peak (MI355X_MICROARCH.md).  Power management lowers the clock when the matrix cores
// toggle real data; this measures the ceiling a data-carrying kernel can reach, next to the spec peak the rooflines quote.
// The 16x16x32 loop holds 48 operand registers beside its 128 accumulators: three of its waves do not fit a SIMD, so it runs at two waves
// per SIMD only; the 32x32x16 loop runs at two and three.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/mfma_peak.hip -o tools/micro/mfma_peak
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int PITCH = 128 * 2 + 16;   // bytes per LDS row: 128 16-bit channels + one 16-byte slot (17 slots: odd)
constexpr int ROWS = 128 + 64;        // A rows, then B rows

template <bool BF>
__device__ __forceinline__ f32x16 mfma32(const uint4& a, const uint4& b, const f32x16& c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <bool BF>
__device__ __forceinline__ f32x4 mfma16(const uint4& a, const uint4& b, const f32x4& c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// SH = 32: 4 x 2 tiles of 32x32, 16 k per iteration; SH = 16: 8 x 4 tiles of 16x16, 32 k per iteration (twice the FLOP of an iteration,
// the same MFMA cycles per FLOP).  LDS: the operand fragments of every iteration come from the LDS tile (the k offset moves with the
// iteration so that the reads stay inside the loop).
template <int SH, bool BF, bool LDS>
__global__ __launch_bounds__(256) void mfma_loop(const uint4* ab, float* out, int iters) {
    __shared__ __attribute__((aligned(16))) char tile[LDS ? ROWS * PITCH : 16];
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr int NA = 128 / SH, NB = 64 / SH, KB = SH == 32 ? 32 : 64;   // fragments per operand; bytes of a k-step in a row
    typedef typename std::conditional<SH == 32, f32x16, f32x4>::type acc_t;
    uint4 a[NA], b[NB];
    if constexpr (LDS) {
        for (int i = tid; i < ROWS * (PITCH / 16); i += 256) ((uint4*)tile)[i] = ab[i % 2048];
        __syncthreads();
    }
    for (int i = 0; i < NA; ++i) a[i] = ab[(i * 256 + tid) % 2048];
    for (int i = 0; i < NB; ++i) b[i] = ab[((NA + i) * 256 + tid) % 2048];
    acc_t acc[NA * NB];
    for (int i = 0; i < NA * NB; ++i)
        for (int r = 0; r < (SH == 32 ? 16 : 4); ++r) acc[i][r] = 0.f;
    const int lrow = SH == 32 ? (lane & 31) * PITCH + (lane >> 5) * 16 : (lane & 15) * PITCH + (lane >> 4) * 16;
    for (int it = 0; it < iters; ++it) {
        if constexpr (LDS) {
            const char* base = tile + lrow + (it & 3) * KB;
#pragma unroll
            for (int i = 0; i < NA; ++i) a[i] = *(const uint4*)(base + i * SH * PITCH);
#pragma unroll
            for (int i = 0; i < NB; ++i) b[i] = *(const uint4*)(base + (128 + i * SH) * PITCH);
        }
#pragma unroll
        for (int i = 0; i < NA * NB; ++i) {
            if constexpr (SH == 32) acc[i] = mfma32<BF>(a[i % NA], b[i / NA], acc[i]);
            else acc[i] = mfma16<BF>(a[i % NA], b[i / NA], acc[i]);
        }
    }
    float s = 0.f;
    for (int i = 0; i < NA * NB; ++i)
        for (int r = 0; r < (SH == 32 ? 16 : 4); ++r) s += acc[i][r];
    if (s == 123.456f) out[0] = s;   // keep the loop alive
}

static unsigned short f2h(float f) { _Float16 h = (_Float16)f; unsigned short u; __builtin_memcpy(&u, &h, 2); return u; }
static unsigned short f2b(float f) { unsigned u; __builtin_memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }

typedef void (*kern_t)(const uint4*, float*, int);

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;   // k-steps of 16 per wave (a 16x16x32 loop runs half as many iterations)
    uint4* dab;
    float* dout;
    if (hipMalloc(&dab, 2048 * 16) != hipSuccess || hipMalloc(&dout, 64) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    // [lds][bf][shape]
    const kern_t kern[2][2][2] = {{{mfma_loop<32, false, false>, mfma_loop<16, false, false>}, {mfma_loop<32, true, false>, mfma_loop<16, true, false>}},
                                  {{mfma_loop<32, false, true>, mfma_loop<16, false, true>}, {mfma_loop<32, true, true>, mfma_loop<16, true, true>}}};
    for (int lds = 0; lds < 2; ++lds)
        for (int bf = 0; bf < 2; ++bf)
            for (int data = 0; data < 3; ++data) {
                std::vector<unsigned short> h(2048 * 8);
                srand(1);
                for (auto& v : h) {
                    float x = data == 0 ? 0.f : (data == 1 ? (rand() / (float)RAND_MAX - 0.5f) * 1e-2f : (rand() / (float)RAND_MAX - 0.5f) * 2.f);
                    v = bf ? f2b(x) : f2h(x);
                }
                if (hipMemcpy(dab, h.data(), h.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
                for (int wg_per_cu = 2; wg_per_cu <= 3; ++wg_per_cu) {
                    const int blocks = 256 * wg_per_cu;
                    double tf[2] = {0, 0};
                    for (int sh = 0; sh < (wg_per_cu == 2 ? 2 : 1); ++sh)   // (three 16x16x32 waves are not resident at once: no such row)
                        for (int rep = 0; rep < 2; ++rep) {
                            hipEventRecord(e0);
                            hipLaunchKernelGGL(kern[lds][bf][sh], dim3(blocks), dim3(256), 0, 0, dab, dout, sh ? iters / 2 : iters);
                            hipEventRecord(e1);
                            if (hipEventSynchronize(e1) != hipSuccess) return 1;
                            float ms;
                            hipEventElapsedTime(&ms, e0, e1);
                            const double flop = (double)blocks * 4 * (iters / 2 * 2) * 8 * 32768.0;
                            tf[sh] = flop / ms / 1e9;
                            if (rep)
                                printf("%s %s %-8s %-18s %d waves/SIMD: %8.2f ms  %7.1f TFLOP/s = %5.1f %% of 2.5 PF\n", lds ? "lds" : "reg", bf ? "bf16" : "f16 ",
                                       sh ? "16x16x32" : "32x32x16", data == 0 ? "all zero" : (data == 1 ? "random |x| < 5e-3" : "random |x| < 1"),
                                       wg_per_cu, ms, tf[sh], tf[sh] / 2500.0 * 100);
                        }
                    if (wg_per_cu == 2) printf("    16x16x32 / 32x32x16 = %.3f\n", tf[1] / tf[0]);
                }
            }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
