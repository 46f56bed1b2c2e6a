// Grouped channels-last 1-D convolution (k = 41, pad 20, stride 1 / 2 / 4) on the fp32 matrix cores: the MultiScaleDiscriminator's five
// grouped layers (disc.h).  One workgroup = one tile of output rows of ONE group of one sequence.
//   * The group's input channels are contiguous in the channels-last row; the staged span is (rows - 1) * stride + 41 input rows of those
//     cig channels, leaky_relu applied on the way in, rows outside [0, in_len) zero.
//   * The contraction index runs over (tap, channel in group): kk = tap * cig + ci, 41 * cig values, so the taps fill the MFMA's k where the
//     group is narrow (cig = 8).  Output row i reads the span at row i * stride + tap, column ci: one ds_read_b128 gives a lane the four
//     consecutive kk of its k-half, spent on four v_mfma_f32_32x32x2_f32 (A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; the weights
//     are packed with the same permutation: disc.h).  Products are exact fp32, one fp32 accumulation chain per output in kk order.
//   * LDS row pitch cig + 4 floats: 16 B aligned, and it moves consecutive output rows (stride * pitch floats apart) off a common bank.
//   * cog = 64: 2 row tiles x 2 co-tiles per workgroup (64 rows); cog <= 32: 4 row tiles (128 rows); cog = 16 computes on a half-empty
//     co-tile (its layer is 11 % of the grouped work).
#include "disc.h"

namespace dtts {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <int WT>
__global__ __launch_bounds__(256) void gconv_kernel(const GConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float glds[];
    constexpr int TR = 32 * WT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wt = wave % WT, wc = wave / WT;
    const int seq = blockIdx.z, g = blockIdx.y, t0 = blockIdx.x * TR;
    const int in_len = p.in_lens[seq], out_len = p.out_lens[seq];
    if (t0 >= out_len) return;
    const int cig = p.cig, pitch = cig + 4;
    const int span = (TR - 1) * p.stride + GCONV_K;
    const int in0 = t0 * p.stride - GCONV_PAD;
    const float* xb = p.x + (size_t)seq * p.T_in * p.C_in + (size_t)g * cig;
    const int pieces = cig >> 2;
    for (int idx = tid; idx < span * pieces; idx += 256) {
        const int r = idx / pieces, c4 = idx - r * pieces;
        const int t = in0 + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < in_len) {
            v = *(const f32x4*)(xb + (size_t)t * p.C_in + c4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        }
        *(f32x4*)(glds + r * pitch + c4 * 4) = v;
    }
    __syncthreads();

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int hh = lane >> 5;
    const int rowbase = (wt * 32 + (lane & 31)) * p.stride;
    const f32x4* w = (const f32x4*)p.w + (size_t)(g * p.ntg + wc) * p.nq * 64 + lane;
#pragma unroll 2
    for (int Q = 0; Q < p.nq; ++Q) {
        const int kk = 8 * Q + 4 * hh;
        const int tap = kk >> p.cig_shift, ci = kk & (cig - 1);
        const f32x4 a = *(const f32x4*)(glds + (rowbase + tap) * pitch + ci);
        const f32x4 b = w[(size_t)Q * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
    }

    const int cg = wc * 32 + (lane & 31);
    if (cg >= p.cog) return;
    const int co = g * p.cog + cg;
    const float bias = p.bias[co];
    float* yb = p.y + (size_t)seq * p.T_out * p.C_out + co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + wt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        if (t < out_len) yb[(size_t)t * p.C_out] = acc[r] + bias;
    }
}

hipError_t gconv_launch(const GConvParams& p, hipStream_t stream) {
    if (p.nseq < 1 || p.nseq > 65535 || p.T_in < 1 || p.T_out < 1 || p.cig < 8 || (p.cig & (p.cig - 1)) || (1 << p.cig_shift) != p.cig || p.cog < 1 ||
        p.cog > 64 || p.ntg != (p.cog + 31) / 32 || p.nq * 8 != GCONV_K * p.cig || p.C_in % p.cig || p.C_in / p.cig > 65535 ||
        p.C_in / p.cig * p.cog != p.C_out || !p.in_lens || !p.out_lens)
        return hipErrorInvalidValue;
    const size_t lds = gconv_lds_bytes(p.cig, p.cog, p.stride);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const int tr = gconv_tile_rows(p.cog);
    const dim3 grid((unsigned)((p.T_out + tr - 1) / tr), (unsigned)(p.C_in / p.cig), (unsigned)p.nseq);
    if (gconv_wide(p.cog)) hipLaunchKernelGGL(gconv_kernel<2>, grid, dim3(256), lds, stream, p);
    else hipLaunchKernelGGL(gconv_kernel<4>, grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

} // namespace dtts
