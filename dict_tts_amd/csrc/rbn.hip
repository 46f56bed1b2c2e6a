// Fused HifiGAN ResBlock1 (modules/hifigan/hifigan.py:27-58) at C = 16 / 8 channels: the last two stages of the V2 generators
// (upsample_initial_channel 128).  One launch per ResBlock, the contract of rblock.hip (RBlockParams): fp32 x in, the stage sum out.
//
// At these widths 32 output channels do not exist, so the TAPS go into the contraction index: v_mfma_f32_16x16x32,
//   D[co 16][t 16] += W[co][k 32] * X[k 32][t],   k = (tap within the k-step) * C + ci,
// two taps x 16 channels per MFMA at C = 16, four taps x 8 channels at C = 8 (where output rows 8 .. 15 of every MFMA are idle: the
// stage is bound by its bytes, not by the matrix pipe).  Lane l holds B[k = 8 (l >> 4) + j][column l & 15]: the activation fragment of a
// lane is ONE 16-byte read — 8 consecutive channels of row t + (tap - (K - 1) / 2) * dil, the tap (and at C = 16 the channel half) chosen
// by l >> 4 — a dilated, row-shifted window of the one 16-bit LDS tile.  Taps are zero padded to whole k-steps (rbn_padded_taps).
//   * the fp32 residual stream lives in registers in accumulator layout (lane = 4 consecutive channels of one row) for all three iterations;
//     in that layout a wave's 16-byte accesses to [T][C] fp32 tensors cover 16 whole consecutive rows: x, the stage sum and the outputs move
//     straight between HBM and registers, no LDS transposition;
//   * all six packs of the ResBlock (<= 36 KB at C = 16, <= 9 KB at C = 8) are copied to LDS once per persistent workgroup;
//   * rounding points are rblock's: weights rounded at pack time, operands through act4<EL>, bias as the accumulator's initial value,
//     stage sum and / num_kernels in fp32;
//   * every tile size sums a layer's contraction in the same order (k-steps in order, one MFMA each): an utterance alone is bit-identical to
//     the same utterance inside any batch.
#include "rbn.h"
#include "rb_common.h"
#include "rb_tiles.h"
#include "../../include/dicttts_hip.h"

#include <algorithm>

namespace dtts {

template <int EL>
__device__ __forceinline__ f32x4 rbn_mfma(const uint4& a, const uint4& b, const f32x4& c) {
    if constexpr (EL == EL_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// WT waves over time, MT 16-row tiles per wave: W = 16 MT WT rows per tile
template <int C, int MT, int WT, int EL, bool GUARD>
__global__ __launch_bounds__(64 * WT) void rbn_kernel(const RBnParams p) {
    static_assert(C == 16 || C == 8, "the tap-folded contraction is written for 16 and 8 channels");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    constexpr int THREADS = 64 * WT;
    constexpr int W = 16 * MT * WT;
    constexpr int PITCH = C * 2;                    // bytes of a 16-bit activation row
    constexpr int TPS = 32 / C;                     // taps per k-step
    constexpr int PK = 7, PH = (PK - 1) / 2;        // the fused conv_post
    constexpr int OOB = (int)0x80000000;            // a buffer offset past every resource: loads return zero, stores are dropped

    const int tid = threadIdx.x, lane = tid & 63, wt = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;       // accumulator layout: time row fr of a 16-row tile, channels 4 fq .. 4 fq + 3
    const bool active = 4 * fq < C;                 // (C = 8: the upper half of the MFMA's output rows is idle)
    const int K = p.K, NS = p.Kp / TPS;             // k-steps per convolution
    const int H = p.halo, G = p.guard;
    const int TT = W - 2 * H;
    const int TTo = p.wav ? TT - 2 * PH : TT;       // tiles step by the samples they output, and start PH rows early

    uint4* wl = (uint4*)smem;                                          // [conv 6][k-step][lane]
    char* act = smem + (size_t)6 * NS * 1024;                          // 16-bit activation tile, G zero rows on both sides
    char* otile = act + (size_t)(W + 2 * G) * PITCH;                   // fused conv_post: the fp32 stage output [TT][C]
    const RbTiles tiles{(int*)(smem + p.pre_off), p.B};

    // ---- once per workgroup: the packs, the guard bands, the tile table (rb_tiles.h: RbTiles)
    for (int c = 0; c < 6; ++c) {
        const uint4* src = (c & 1) ? p.w2[c >> 1] : p.w1[c >> 1];
        for (int i = tid; i < NS * 64; i += THREADS) wl[c * NS * 64 + i] = src[i];
    }
    for (int idx = tid; idx < 2 * G * (PITCH / 16); idx += THREADS) {
        const int r = idx / (PITCH / 16), c = idx % (PITCH / 16);
        *(uint4*)(act + (r < G ? r : W + r) * PITCH + c * 16) = make_uint4(0, 0, 0, 0);
    }
    tiles.build(p.lens, p.T, TTo, tid, THREADS);
    const int total = tiles.total();
    int j = blockIdx.x;
    if (j >= total) return;
    const int Gd = gridDim.x;

    // this lane's 16 bytes of local row `row` of a [len][C] fp32 tensor whose local row 0 is global row base: byte offset into the utterance's
    // buffer resource.  Rows before the utterance wrap to a huge unsigned offset, rows behind it exceed the resource: zeros / dropped.
    auto goff = [&](int base, int row) { return active ? ((base + row) * C + 4 * fq) * 4 : OOB; };
    auto load_x = [&](f32x4& d, int m, int bb, int base, int ln) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (long long)bb * p.T * C), 0, ln * C * 4, 0x00020000);
        d = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, goff(base, (wt * MT + m) * 16 + fr), 0, RB_X_AUX));
    };

    int b = 0;
    tiles.locate(j, b);
    int len = tiles.len_of(b);
    int t0 = tiles.first_row(j, b, TTo) - (p.wav ? PH : 0);
    f32x4 xr[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) load_x(xr[m], m, b, t0 - H, len);

    // B-operand fragment of this lane: tap tl of the k-step, channels ci0 .. ci0 + 7
    const int tl = C == 16 ? fq >> 1 : fq, ci0 = C == 16 ? 8 * (fq & 1) : 0;
    const int pad = (K - 1) / 2;
    int n_ovf = 0;

#pragma unroll 1
    for (;;) {
        t0 = __builtin_amdgcn_readfirstlane(t0);
        const int base_t = t0 - H;                  // global time of local row 0
        const long long brow = (long long)b * p.T;
        // the workgroup's next tile: static (j + Gd), or the next unclaimed tile of the launch from a device counter (rb_tiles.h): one lane issues
        // the atomic here, its result is broadcast through LDS behind the last contraction's barrier
        unsigned claim = 0;
        if (p.tile_ctr && tid == 0) claim = atomicAdd(p.tile_ctr, 1u);
        const bool all_inb = base_t >= 0 && base_t + W <= len;
        const int c_lo = H + (p.wav ? PH : 0), c_hi = c_lo + TTo;   // the rows the census counts

        // 16-bit leaky_relu(v, 0.1) of this wave's rows -> the LDS tile, zero outside the utterance (= the reference's zero padding)
        auto write_act = [&](const f32x4 (&v)[MT]) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int row = (wt * MT + m) * 16 + fr, t = base_t + row;
                const bool inb = all_inb || (t >= 0 && t < len);
                uint2 pk = act4<EL>(v[m], 0.1f);
                // range guard: a census — every in-utterance row is counted by exactly ONE tile.  With the fused conv_post the tiles overlap by 2 PH rows:
                // rows [H + PH, H + PH + TTo) are the ones a tile steps by, whatever the tile size
                if constexpr (GUARD) n_ovf += (active && inb && row >= c_lo && row < c_hi) ? ovf4(v[m], 0.1f) : 0;
                if (!inb) pk = make_uint2(0, 0);
                if (active) *(uint2*)(act + (G + row) * PITCH + fq * 8) = pk;
            }
        };
        // acc += W[conv] * act with dilation d: k-steps in order, the weight fragment of a step read once for the wave's MT row tiles
        auto contract = [&](f32x4 (&acc)[MT], int conv, int d) {
            const char* xb = act + (G + wt * MT * 16 + fr + (tl - pad) * d) * PITCH + ci0 * 2;
            const uint4* wf = wl + conv * NS * 64 + lane;
            const int step = TPS * d * PITCH;
#pragma unroll 1
            for (int s = 0; s < NS; ++s) {
                const uint4 a = wf[s * 64];
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = rbn_mfma<EL>(a, *(const uint4*)(xb + m * 16 * PITCH), acc[m]);
                xb += step;
            }
        };

        write_act(xr);
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < 3; ++it) {
            const f32x4 bias1 = *(const f32x4*)(p.b1[it] + 4 * fq), bias2 = *(const f32x4*)(p.b2[it] + 4 * fq);
            f32x4 acc[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = bias1;   // the bias is the accumulator's initial value
            contract(acc, 2 * it, p.dil[it]);
            __syncthreads();                               // every wave is done reading leaky_relu(x)
            write_act(acc);                                // xt overwrites it
            __syncthreads();
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) xr[m][e] += bias2[e];
            contract(xr, 2 * it + 1, 1);                   // x = x + b2 + W2 * xt, straight into the residual registers
            if (it == 2 && p.tile_ctr && tid == 0) tiles.publish_claim(Gd, claim);
            __syncthreads();                               // every wave is done reading xt
            if (it < 2) {
                write_act(xr);
                __syncthreads();
            }
        }

        int jn = p.tile_ctr ? tiles.claimed() : j + Gd;
        const bool has_next = jn < total;
        int bn = b, lenn = len, t0n = 0;
        if (has_next) {
            tiles.locate(jn, bn);
            lenn = tiles.len_of(bn);
            t0n = tiles.first_row(jn, bn, TTo) - (p.wav ? PH : 0);
        }

        // ---- epilogue: rows [H, H + TT) of the tile leave straight from the accumulator layout (a wave's access = 16 whole consecutive rows)
        {
            const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)(p.S + brow * C), 0, len * C * 4, 0x00020000);
            const auto rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Sa ? p.Sa + brow * C : (unsigned short*)(p.S + brow * C)), 0, len * C * 2, 0x00020000);
            auto eoff = [&](int m) {
                const int row = (wt * MT + m) * 16 + fr;
                return (row >= H && row < H + TT) ? goff(base_t, row) : OOB;
            };
            u32x4 sold[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                sold[m] = u32x4{0u, 0u, 0u, 0u};
                if (p.mode >= 1) sold[m] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, eoff(m), 0, VP_LD_AUX);
            }
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int off = eoff(m);
                f32x4 o = xr[m] + __builtin_bit_cast(f32x4, sold[m]);   // xs += resblock(x)  (hifigan.py:133-135); zeros in mode 0
                // slab m of the residual registers is free: the next tile's slab m starts its trip into them
                if (has_next) load_x(xr[m], m, bn, t0n - H, lenn);
                if (p.wav) {
                    const int row = (wt * MT + m) * 16 + fr, t = base_t + row;
                    if (active && row >= H && row < H + TT) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (t >= 0 && t < len) ? lrelu(o[e] / p.div, p.slope) : 0.f;
                        *(f32x4*)(otile + (size_t)(row - H) * (C * 4) + fq * 16) = o;
                    }
                    continue;
                }
                rb_stage_row(o, rs_s, rs_a, off, p.mode, p.div, p.slope, p.drop_S != 0, p.Sa != nullptr, false);
            }
        }
        if (p.wav) {
            // ---- wav[t] = tanh(b + sum_{tap, c} w[c][tap] * otile[t + tap - 3][c])  (conv_post + tanh, hifigan.py:139-141) in exact fp32:
            // rb_tiles.h's rb_conv_post_tanh with one sample per group, kept as a LOCAL copy: called as the shared function (PR = 1) it is bit-identical, but
            // hipcc then keeps what it derives from the thread index alive through the contractions (1 - 2 VGPRs more, the C = 8 census kernel of the 512-row
            // tile falls to two waves per SIMD), and with an opaque move of the index in front of the call the V2 forward measured 2 % slower (LABNOTES).
            // C / 4 lanes per sample (4 channels each, 7 taps in order), partial sums joined by xor-shuffles: the same rounding sequence for
            // every sample, whatever its place in a tile
            __syncthreads();
            constexpr int LPO = C / 4;
            const int q = tid % LPO, rr = tid / LPO;
            f32x4 wq[PK];
#pragma unroll
            for (int k = 0; k < PK; ++k) wq[k] = *(const f32x4*)(p.post_w + k * C + q * 4);
            const float pb = p.post_b[0];
            float* wb = p.wav + brow;
            for (int o0 = 0; o0 < TTo; o0 += THREADS / LPO) {
                const int o = o0 + rr;
                float a = 0.f;
                if (o < TTo) {
#pragma unroll
                    for (int k = 0; k < PK; ++k) {
                        const f32x4 v = *(const f32x4*)(otile + (size_t)(o + k) * (C * 4) + q * 16);
                        const float d = __builtin_fmaf(v[3], wq[k][3], __builtin_fmaf(v[2], wq[k][2], __builtin_fmaf(v[1], wq[k][1], __fmul_rn(v[0], wq[k][0]))));
                        a = __fadd_rn(a, d);
                    }
                }
                a += __shfl_xor(a, 1, 64);
                if constexpr (LPO == 4) a += __shfl_xor(a, 2, 64);
                // the always-on overflow detector and the tanh of rb_tiles.h's rb_conv_post_tanh, operation for operation: a non-finite pre-tanh value is
                // poisoned with NaN and counted
                const float prv = a + pb;
                const float th = __builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(__fadd_rn(__builtin_amdgcn_exp2f(prv * 2.885390081777927f), 1.f)), 1.f);
                const int t = t0 + PH + o;
                if (q == 0 && o < TTo && t < len) {
                    const bool nonfin = !(__builtin_fabsf(prv) <= 3.0e38f);
                    wb[t] = nonfin ? __builtin_nanf("") : th;
                    if (nonfin && p.bad) atomicAdd(p.bad, 1u);   // (never on a healthy call)
                }
            }
        }
        if (!has_next) break;
        j = jn;
        b = bn;
        len = lenn;
        t0 = t0n;
    }
    if constexpr (GUARD) {
        if (n_ovf) atomicAdd(p.ovf, (unsigned long long)n_ovf);
    }
}

bool rbn_supported(int C, int K, int d0, int d1, int d2) {
    if (C != 16 && C != 8) return false;
    if (!(K & 1) || K < 3 || K > 11 || d0 < 1 || d1 < 1 || d2 < 1) return false;
    const int dil[3] = {d0, d1, d2};
    const int halo = rblock_halo_of(K, dil), W = RBN_ROWS[2];
    if (W - 2 * halo - 6 < 32) return false;
    return rbn_lds_bytes(C, W, rbn_padded_taps(C, K), halo, rbn_guard(C, K, dil), true) + rb_table_bytes(DTTS_MAX_VOCODER_BATCH) <= 160 * 1024;
}

// hipErrorOutOfMemory: the tile does not fit (its LDS with the tile table of p.B utterances exceeds 160 KB, or fewer than 32 rows are left): the caller
// takes the next smaller one
template <int C, int MT, int WT, int EL, bool GUARD = false>
static hipError_t rbn_launch_cfg(const RBnParams& p, hipStream_t stream) {
    constexpr int W = 16 * MT * WT, THREADS = 64 * WT;
    const int TT = W - 2 * p.halo, TTo = p.wav ? TT - 6 : TT;
    if (TTo < 32) return hipErrorOutOfMemory;
    size_t lds = rbn_lds_bytes(C, W, p.Kp, p.halo, p.guard, p.wav != nullptr);
    RBnParams q = p;
    q.pre_off = (int)lds;
    lds += rb_table_bytes(p.B);
    if (lds > 160 * 1024) return hipErrorOutOfMemory;
    if constexpr (EL == EL_F16 && !GUARD) {
        if (p.ovf) return rbn_launch_cfg<C, MT, WT, EL, true>(p, stream);
    }
    constexpr auto kern = rbn_kernel<C, MT, WT, EL, GUARD>;
    if (const hipError_t e = rb_allow_full_lds<kern>(); e != hipSuccess) return e;
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    // resident workgroups by registers: the 1024-row kernels take 175 - 182 VGPRs (one 8-wave workgroup per CU), the 4-wave ones 2 - 4 per CU
    int by_regs = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&by_regs, (const void*)kern, THREADS, lds) != hipSuccess || by_regs < 1) by_regs = 1;
    const int grid = rb_resident_grid(cus, lds, THREADS, by_regs, (long long)p.B * ((p.T + TTo - 1) / TTo));
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), lds, stream, q);
    return hipGetLastError();
}

// The tile rule (tests/rbn_shapes.py restates it): 1024-row tiles; while they would leave more than half of the CUs without one (small batches: the launch
// takes as long as ONE tile) 512-row tiles, and 256-row tiles while those still do.  A tile that does not fit falls through to the next smaller one.
template <int C, int EL>
static hipError_t rbn_launch_el(const RBnParams& p, hipStream_t stream) {
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    auto few = [&](int W) {
        const int tt = W - 2 * p.halo - (p.wav ? 6 : 0);
        return tt >= 32 && 2 * (long long)p.B * ((p.T + tt - 1) / tt) <= cus;
    };
    const int first = few(RBN_ROWS[0]) ? (few(RBN_ROWS[1]) ? 2 : 1) : 0;
    hipError_t e = hipErrorOutOfMemory;
    if (first <= 0 && e == hipErrorOutOfMemory) e = rbn_launch_cfg<C, 8, 8, EL>(p, stream);
    if (first <= 1 && e == hipErrorOutOfMemory) e = rbn_launch_cfg<C, 8, 4, EL>(p, stream);
    if (e == hipErrorOutOfMemory) e = rbn_launch_cfg<C, 4, 4, EL>(p, stream);
    return e == hipErrorOutOfMemory ? hipErrorInvalidValue : e;
}

hipError_t rbn_launch(const RBnParams& p, int C, int frag, hipStream_t stream) {
    if (frag != RBN_FRAG) return hipErrorInvalidValue;   // the kernel walks a pack in its own order or not at all
    if (!rbn_supported(C, p.K, p.dil[0], p.dil[1], p.dil[2]) || p.Kp != rbn_padded_taps(C, p.K)) return hipErrorInvalidValue;
    // 32-bit byte offsets inside an utterance's buffer resource: a tile's local rows reach up to RBN_ROWS[0] rows past the utterance's end
    if (((long long)p.T + RBN_ROWS[0]) * C * 4 >= (1LL << 31)) return hipErrorInvalidValue;
    if (p.wav && (p.mode != 2 || !p.post_w || !p.post_b)) return hipErrorInvalidValue;
    if (p.B < 1 || p.B > DTTS_MAX_VOCODER_BATCH) return hipErrorInvalidValue;
    RBnParams q = p;
    q.halo = rblock_halo_of(p.K, p.dil);
    q.guard = rbn_guard(C, p.K, p.dil);
    if (C == 16) return p.el == EL_F16 ? rbn_launch_el<16, EL_F16>(q, stream) : rbn_launch_el<16, EL_BF16>(q, stream);
    return p.el == EL_F16 ? rbn_launch_el<8, EL_F16>(q, stream) : rbn_launch_el<8, EL_BF16>(q, stream);
}

} // namespace dtts
