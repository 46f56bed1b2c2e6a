// Fused HifiGAN ResBlock2 (modules/hifigan/hifigan.py:67-84), 16-bit MFMA, widths 32 / 64 / 128 / 256:
//     for c, d in zip(convs, (d0, d1)):  x = c(leaky_relu(x, 0.1)) + x          (both convolutions dilated, a residual add after each)
//
// Neither ResBlock1 kernel computes this (vpair: "dilated, then d = 1, then one add"; rblock: three such pairs).  One launch runs the
// whole block on a time tile that stays resident, in the manner of rblock.hip with one convolution per iteration and two iterations:
//   * the fp32 residual stream x lives in REGISTERS in MFMA accumulator layout; each convolution accumulates straight into it
//     (x += b + W * act: no second accumulator set, which is what lets 192-row tiles fit at C = 256),
//   * the 16-bit leaky_relu(x) operand tile lives in ONE LDS buffer: conv d0 reads it -> barrier -> it is rewritten from the UPDATED x
//     -> barrier -> conv d1 reads it (rb_common.h: act4 — leaky_relu in fp16 after the conversion in the f16 mode, in fp32 before it
//     in bf16: the rounding points of ResBlock1),
//   * weights stream from L2 through rb_common.h's register ring,
//   * the tile carries rb2x_halo = (K - 1) / 2 * (d0 + d1) recomputed rows per side; rows outside the utterance are forced to zero in
//     every activation write = the reference's zero padding; the LDS guard bands are rb2x_guard rows (rb2x.h derives both),
//   * persistent workgroups walk the batch's valid tiles (static, or claimed from a device counter); the next tile's x is fetched
//     straight into the residual registers slab by slab as the epilogue releases them.
// A ResBlock2 is the work of one vpair launch, so all four widths fuse whole: no stream between launches exists here.
// HBM traffic per ResBlock: read x once, read-modify-write the stage sum once (the per-convolution path: ~5 passes).
#include "rb2x.h"
#include "rblock.h"
#include "rb_common.h"
#include "rb_tiles.h"
#include "../../include/dicttts_hip.h"

#include <algorithm>
#include <type_traits>

namespace dtts {

template <int C, int MT, int NT, int WT, int WC, int EL, bool GUARD>
__global__ __launch_bounds__(64 * WT * WC, (64 * WT * WC <= 256) ? 2 : 1) void rb2x_kernel(const RB2xParams p) {
    static_assert(WC * NT * 32 == C, "channel tiling must cover C");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int THREADS = 64 * WT * WC;
    constexpr int W = 32 * MT * WT;
    constexpr int PITCH = C * 2 + 16;
    constexpr int NKG = C / 16;
    constexpr bool REAL_STEPS = (NKG < 4);         // C = 32: the real k-steps only (rb2_contract), as rblock.hip
    constexpr int EP = C * 4 + 16;                 // fp32 staging row
    static_assert((size_t)WT * 32 * EP <= (size_t)W * PITCH, "the epilogue's transposition rows lie inside the tile rows");
    const int H = p.halo, GR = p.guard;
    const size_t ACT_BYTES = (size_t)(W + 2 * GR) * PITCH;
    char* act = smem;

    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int wt = wave % WT, wc = wave / WT;
    const int TT = W - 2 * H;
    // fused conv_post (p.wav): the tile's TT valid rows give TT - (PK - 1) output samples, so tiles step by that and start (PK - 1) / 2 rows early
    constexpr int PK = 7, PH = (PK - 1) / 2;
    const int TTo = p.wav ? TT - 2 * PH : TT;

    const RbTiles tiles{(int*)(smem + p.pre_off), p.B};
    // zero the guard bands (once; the fused conv_post's fp32 output tile aliases them: again after every tile there)
    auto zero_guard_bands = [&](int t) {
        for (int idx = t; idx < 2 * GR * (PITCH / 16); idx += THREADS) {
            const int r = idx / (PITCH / 16), c = idx % (PITCH / 16);
            const int row = r < GR ? r : W + r;
            *(uint4*)(act + row * PITCH + c * 16) = make_uint4(0, 0, 0, 0);
        }
    };
    zero_guard_bands(tid);
    // the valid tiles of the batch are numbered through (rb_tiles.h: RbTiles)
    int total = 0, j = blockIdx.x;
    tiles.build(p.lens, p.T, TTo, tid, THREADS);
    total = tiles.total();
    if (j >= total) return;
    const int G = gridDim.x;

    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    // the residual stream of a tile, fp32, straight into accumulator layout (lane & 31 = row, 4 consecutive channels per 16 B access).
    // Buffer loads over the utterance [0, len) x C return zeros for rows outside it (t < 0 wraps to a huge unsigned offset) = the zero padding.
    auto load_x = [&](f32x16 (&d)[NT], int m, int bb, int base, int ln) {   // 32-row slab m of this wave
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (long long)bb * p.T * C), 0, ln * C * 4, 0x00020000);
        const int o0 = ((base + wt * MT * 32 + (lane & 31)) * C + wc * NT * 32 + 4 * (lane >> 5)) * 4;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o0 + (m * 32 * C + n * 32 + 8 * q) * 4, 0, RB_X_AUX);
                const f32x4 f = __builtin_bit_cast(f32x4, v);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[n][4 * q + e] = f[e];
            }
    };

    int b = 0, len, t0;
    tiles.locate(j, b);
    len = tiles.len_of(b);
    t0 = tiles.first_row(j, b, TTo) - (p.wav ? PH : 0);
    f32x16 xr[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) load_x(xr[m], m, b, t0 - H, len);

    const int kg_stride = (C / 32) * 64;
    const int S = (REAL_STEPS ? p.K : p.Kp) * NKG;   // k-steps (packed taps are zero padded so that Kp * NKG % 4 == 0)

#pragma unroll 1
    for (;;) {
    // the thread index passes through an opaque move every tile: everything derived from it is recomputed per tile instead of being
    // hoisted out of the tile loop and spilled (rblock.hip)
    tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    wt = wave % WT, wc = wave / WT;
    const int xlane = (GR + wt * MT * 32 + (lane & 31)) * PITCH + (lane >> 5) * 16;
    const size_t wlane = (size_t)(wc * NT) * 64 + lane;
    const bool wav_now = p.wav != nullptr;
    t0 = __builtin_amdgcn_readfirstlane(t0);
    const int base_t = t0 - H;  // global time of local row 0
    const long long brow = (long long)b * p.T;
    // the workgroup's next tile: static (j + G), or — p.tile_ctr — the next unclaimed tile of the launch (tiles 0 .. G-1 are the
    // workgroups' first tiles, the counter hands out G, G+1, ...); the claim is broadcast through LDS behind a barrier that exists anyway
    unsigned claim = 0;
    if (p.tile_ctr && tid == 0) claim = atomicAdd(p.tile_ctr, 1u);
    int jn = j + G;
    bool has_next = jn < total;
    int bn = b, lenn = len, t0n = 0;
    auto plan_next = [&]() {
        has_next = jn < total;
        bn = b;
        if (has_next) {
            tiles.locate(jn, bn);
            lenn = tiles.len_of(bn);
            t0n = tiles.first_row(jn, bn, TTo) - (p.wav ? PH : 0);
        }
    };
    if (!p.tile_ctr) plan_next();
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)(p.S + brow * C), 0, len * C * 4, 0x00020000);

    auto load_bias = [&](f32x4 (&bb)[NT][4], const float* bias) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) bb[n][q] = *(const f32x4*)(bias + (wc * NT + n) * 32 + 8 * q + 4 * (lane >> 5));
    };
    const bool all_inb = base_t >= 0 && base_t + W <= len;   // block-uniform: no row of the tile needs masking
    int n_ovf = 0;
    // 16-bit leaky_relu(v, 0.1) of this wave's rows -> LDS operand tile, zero outside the utterance (MASKED = false: a tile wholly inside it)
    auto write_act_impl = [&](const f32x16 (&v)[MT][NT], auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int row = (wt * MT + m) * 32 + (lane & 31);
            const int t = base_t + row;
            const bool inb = !MASKED || (t >= 0 && t < len);
            // range guard: only the rows this tile OUTPUTS are counted — every in-utterance row is an output row of exactly one tile and
            // carries the exact activation there at both conversion points, so the count is a census
            const bool counted = inb && row >= H && row < H + TT;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = (wc * NT + n) * 32 + 8 * q + 4 * (lane >> 5);
                    const f32x4 v4 = {v[m][n][4 * q], v[m][n][4 * q + 1], v[m][n][4 * q + 2], v[m][n][4 * q + 3]};
                    uint2 pk = act4<EL>(v4, 0.1f);
                    if constexpr (GUARD) n_ovf += counted ? ovf4(v4, 0.1f) : 0;
                    if constexpr (MASKED) {
                        if (!inb) pk = make_uint2(0, 0);
                    }
                    *(uint2*)(act + (GR + row) * PITCH + co * 2) = pk;
                }
        }
    };
    auto write_act = [&](const f32x16 (&v)[MT][NT]) {
        if (all_inb) write_act_impl(v, std::false_type{});
        else write_act_impl(v, std::true_type{});
    };

    uint4 ring[4][NT];
    f32x4 bb[NT][4];
    rb_preload<NT>(ring, p.w[0] + wlane, kg_stride);   // in flight during the first activation write
    load_bias(bb, p.b[0]);
    write_act(xr);
    __syncthreads();

#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
        // x = x + b + W * leaky_relu(x): the convolution accumulates straight into the residual registers
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) xr[m][n][4 * q + e] += bb[n][q][e];
        if (it == 0) load_bias(bb, p.b[1]);
        const int d = p.dil[it];
        const uint4* wq = p.w[it] + wlane;
        if constexpr (REAL_STEPS) {
            f32x16 unused[NT];
            rb2_contract<EL, MT, NT, NKG, PITCH, 4, false>(xr, ring, act, xlane - ((p.K - 1) / 2) * d * PITCH, wq, S, d * PITCH, unused);
        } else
            rb_contract<EL, MT, NT, NKG, PITCH, false, 1>(xr, ring, act, xlane - ((p.K - 1) / 2) * d * PITCH, wq, S, d * PITCH);
        if (it == 0) rb_preload<NT>(ring, p.w[1] + wlane, kg_stride);   // the second convolution's first weights fly during barrier + rewrite
        if (p.tile_ctr && it == 1 && tid == 0) tiles.publish_claim(G, claim);   // the claimed tile, for everyone (read behind the barrier)
        __syncthreads();               // every wave is done reading the operand tile
        if (it == 0) {
            write_act(xr);             // the operand of the second convolution: leaky_relu of the UPDATED x
            __syncthreads();
        }
    }

    if (p.tile_ctr) {
        jn = tiles.claimed();
        plan_next();
    }
    {
    // ---- epilogue (rblock.hip's transposition, rb_tiles.h's row body): rows [H, H+TT) leave as whole rows through wave-private fp32 staging rows; halo rows are sent out of
    // range explicitly, rows >= len are dropped by the buffer range check
    const auto rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Sa ? p.Sa + brow * C : (unsigned short*)(p.S + brow * C)), 0,
                                                        len * C * 2, 0x00020000);
    constexpr int CW = NT * 32, F4W = CW / 4, RPI = 64 / F4W, NRD = 32 / RPI;
    const int er = lane / F4W, ec = lane % F4W;
    const int goffw = base_t * C * 4 + (wc * CW + ec * 4) * 4;
    static_assert(F4W == 8 && RPI == 8 && NRD == 4, "8 lanes per row, 8 rows per access");
    // (the conflict-free row order of rblock.hip's epilogue; C = 32 keeps consecutive rows)
    const int erow_slab_base = C == 32 ? er : (er >> 2) + ((er & 1) ? 16 : 0) + ((er & 2) ? 8 : 0);
    auto srow = [&](int u) { return (C == 32 ? 8 : 2) * u + erow_slab_base; };
    auto erow = [&](int m, int u) { return (wt * MT + m) * 32 + srow(u); };
    auto eoff = [&](int m, int u) {
        const int row = erow(m, u);
        return (row >= H && row < H + TT) ? goffw + row * (C * 4) : (int)0x80000000;
    };
    u32x4 sold[MT][NRD];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NRD; ++u) {
            sold[m][u] = u32x4{0u, 0u, 0u, 0u};
            if (p.mode >= 1) sold[m][u] = __builtin_amdgcn_raw_buffer_load_b128(rs_s, eoff(m, u), 0, VP_LD_AUX);
        }
    // fused conv_post: the stage output leaky_relu(xs / num_kernels) stays in LDS as an fp32 tile ([TT rows][C], rows outside the
    // utterance zero = conv_post's zero padding); the transposition rows move behind it.  Otherwise they lie inside the operand tile's
    // rows (dead behind the barrier above; the guard bands stay untouched)
    constexpr int OP = C * 4;
    char* otile = smem;
    char* estage = wav_now ? smem + std::max((size_t)TT * OP, ACT_BYTES) : smem + (size_t)GR * PITCH;
    char* stg = estage + (wt * 32) * EP + (wc * CW) * 4;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = xr[m][n][4 * q + e];
                *(f32x4*)(stg + (lane & 31) * EP + (n * 32 + 8 * q + 4 * (lane >> 5)) * 4) = v;
            }
        // slab m of the residual registers is free: the NEXT tile's slab m starts its trip into them
        if (has_next) load_x(xr[m], m, bn, t0n - H, lenn);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < NRD; ++u) {
            const int off = eoff(m, u);
            f32x4 o = *(const f32x4*)(stg + srow(u) * EP + ec * 16);
            o += __builtin_bit_cast(f32x4, sold[m][u]);                // xs += resblock(x)  (hifigan.py:133-135); zeros in mode 0
            if (wav_now) {
                const int row = erow(m, u);
                if (row >= H && row < H + TT) {
                    const int t = base_t + row;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (t >= 0 && t < len) ? lrelu(o[e] / p.div, p.slope) : 0.f;
                    *(f32x4*)(otile + (size_t)(row - H) * OP + (wc * CW + ec * 4) * 4) = o;
                }
                continue;
            }
            rb_stage_row(o, rs_s, rs_a, off, p.mode, p.div, p.slope, p.drop_S != 0, p.Sa != nullptr, false);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                               // slab m + 1 reuses this wave's staging block
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if constexpr (C == 32) if (wav_now) {   // (the launcher rejects p.wav for other widths)
        __syncthreads();                                               // the fp32 output tile is whole
        rb_conv_post_tanh<C, THREADS, 3>(otile, p.post_w, p.post_b, p.wav + brow, t0, TTo, len, p.bad, tid);
    }
    }   // (epilogue)
    if constexpr (GUARD) {
        if (n_ovf) atomicAdd(p.ovf, (unsigned long long)n_ovf);
    }
    if (!has_next) break;
    // the transposition rows (and the fp32 output tile) alias the operand tile: every wave's epilogue reads are over behind this barrier,
    // before the next tile's first activation write.  The output tile also covers the guard bands: zero again (ordered before the first
    // contraction by the barrier behind that write)
    __syncthreads();
    if (wav_now) zero_guard_bands(threadIdx.x);
    j = jn;
    b = bn;
    len = lenn;
    t0 = t0n;
    }   // (tiles of this workgroup)
}

template <int C, int MT, int NT, int WT, int WC, int EL, bool GUARD = false>
static hipError_t rb2x_launch_cfg(const RB2xParams& p, hipStream_t stream) {
    constexpr int W = 32 * MT * WT;
    RB2xParams q = p;
    q.halo = rb2x_halo(p.K, p.dil[0], p.dil[1]);
    q.guard = rb2x_guard(p.K, p.dil[0], p.dil[1]);
    const int TT = W - 2 * q.halo, TTo = p.wav ? TT - 6 : TT;
    if (TTo < 32) return hipErrorOutOfMemory;          // (no useful tile: the caller tries the next configuration)
    if ((long long)p.T * C * 4 >= (1LL << 31)) return hipErrorInvalidValue;   // 32-bit byte offsets inside an utterance's buffer resource
    if (p.wav && (C != 32 || p.mode != 2 || !p.post_w || !p.post_b)) return hipErrorInvalidValue;
    size_t lds = rb2x_lds_bytes(C, W, WT, q.halo, q.guard, p.wav != nullptr);
    q.pre_off = (int)lds;
    lds += rb_table_bytes(p.B);
    if (lds > 160 * 1024) return hipErrorOutOfMemory;
    if constexpr (EL == EL_F16 && !GUARD) {
        if (p.ovf) return rb2x_launch_cfg<C, MT, NT, WT, WC, EL, true>(p, stream);
    }
    constexpr auto kern = rb2x_kernel<C, MT, NT, WT, WC, EL, GUARD>;
    if (const hipError_t e = rb_allow_full_lds<kern>(); e != hipSuccess) return e;
    constexpr int THREADS = 64 * WT * WC;
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    const int grid = rb_resident_grid(cus, lds, THREADS, THREADS <= 256 ? 2 : 1, (long long)p.B * ((p.T + TTo - 1) / TTo));
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), lds, stream, q);
    return hipGetLastError();
}

// the `base` configuration's time-waves per width (rb2x_lds_bytes' third argument)
static int rb2x_base_time_waves(int C) { return C == 32 ? 4 : (C == 64 ? 4 : (C == 128 ? 2 : 1)); }

bool rb2x_supported(int C, int K, int d0, int d1) {
    if (C != 32 && C != 64 && C != 128 && C != 256) return false;
    if (!(K & 1) || K < 3 || K > 11 || d0 < 1 || d1 < 1) return false;
    const int halo = rb2x_halo(K, d0, d1), guard = rb2x_guard(K, d0, d1), W = rb2x_base_rows(C);
    if (W - 2 * halo < (C == 32 ? 38 : 32)) return false;
    return rb2x_lds_bytes(C, W, rb2x_base_time_waves(C), halo, guard, C == 32) + rb_table_bytes(DTTS_MAX_VOCODER_BATCH) <= 160 * 1024;
}

template <int EL>
static hipError_t rb2x_launch_el(const RB2xParams& p, int C, hipStream_t stream) {
    const bool wide = rb2x_wide_wanted(C, p.K, rb2x_halo(p.K, p.dil[0], p.dil[1]));
    // RB_TRY: a configuration whose LDS cannot hold the tile table of this many utterances, or whose tile the halo eats, falls through to `base`
    if (C == 32 && wide) RB_TRY((rb2x_launch_cfg<32, 4, 1, 8, 1, EL>(p, stream)));    // 1024-row tile, 8 waves over time
    if (C == 32) return rb2x_launch_cfg<32, 4, 1, 4, 1, EL>(p, stream);               // 512-row tile, 4 waves, two workgroups per CU
    if (C == 64) return rb2x_launch_cfg<64, 4, 1, 4, 2, EL>(p, stream);               // 512-row tile, 8 waves (4 time x 2 channel)
    if (C == 128 && wide) RB_TRY((rb2x_launch_cfg<128, 6, 1, 2, 4, EL>(p, stream)));  // 384-row tile
    if (C == 128) return rb2x_launch_cfg<128, 4, 1, 2, 4, EL>(p, stream);             // 256-row tile, 8 waves (2 time x 4 channel)
    if (C == 256 && wide) RB_TRY((rb2x_launch_cfg<256, 6, 1, 1, 8, EL>(p, stream)));  // 192-row tile
    if (C == 256) return rb2x_launch_cfg<256, 4, 1, 1, 8, EL>(p, stream);             // 128-row tile, 8 waves over channels
    return hipErrorInvalidValue;
}

hipError_t rb2x_launch(const RB2xParams& p, int C, hipStream_t stream) {
    if (!rb2x_supported(C, p.K, p.dil[0], p.dil[1])) return hipErrorInvalidValue;
    const hipError_t e = p.el == EL_F16 ? rb2x_launch_el<EL_F16>(p, C, stream) : rb2x_launch_el<EL_BF16>(p, C, stream);
    return e == hipErrorOutOfMemory ? hipErrorInvalidValue : e;
}

} // namespace dtts
