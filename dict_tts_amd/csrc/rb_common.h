// Shared device helpers of the fused HifiGAN kernels (rblock.hip, vpair.hip, rb2x.hip): bf16 conversion, the weight-fragment
// ring preload and the static-offset MFMA contraction loop over an LDS activation tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "voc_el.h"

namespace dtts {

// Cache policy of the fused vocoder kernels' global accesses (buffer-instruction aux bits on gfx950: 1 = sc0, 2 = nt, 16 = sc1).
// Their results are consumed by the NEXT launch, ~1 ms and ~1 GB of traffic later: streaming them (nt + sc1) keeps them from evicting
// what the kernel re-reads — the x tile between staging and the epilogue's residual, the weight fragments.  Same-box A/B
// (LABNOTES (yy)): stores 0 -> 18: -0.9 %; + the read-once operands (the stage sum, the epilogue's last read of x): -1.2 %; streaming
// rblock's x loads as well: +2 % (worse: neighbouring tiles' halos re-read them).
constexpr int VP_ST_AUX = 18;   // y / activated-copy stores
constexpr int VP_LD_AUX = 18;   // the stage sum read once by the accumulating ResBlocks
constexpr int VP_XI_AUX = 2;    // vpair's epilogue: the last read of the x tile
constexpr int RB_X_AUX = 0;     // rblock's residual-stream loads: cached (halo rows are shared with the neighbouring tiles)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ unsigned rf2bf(float f) {  // round-to-nearest-even fp32 -> bf16 bits (hardware convert)
    const __bf16 h = (__bf16)f;
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
// two fp32 -> one dword of two bf16 (round-to-nearest-even), a single v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pack2bf(float a, float b) {
    const bf16x2_t v = __builtin_convertvector(f32x2_t{a, b}, bf16x2_t);
    return __builtin_bit_cast(unsigned, v);
}
// leaky_relu for 0 <= slope <= 1 as max(a, a * slope): v_mul + v_max (the asm keeps hipcc from adding the
// canonicalising v_max a,a in front of fmaxf; NaNs do not occur on this path)
__device__ __forceinline__ float lrelu(float a, float slope) {
    float r;
    const float b = a * slope;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---- element type of the 16-bit MFMA operands.  EL_BF16: v_mfma_f32_32x32x16_bf16 (8-bit significand); EL_F16:
// v_mfma_f32_32x32x16_f16 (11-bit significand, same rate) — the ResBlock stages of the waveform-exact vocoder mode.
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;

template <int EL>
__device__ __forceinline__ unsigned pack2(float a, float b) {   // two fp32 -> one dword of two 16-bit values, round-to-nearest-even
    if constexpr (EL == EL_F16) {
        const f16x2_t v = __builtin_convertvector(f32x2_t{a, b}, f16x2_t);   // v_cvt_pk_f16_f32
        return __builtin_bit_cast(unsigned, v);
    } else {
        return pack2bf(a, b);
    }
}
// leaky_relu feeding a 16-bit operand.  fp16 saturates at 65504 instead of overflowing to inf: median(a, a*slope, 65504)
// = min(max(a, a*slope), 65504) for every a > -655040 — still two instructions (v_mul + v_med3).
template <int EL>
__device__ __forceinline__ float lrelu_op(float a, float slope) {
    if constexpr (EL == EL_F16) return __builtin_amdgcn_fmed3f(a, a * slope, 65504.f);
    else return lrelu(a, slope);
}
// four consecutive channels -> two dwords of 16-bit leaky_relu(v, slope): the slope products as two packed fp32 multiplies
// (v_pk_mul_f32), the max / saturation per value, two packed converts — 8 VALU instructions for 4 values, same arithmetic as
// pack2<EL>(lrelu_op<EL>(.), .) value by value (10)
template <int EL>
__device__ __forceinline__ uint2 act4(const f32x4& v, float slope) {
    const f32x2_t a = {v[0], v[1]}, b = {v[2], v[3]};
    const f32x2_t ta = a * slope, tb = b * slope;
    if constexpr (EL == EL_F16) {
        // convert first, then leaky_relu on PACKED fp16 pairs: v_cvt_pk_f16_f32, v_pk_mul_f16, v_pk_max_f16 = 6 VALU per 4 values (the
        // activation rewrites of the narrow ResBlock kernels are VALU-bound, LABNOTES round 4 (C)).  The slope is fp16(0.1) and negative
        // values round twice: simulated waveform error 5.19e-5 -> 5.28e-5 (tools/precision_sim.py arithmetic).  NO saturation, on purpose: a
        // pre-activation beyond the fp16 range becomes +-inf (also a NEGATIVE one below -65504, whose exact leaky_relu would still be
        // representable), the inf / NaN it makes of every later sum reaches conv_post, and the always-on detector there (rblock.hip /
        // vconv.hip: non-finite pre-tanh value) reports the call — no overflow returns plausible-looking samples.  ovf4 below counts
        // exactly these values.
        const _Float16 hs = (_Float16)slope;   // (a compile-time constant at every call site: folds)
        const f16x2_t slope2 = {hs, hs};
        const f16x2_t ha = __builtin_convertvector(a, f16x2_t), hb = __builtin_convertvector(b, f16x2_t);
        const f16x2_t ra = __builtin_elementwise_max(ha, ha * slope2), rb = __builtin_elementwise_max(hb, hb * slope2);
        (void)ta;
        (void)tb;
        return make_uint2(__builtin_bit_cast(unsigned, ra), __builtin_bit_cast(unsigned, rb));
    } else {
        float r0, r1, r2, r3;
        asm("v_max_f32 %0, %1, %2" : "=v"(r0) : "v"(a[0]), "v"(ta[0]));
        asm("v_max_f32 %0, %1, %2" : "=v"(r1) : "v"(a[1]), "v"(ta[1]));
        asm("v_max_f32 %0, %1, %2" : "=v"(r2) : "v"(b[0]), "v"(tb[0]));
        asm("v_max_f32 %0, %1, %2" : "=v"(r3) : "v"(b[1]), "v"(tb[1]));
        return make_uint2(pack2<EL>(r0, r1), pack2<EL>(r2, r3));
    }
}

// fp16 range guard (GUARD instantiations of vpair / rblock, DTTS_VOC_F16 only): how many of four pre-activation values the 16-bit
// conversion of act4 turns into +-inf — the conversion comes FIRST there, so |v| > 65504 overflows on either side (round 3's form
// applied leaky_relu in fp32 first: v > 65504 saturated, v * slope < -65504 overflowed).  The reference computes these
// convolutions in fp32 (modules/hifigan/hifigan.py:51-58): a non-zero count means the fp16 mode is not valid for this checkpoint /
// input, and the caller falls back to DTTS_VOC_BF16X3 (dict_tts_amd/vocoder.py).
__device__ __forceinline__ int ovf4(const f32x4& v, float slope) {
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) n += (__builtin_fabsf(v[e]) > 65504.f) ? 1 : 0;
    return n;
}

template <int EL>
__device__ __forceinline__ f32x16 mfma16(const uint4& a, const uint4& b, const f32x16& c) {
    if constexpr (EL == EL_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- MFMA shape of a contraction.  A block of 32 output channels x 32 time rows x 32 input channels is either two
// v_mfma_f32_32x32x16 (MfmaShape<32>: rb2x.hip, rblock.hip at C = 32 / 128 / 256) or four v_mfma_f32_16x16x32 (MfmaShape<16>: vpair.hip, rblock.hip at C = 64; 2 channel halves x
// 2 row halves) — the same MFMA cycles, the same number of 16-byte operand fragments per lane, 16 fp32 accumulators per lane either way.
// An accumulator QUAD qi (0..3) is four consecutive output channels of one time row in both shapes, so act4, the 8-byte LDS rewrite and
// the 16-byte fp32 accesses keep their form; which (row, channel) a quad is comes from row() / chan().  The weights are the A operand
// (its row = output channel), the activations the B operand (its column = time row):
//   32: A/B lane l <-> row/column l & 31, k = 8 (l >> 5) + j;  D: column l & 31, row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
//   16: A/B lane l <-> row/column l & 15, k = 8 (l >> 4) + j;  D: column l & 15, row 4 (l >> 4) + reg
// A pack in the shape's fragment order (pack.hip: pack_conv, `frag`) goes with it.
template <int M>
struct MfmaShape;

template <>
struct MfmaShape<32> {
    static constexpr int FRAG = 32;   // pack_conv's fragment order
    static constexpr int CI = 16;     // input channels per k-step
    static constexpr int KB = 32;     // bytes of a k-step within an activation row
    static constexpr int WF = 1;      // weight fragments per 32-channel co-tile and k-step
    static constexpr int XF = 1;      // activation fragments per 32-row tile and k-step
    static constexpr int XROWS = 32;  // rows between two activation fragments of a row tile
    static constexpr int RD = 4;      // depth of the weight ring in k-steps (fragments RD - 1 steps = 48 input channels ahead)
    static constexpr int QB = 1;      // accumulator quads that share their four channels (= their bias): quads QB * b ... QB * b + QB - 1
    typedef f32x16 acc_t;
    static __device__ __forceinline__ int row(int lane, int qi) { return lane & 31; }                   // row within the 32-row tile
    static __device__ __forceinline__ int chan(int lane, int qi) { return 8 * qi + 4 * (lane >> 5); }   // first channel within the co-tile
    static __device__ __forceinline__ int xoff(int lane, int pitch) { return (lane & 31) * pitch + (lane >> 5) * 16; }   // activation fragment of a lane: LDS byte offset
    static __device__ __forceinline__ f32x4 quad(const acc_t& a, int qi) { return f32x4{a[4 * qi], a[4 * qi + 1], a[4 * qi + 2], a[4 * qi + 3]}; }
    static __device__ __forceinline__ void set_quad(acc_t& a, int qi, const f32x4& v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[4 * qi + e] = v[e];
    }
    // quad qi += v, element by element (as a vector sum hipcc forms packed adds on aligned register pairs and copies accumulators to get them:
    // 15 registers more in rblock's kernels, spills in its 640-row one)
    static __device__ __forceinline__ void add_quad(acc_t& a, int qi, const f32x4& v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[4 * qi + e] += v[e];
    }
    template <int EL>
    static __device__ __forceinline__ void mma(acc_t& d, const uint4* w, const uint4* const (&x)[XF], const acc_t& c) {
        d = mfma16<EL>(w[0], *x[0], c);
    }
};

template <>
struct MfmaShape<16> {
    static constexpr int FRAG = 16;
    static constexpr int CI = 32;
    static constexpr int KB = 64;
    static constexpr int WF = 2;      // the two 16-channel halves of a co-tile
    static constexpr int XF = 2;      // the two 16-row halves of a row tile
    static constexpr int XROWS = 16;
    static constexpr int QB = 2;      // (the two row halves)
    static constexpr int RD = 2;      // fragments one k-step = 32 input channels ahead, in the registers of the 32x32x16 ring (4 x 16 channels)
    struct acc_t {
        f32x4 q[4];                   // quad 2 ch + rh: channel half ch, row half rh
    };
    static __device__ __forceinline__ int row(int lane, int qi) { return 16 * (qi & 1) + (lane & 15); }
    static __device__ __forceinline__ int chan(int lane, int qi) { return 16 * (qi >> 1) + 4 * (lane >> 4); }
    static __device__ __forceinline__ int xoff(int lane, int pitch) { return (lane & 15) * pitch + (lane >> 4) * 16; }
    static __device__ __forceinline__ f32x4 quad(const acc_t& a, int qi) { return a.q[qi]; }
    static __device__ __forceinline__ void set_quad(acc_t& a, int qi, const f32x4& v) { a.q[qi] = v; }
    static __device__ __forceinline__ void add_quad(acc_t& a, int qi, const f32x4& v) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a.q[qi][e] += v[e];
    }
    template <int EL>
    static __device__ __forceinline__ void mma(acc_t& d, const uint4* w, const uint4* const (&x)[XF], const acc_t& c) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int rh = 0; rh < 2; ++rh) {
                if constexpr (EL == EL_F16)
                    d.q[2 * ch + rh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w[ch]), __builtin_bit_cast(f16x8, *x[rh]), c.q[2 * ch + rh], 0, 0, 0);
                else
                    d.q[2 * ch + rh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w[ch]), __builtin_bit_cast(bf16x8, *x[rh]), c.q[2 * ch + rh], 0, 0, 0);
            }
    }
};

// Zero rows on both sides of rblock's LDS tile.  Below the tile a contraction reaches (K - 1) / 2 * dil rows (25 at k = 11, dilation 5).  Above
// it the LAST real tap reaches the same 25 rows, a zero tap of a pack padded to whole groups would reach dil rows more (30; no configuration
// multiplies one today: 4 or more steps per tap, rb_contract's half group at two steps per tap, the real steps at C = 32), and the activation
// fragment prefetched behind the last step is the first k-step of the tap behind that one: dil rows more (35), bytes 0 .. SH::KB - 1 <= 63 of
// rows that exist.  The prefetch reaches no further
// with MfmaShape<16> than with <32>: its two fragments are the two 16-row halves of the SAME 32-row tile (rb_group: row offsets 32 m + 16 f),
// and 64 bytes instead of 32 stay inside a row (PITCH >= 80).  40 >= 35 covers both shapes.
constexpr int RB_GUARD = 40;

// acc += W * act, all taps; act is the LDS tile (bf16, pitch PITCH), weights in fragment order [step][co-tile][lane] ([step][co-tile][half][lane], MfmaShape<16>)
// first RD - 1 weight fragment sets of a convolution (issued early: before the barriers / activation writes that precede it)
template <int NTW, int RD>
__device__ __forceinline__ void rb_preload(uint4 (&ring)[RD][NTW], const uint4* w, int kg_stride) {
#pragma unroll
    for (int s = 0; s < RD - 1; ++s)
#pragma unroll
        for (int n = 0; n < NTW; ++n) ring[s][n] = w[(size_t)s * kg_stride + n * 64];
}

// One group of 4 k-steps of the contraction (see rb_contract; a k-step is SH::CI input channels of one tap).  CINIT: the very first MFMA of every accumulator tile
// takes its C operand from cinit[n] (the bias pattern of this lane's 16 channel slots, identical for every row tile), so
// the accumulators need no initialisation pass at all.
// MH > 1: the wave owns MH * MT row tiles, processed as MH passes of MT tiles per weight fragment (pass h covers rows
// h * MT * 32 ...): a weight fragment is fetched once per step and used for MH * MT MFMAs, while only MT activation
// fragments are live at a time.
// ONE set of activation fragments (round 5 (Y)).  Instead of reading the next (step, pass)'s MT fragments in one
// burst at the top of a step (a double buffer), row tile m's next fragment is read right behind the MFMAs that consumed the current one and lands while the other
// row tiles' MFMAs run: eight waves' bursts no longer queue on the CU's LDS pipe in front of the matrix pipe (-1.5 ... -5.9 % per kernel), MT * 4 registers less.
// The scheduling barriers around the read keep it where it is written (+0.4 % without them).  (The line "(NT == 1 here)" below: the read follows the LAST co-tile's MFMA.)
// NKG: k-steps per tap (C / SH::CI).  NU: steps of this group: 4, or 2 for the half group that ends a contraction of 4 n + 2 steps (rb_contract: TAIL).
template <int EL, int MT, int NT, int NKG, int PITCH, bool CINIT, int MH = 1, class SH = MfmaShape<32>, int NU = 4>
__device__ __forceinline__ void rb_group(typename SH::acc_t (&acc)[MH * MT][NT], const typename SH::acc_t (&cinit)[NT], uint4 (&ring)[SH::RD][NT * SH::WF],
                                         uint4 (&xa)[MT], const char* act, const uint4* wpf, int xb, int dilP, int g) {
    constexpr int GPT = (NKG >= 4) ? NKG / 4 : 1;     // groups per tap
    constexpr int KGS = NKG * SH::CI * 2 * SH::WF;    // uint4 elements between consecutive steps (= NCT * 64 per fragment of a co-tile, NCT = C / 32)
    constexpr int HSTRIDE = MT * 32 * PITCH;          // LDS bytes between two passes
    constexpr int RD = SH::RD, WF = SH::WF, KB = SH::KB;
    static_assert(NU % RD == 0, "a group is whole turns of the ring");
    static_assert(NU == 4 || (NKG < 4 && NU % NKG == 0), "a short group is whole taps");
#pragma unroll
    for (int u = 0; u < NU; ++u) {
#pragma unroll
        for (int h = 0; h < MH; ++h) {
            if (h == 0) {
#pragma unroll
                for (int n = 0; n < NT * WF; ++n) ring[(u + RD - 1) % RD][n] = wpf[u * KGS + n * 64];
            }
            // The activation fragments of a (step, pass) are NP = MT * XF positions p = XF * m + f (row tile m, fragment f), consumed in this order;
            // MT of them are live at a time, position p in register set p % MT, and the one MT positions ahead is read behind the MFMAs that
            // consumed position p: from this (step, pass) at `cur` (XF = 2, p < MT), or from the next at `off`.
            constexpr int NP = MT * SH::XF;
            int cur = 0;   // this (step, pass)
            if constexpr (SH::XF > 1) {
                if constexpr (NKG >= 4) cur = xb + ((g * 4 + u) % NKG) * KB + h * HSTRIDE;
                else cur = xb + (u / NKG) * dilP + (u % NKG) * KB + h * HSTRIDE;
            }
            int off;   // the next (step, pass)
            if (h + 1 < MH) {
                // same step, next pass
                if constexpr (NKG >= 4) off = xb + ((g * 4 + u) % NKG) * KB + (h + 1) * HSTRIDE;
                else off = xb + (u / NKG) * dilP + (u % NKG) * KB + (h + 1) * HSTRIDE;
            } else if constexpr (NKG >= 4) {
                const int kgn = (g * 4 + u + 1);            // k-group index within the tap (may be NKG: next tap)
                off = (u == 3 && g == GPT - 1) ? xb + dilP : xb + (kgn % NKG) * KB;
            } else {
                const int un = u + 1;                        // step within the group of TU taps
                off = xb + (un / NKG) * dilP + (un % NKG) * KB;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const uint4* xf[SH::XF];
#pragma unroll
                    for (int f = 0; f < SH::XF; ++f) xf[f] = &xa[(m * SH::XF + f) % MT];
                    if (CINIT && u == 0) SH::template mma<EL>(acc[h * MT + m][n], &ring[u % RD][n * WF], xf, cinit[n]);
                    else SH::template mma<EL>(acc[h * MT + m][n], &ring[u % RD][n * WF], xf, acc[h * MT + m][n]);
                    if (n == NT - 1) {   // the fragments MT positions ahead, behind the MFMAs that read row tile m's (NT == 1 here)
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int f = 0; f < SH::XF; ++f) {
                            const int p = m * SH::XF + f, pn = (p + MT) % NP;
                            xa[p % MT] = *(const uint4*)(act + (p + MT < NP ? cur : off) + (pn / SH::XF * 32 + pn % SH::XF * SH::XROWS) * PITCH);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// acc (+)= W * act over all taps.  k-steps (SH::CI input channels of one tap: 16 or 32) are processed 4 at a time (a group =
// TU taps, or 1 / GPT of a tap); inside a group every LDS / global offset is a compile-time immediate off two bases that advance once
// per group, so the loop body is MFMAs, ds_read_b128, global_load_dwordx4 and ~4 address instructions.  CINIT: acc = cinit + W * act
// (acc not read).  What the prefetches read past the end, and why neither needs a clamp:
//   weights: fragments run RD - 1 steps ahead, so the last group loads RD - 1 steps behind step S - 1: 3 x 16 channels (MfmaShape<32>) or
//     1 x 32 channels (MfmaShape<16>), i.e. at most three 16-channel steps of every co-tile.  pack_conv appends C_in_pad / 16 + 8 >= 10
//     zero 16-channel steps to every pack, in either fragment order (the two orders have the same size per 32 channels);
//   activations: MT fragment positions ahead, i.e. at most the first k-group of the tap BEHIND the last one (row offset K * dil from the
//     wave's first row, the same 32 rows per row tile in both shapes, bytes 0 .. SH::KB - 1 <= 63 of a row): one spare tap of rows, which
//     vpair's launcher allots (TT + dil (K - 1) + max(dil + 1, .) rows for c1, TT + K + 1 for c2) and rblock's RB_GUARD covers.
template <int EL, int MT, int NT, int NKG, int PITCH, bool CINIT = false, int MH = 1, class SH = MfmaShape<32>>
__device__ __forceinline__ void rb_contract(typename SH::acc_t (&acc)[MH * MT][NT], uint4 (&ring)[SH::RD][NT * SH::WF], const char* act, int xrow0,
                                            const uint4* w, int S, int dilP, const typename SH::acc_t (*cinit)[NT] = nullptr) {
    typedef typename SH::acc_t acc_t;
    constexpr int TU = (NKG >= 4) ? 1 : 4 / NKG;      // taps per group of 4 steps
    constexpr int GPT = (NKG >= 4) ? NKG / 4 : 1;     // groups per tap
    constexpr int KGS = NKG * SH::CI * 2 * SH::WF;
    // TAIL: two k-steps per tap (C = 64 on MfmaShape<16>) and an ODD number of taps, so S = 4 n + 2: whole groups, then one half group of 2
    // steps = the last tap.  Nothing is padded: no zero tap is multiplied to round S up to whole groups (it would be 1 / K of the MFMAs more).
    // The caller guarantees S % 4 == 2 (rblock_supported: odd kernel sizes only; the launcher refuses anything else).
    constexpr bool TAIL = (NKG == 2 && SH::FRAG == 16);
    const int SG = TAIL ? S - 2 : S;                  // steps in whole groups
    uint4 xa[MT];   // the first MT fragment positions of step 0 (rb_group)
#pragma unroll
    for (int p = 0; p < MT; ++p) xa[p] = *(const uint4*)(act + xrow0 + (p / SH::XF * 32 + p % SH::XF * SH::XROWS) * PITCH);
    const uint4* wpf = w + (SH::RD - 1) * KGS;        // prefetch pointer, RD - 1 steps ahead
    int xb = xrow0;                                   // LDS byte offset of (tap of this group, kg 0)
    int g = 0;
    int s0 = 0;
    if constexpr (CINIT) {
        // (MfmaShape<16> has no S == 0 arm: the arm's copies of 4 * MH * MT * NT accumulator quads at the join cost the new shape 4 - 10
        // registers.  Its only caller, vpair_launch, refuses K < 3 (vpair_supported), so S = K * NKG >= 3 there, and vpair_kernel returns
        // before staging anything if it is ever entered with K < 1.  MfmaShape<32> keeps the arm, see below)
        if (SH::FRAG == 16 || S > 0) {
            rb_group<EL, MT, NT, NKG, PITCH, true, MH, SH>(acc, *cinit, ring, xa, act, wpf, xb, dilP, 0);
            s0 = 4;
            wpf += 4 * KGS;
            if constexpr (NKG >= 4) {
                if (++g == GPT) {
                    g = 0;
                    xb += dilP;
                }
            } else {
                xb += TU * dilP;
            }
        } else {   // no k-steps: acc = cinit (S > 0 at every call, which the compiler cannot know: dropping the test would change the generated code)
#pragma unroll
            for (int m = 0; m < MH * MT; ++m)
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n] = (*cinit)[n];
        }
    }
    for (; s0 < SG; s0 += 4) {
        const acc_t(&dummy)[NT] = *(const acc_t(*)[NT])acc[0];
        rb_group<EL, MT, NT, NKG, PITCH, false, MH, SH>(acc, dummy, ring, xa, act, wpf, xb, dilP, g);
        wpf += 4 * KGS;
        if constexpr (NKG >= 4) {
            if (++g == GPT) {
                g = 0;
                xb += dilP;
            }
        } else {
            xb += TU * dilP;
        }
    }
    if constexpr (TAIL) {
        const acc_t(&dummy)[NT] = *(const acc_t(*)[NT])acc[0];
        rb_group<EL, MT, NT, NKG, PITCH, false, MH, SH, 2>(acc, dummy, ring, xa, act, wpf, xb, dilP, 0);
    }
}

// ---- contraction over the REAL k-steps with a weight ring of RD register sets (fragments RD - 1 steps ahead; the activation fragments one
// step ahead; one fragment set, as in rb_group).  The C = 32 configurations of rblock.hip / rb2x.hip use RD = 4.  Steps are the REAL k-steps K * NKG (the zero
// padding of the packs to a multiple of four steps is not computed): the loop is unrolled over RD steps with a uniform exit at every tap
// boundary.  The packs carry >= 8 k-steps of slack and the LDS tile a spare tap of guard rows, so the prefetches past the end need no clamps.
template <int NT, int RD>
__device__ __forceinline__ void rb2_preload(uint4 (&ring)[RD][NT], const uint4* w, int kgs) {
#pragma unroll
    for (int s = 0; s < RD - 1; ++s)
#pragma unroll
        for (int n = 0; n < NT; ++n) ring[s][n] = w[(size_t)s * kgs + n * 64];
}

template <int EL, int MT, int NT, int NKG, int PITCH, int RD, bool FIRST, bool CINIT>
__device__ __forceinline__ bool rb2_group(f32x16 (&acc)[MT][NT], const f32x16 (&cinit)[NT], uint4 (&ring)[RD][NT], uint4 (&xa)[MT],
                                          const char* act, const uint4* wpf, int xb, int dilP, int left) {   // left: steps still to do (> 0)
    constexpr int KGS = (NKG / 2) * 64;
    static_assert(RD % NKG == 0 && RD % 2 == 0, "a ring turn covers whole taps");
#pragma unroll
    for (int u = 0; u < RD; ++u) {
        if (u && u % NKG == 0 && u >= left) return true;                // (uniform) the last tap is done
#pragma unroll
        for (int n = 0; n < NT; ++n) ring[(u + RD - 1) % RD][n] = wpf[u * KGS + n * 64];
        const int off = xb + ((u + 1) / NKG) * dilP + ((u + 1) % NKG) * 32;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                if (FIRST && CINIT && u == 0) acc[m][n] = mfma16<EL>(ring[u][n], xa[m], cinit[n]);
                else acc[m][n] = mfma16<EL>(ring[u][n], xa[m], acc[m][n]);
                if (n == NT - 1) {   // row tile m's fragment of the next step, behind the MFMAs that read the current one
                    __builtin_amdgcn_sched_barrier(0);
                    xa[m] = *(const uint4*)(act + off + m * 32 * PITCH);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
    }
    return left <= RD;
}

// acc (+)= W * act over the S = K * NKG real steps; ring holds steps 0 .. RD - 2 on entry (rb2_preload).  CINIT: acc = cinit + W * act.
template <int EL, int MT, int NT, int NKG, int PITCH, int RD, bool CINIT>
__device__ __forceinline__ void rb2_contract(f32x16 (&acc)[MT][NT], uint4 (&ring)[RD][NT], const char* act, int xrow0, const uint4* w, int S,
                                             int dilP, const f32x16 (&cinit)[NT]) {
    constexpr int KGS = (NKG / 2) * 64;
    uint4 xa[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) xa[m] = *(const uint4*)(act + xrow0 + m * 32 * PITCH);
    const uint4* wpf = w + (RD - 1) * KGS;
    int xb = xrow0;
    if (rb2_group<EL, MT, NT, NKG, PITCH, RD, true, CINIT>(acc, cinit, ring, xa, act, wpf, xb, dilP, S)) return;
    for (int left = S - RD;; left -= RD) {
        wpf += RD * KGS;
        xb += (RD / NKG) * dilP;
        if (rb2_group<EL, MT, NT, NKG, PITCH, RD, false, CINIT>(acc, cinit, ring, xa, act, wpf, xb, dilP, left)) return;
    }
}

} // namespace dtts
