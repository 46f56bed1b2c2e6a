// One ResBlock1 iteration  x <- x + c2(leaky_relu(c1(leaky_relu(x))))  (modules/hifigan/hifigan.py:51-58) in ONE
// kernel, for the C = 128 stage (bf16 MFMA).  Per-convolution, that stage is HBM-bound: 2.2 KB per row and iteration
// (bf16 copies in/out, the bf16 xt round trip, fp32 residual in/out).  Here a workgroup
//   * reads the fp32 stream once (tile + halo of d(k-1)/2 + (k-1)/2 rows), applies leaky_relu + bf16 rounding while
//     staging it into LDS (the same rounding point as everywhere else),
//   * runs c1 for 128 rows of xt, barriers, overwrites the LDS tile with bf16(leaky_relu(xt)) (zero outside the
//     utterance = the reference's zero padding), runs c2 for 128 - (k-1) valid output rows,
//   * re-reads the centre rows of x for the residual (L2-hot: this block staged them a moment ago) in the coalesced
//     epilogue and writes only the fp32 result (or accumulates into the stage sum xs for the last iteration).
// HBM bytes per row and iteration: ~0.8 KB in + 0.5 KB out.  4 waves over output channels, 3 workgroups per CU.
#include "vpair.h"
#include "rb_common.h"
#include "rb_tiles.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace dtts {

// TT = 128: 3 workgroups per CU; TT = 256: every weight fragment feeds 8 MFMAs instead of 4 (half the weight stream
// through the texture path, half the halo), 2 workgroups per CU when the LDS tile allows
// C = 256 (NT = 2 co-tiles per wave): the stage-1 ResBlocks; 128-, 96- and 64-row tiles (vpair_launch_el; the census never takes the 128-row one: vpair_launch_tt).
// WT = 2 (C = 128; no launch configuration selects it: 1.3 / 4 % slower, LABNOTES (K)): the four waves as 2 (time) x 2 (output channels), two co-tiles per wave — every activation fragment read from LDS feeds two
// MFMAs instead of one (half the ds_read_b128 traffic; twice the weight fragments through the texture path, as at C = 256).
// Both contractions run on the MFMA shape of vpair.h: vpair_mfma_shape (rb_common.h: MfmaShape): all row / channel arithmetic below goes through its helpers
// (row / chan of an accumulator quad, a lane's activation-fragment offset), and w1 / w2 arrive in its fragment order.
// X16 (round 6; EL_F16 only): the INPUT stream x is fp16 — iterations 1 and 2 of a ResBlock, whose predecessor stored its result with
// p.y16.  fp16(x) is exactly what the fp32 stream's staging computed as the convolution operand, so c1's operands keep their bits; what
// changes is the residual add (x16 + xt instead of x32 + xt).  The staging loads 8 channels per thread (half the bytes, half the
// accesses), needs no conversion (leaky_relu on the packed pairs as they arrive) and writes 16 bytes per LDS access; the epilogue
// re-reads 8 bytes per four channels and widens them in registers.
template <int C, int TT, int EL, bool GUARD, int WT = 1, bool X16 = false>
__global__ __launch_bounds__(256, (C == 128 && TT == 128 && WT == 1) ? 3 : 2) void vpair_kernel(const VPairParams p) {
    static_assert(!X16 || EL == EL_F16, "the 16-bit stream is fp16");
    const int mode = p.mode;
    if (p.K < 1) return;   // (uniform; vpair_launch refuses K < 3: the contractions assume at least one k-step, rb_common.h rb_contract)
    constexpr bool PS = !(C == 128 && TT == 128 && WT == 1);   // persistent workgroups (below); not the 3-per-CU configuration, which loses 9 % with them
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WC = 4 / WT, TW = TT / WT;     // waves over the output channels; rows of a time-wave
    constexpr int MT = (TW == 192 || TW == 96) ? 3 : (TW == 64 ? 2 : 4), NT = C / (32 * WC), MH = TW / (32 * MT), MTT = MT * MH;   // TW = 192: two passes of 3 row tiles
    typedef MfmaShape<vpair_mfma_shape(C)> SH;   // MFMA shape of both contractions; the packs come in its fragment order (vpair.h)
    typedef typename SH::acc_t acc_t;
    constexpr int PITCH = C * 2 + 16, NKG = C / SH::CI, NCT = C / 32, KGS = NCT * SH::WF * 64;   // KGS: uint4 elements of a k-step's weights
    constexpr int EP = C * 4 + 16, F4 = C / 4;
    static_assert(NCT == WC * NT && (NT == 1 || MH == 1) && WT * WC == 4, "4 waves: WT over time x WC over the output channels");
    const int tid0 = threadIdx.x;
    const int h1 = p.dil * (p.K - 1) / 2, h2 = (p.K - 1) / 2;
    const int TTe = TT - 2 * h2;             // valid output rows per tile
    const int S = p.K * NKG;
    // ---- persistent workgroups (rb_tiles.h: RbTiles): the valid tiles of the batch, ceil(len_b / TTe) per utterance, are numbered
    // through and workgroup w takes tiles w, w + G, ...; the table of the per-utterance tile counts' prefix sums and the lengths
    // live in LDS behind the tile.  A tile's stores drain while the next tile is staged, and no workgroup is launched per tile.
    const RbTiles tiles{(int*)(smem + p.pre_off), p.B};
    int total = 1, b = 0;
    if constexpr (PS) {
        tiles.build(p.lens, p.T, TTe, tid0, 256);
        total = tiles.total();
    }
#pragma unroll 1
    for (int j = PS ? blockIdx.x : 0; j < total;) {
    // the next tile: static (j + G) or, with p.tile_ctr, the next unclaimed tile of the launch (rb_tiles.h: dynamic claiming) — the
    // atomic is issued here, its result is broadcast through LDS behind the barrier that ends the tile
    unsigned claim = 0;
    if (PS && p.tile_ctr && tid0 == 0) claim = atomicAdd(p.tile_ctr, 1u);
    const int j_static = j + (int)gridDim.x;
    // (the thread index passes through an opaque move every tile: everything derived from it is then recomputed per tile — a few
    // VALU instructions — instead of being hoisted out of the tile loop by hipcc and spilled to scratch for lack of registers)
    int tid = tid0;
    if constexpr (PS) asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wc = wv / WT, wt = wv % WT;
    int len, t0;
    if constexpr (PS) {
        tiles.locate(j, b);
        len = tiles.len_of(b);
        t0 = __builtin_amdgcn_readfirstlane(tiles.first_row(j, b, TTe));
    } else {   // one tile per workgroup: grid (tiles, utterances)
        b = blockIdx.y;
        len = __builtin_amdgcn_readfirstlane(p.lens ? p.lens[b] : p.T);
        t0 = blockIdx.x * TTe;
        if (t0 >= len) return;
    }
    const long long brow = (long long)b * p.T;

    int n_ovf = 0;
    uint4 ring[SH::RD][NT * SH::WF];
    const size_t wlane = (size_t)wc * NT * SH::WF * 64 + lane;   // the wave's first co-tile
    rb_preload(ring, p.w1 + wlane, KGS);   // c1's first weights fly while the tile is staged

    // ---- stage bf16(leaky_relu(x)) for rows [t0 - h2 - h1, t0 - h2 + TT + h1) ; zero outside the utterance.
    // Buffer loads over the utterance [0, len) x C: an out-of-range row (t < 0 wraps to a huge unsigned offset,
    // t >= len exceeds num_records) returns zeros = the reference's zero padding, with no per-access compare; a thread
    // keeps its column and walks rows in steps of 8, so each access costs one v_add for its address.
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    constexpr int XB = X16 ? 2 : 4;                 // bytes per element of the input stream
    const char* xu = (const char*)p.x + brow * C * XB;
    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)xu, 0, len * C * XB, 0x00020000);
    constexpr int RSTEP = 256 / F4;                 // rows between two accesses of a thread (8)
    const int c4 = tid % F4, r0 = tid / F4;
    const int a0 = t0 - h2 - h1;
    const int arows = TT + 2 * h1;
    if constexpr (X16) {
        constexpr int F8 = C / 8, RS8 = 256 / F8;   // 8 channels (16 bytes) per access; rows between two accesses of a thread (16 / 8)
        // independent loads in flight per thread and batch.  (All 19 / 23 accesses of a tile in ONE batch — one exposed round trip instead of
        // two — shortens wave 0's staging phase and not the launch: LABNOTES round 6 (b).)
        constexpr int U = RS8 == 16 ? 10 : 12;
        const int c8 = tid % F8, r8 = tid / F8;
        const int nk = (arows + RS8 - 1) / RS8;
        const int voff0 = ((a0 + r8) * C + c8 * 8) * 2;
        char* lrow = smem + r8 * PITCH + c8 * 16;
        const int rlim = p.tile_rows - r8;      // the last pass may reach past the tile's LDS rows (the tile table lives there)
        const _Float16 hs = (_Float16)0.1f;
        const f16x2_t slope2 = {hs, hs};
        for (int kb = 0; kb < nk; kb += U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)   // (an access past the tile's rows is sent out of range: zeros, no memory traffic)
                v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, kb + u < nk ? voff0 + (kb + u) * (RS8 * C * 2) : (int)0x80000000, 0, 0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kb + u >= nk || (kb + u) * RS8 >= rlim) continue;
                u32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned w = v[u][e];   // (a scalar copy first: __builtin_bit_cast applied to a vector-element lvalue reads element 0 whatever the index)
                    const f16x2_t hv = __builtin_bit_cast(f16x2_t, w);
                    if constexpr (GUARD) {   // census: a stored value beyond the fp16 range arrives as +-inf (only the rows this tile outputs)
                        const int rr = r8 + (kb + u) * RS8 - h1 - h2;
                        if (rr >= 0 && rr < TTe)
                            n_ovf += (__builtin_fabsf((float)hv[0]) > 65504.f ? 1 : 0) + (__builtin_fabsf((float)hv[1]) > 65504.f ? 1 : 0);
                    }
                    r[e] = __builtin_bit_cast(unsigned, __builtin_elementwise_max(hv, hv * slope2));
                }
                *(u32x4*)(lrow + (kb + u) * (RS8 * PITCH)) = r;
            }
        }
    } else {
        constexpr int U = 12;                       // independent loads in flight per thread and batch
        const int nk = (arows + RSTEP - 1) / RSTEP;
        const int voff0 = ((a0 + r0) * C + c4 * 4) * 4;
        char* lrow = smem + r0 * PITCH + c4 * 8;
        for (int kb = 0; kb < nk; kb += U) {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                v[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, voff0 + (kb + u) * (RSTEP * C * 4), 0, 0);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kb + u >= nk) continue;
                const f32x4 f = __builtin_bit_cast(f32x4, v[u]);
                if constexpr (GUARD) {   // census: only the rows this tile outputs (rows outside the utterance arrive as zeros)
                    const int rr = r0 + (kb + u) * RSTEP - h1 - h2;
                    n_ovf += (rr >= 0 && rr < TTe) ? ovf4(f, 0.1f) : 0;
                }
                *(uint2*)(lrow + (kb + u) * (RSTEP * PITCH)) = act4<EL>(f, 0.1f);
            }
        }
    }
    // this lane's bias quads (channel of element e of accumulator quad q of co-tile n: (wc * NT + n) * 32 + SH::chan(lane, q) + e)
    constexpr int NBQ = 4 / SH::QB;   // distinct bias quads of a co-tile: quad q takes bb[.][q / SH::QB]
    f32x4 bb[NT][NBQ];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < NBQ; ++q) bb[n][q] = *(const f32x4*)(p.b1 + (wc * NT + n) * 32 + SH::chan(lane, q * SH::QB));
    __syncthreads();

    // ---- c1: xt rows r = 0..127  <->  global t0 - h2 + r ; reads staged rows r + tap * d
    acc_t acc[MTT][NT];
    acc_t cinit[NT];   // bias pattern of this lane's 16 channel slots: the C operand of every tile's first MFMA
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) SH::set_quad(cinit[n], q, bb[n][q / SH::QB]);
    auto load_b2 = [&]() {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < NBQ; ++q) bb[n][q] = *(const f32x4*)(p.b2 + (wc * NT + n) * 32 + SH::chan(lane, q * SH::QB));
    };
    if (NT == 1) load_b2();   // lands while c1 runs; at C = 256 its 32 registers do not fit beside c1's (spills): fetched after c1 there
    const int xlane = wt * TW * PITCH + SH::xoff(lane, PITCH);
    rb_contract<EL, MT, NT, NKG, PITCH, true, MH, SH>(acc, ring, smem, xlane, p.w1 + wlane, S, p.dil * PITCH, &cinit);
    if (NT != 1) load_b2();
    rb_preload(ring, p.w2 + wlane, KGS);
    __syncthreads();   // every wave is done reading the x tile
    // ---- bf16(leaky_relu(xt)) overwrites it (rows 0..127), zero outside the utterance
#pragma unroll
    for (int m = 0; m < MTT; ++m) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = wt * TW + m * 32 + SH::row(lane, q);
                const int t = t0 - h2 + r;
                const bool inb = t >= 0 && t < len;
                const f32x4 v4 = SH::quad(acc[m][n], q);
                uint2 pk = act4<EL>(v4, 0.1f);
                if constexpr (GUARD) n_ovf += (inb && r >= h2 && r < h2 + TTe) ? ovf4(v4, 0.1f) : 0;
                if (!inb) pk = make_uint2(0, 0);
                *(uint2*)(smem + r * PITCH + ((wc * NT + n) * 32 + SH::chan(lane, q)) * 2) = pk;
            }
    }
    __syncthreads();
    // ---- c2: output rows o = 0..127 <-> global t0 + o (valid for o < TTe) ; reads xt rows o + tap
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int q = 0; q < 4; ++q) SH::set_quad(cinit[n], q, bb[n][q / SH::QB]);
    rb_contract<EL, MT, NT, NKG, PITCH, true, MH, SH>(acc, ring, smem, xlane, p.w2 + wlane, S, PITCH, &cinit);
    __syncthreads();   // the xt tile is dead: the staging buffer of the epilogue aliases it

    if constexpr (GUARD) {
        if (n_ovf) atomicAdd(p.ovf, (unsigned long long)n_ovf);   // (output rows only: every in-utterance row exactly once per launch)
    }
    // ---- epilogue: 32-row slabs through LDS, whole rows out; residual x re-read (L2), xs accumulated per mode.
    // Buffer loads / stores again: rows >= len are dropped by the range check, the garbage rows o >= TTe of the last
    // slab are sent out of range explicitly.  The reads of slab m+1 are issued before slab m is processed.
    constexpr int PER = WT * 32 * F4 / 256;     // a pass moves one 32-row slab of every time-wave
    float* yu = p.y + brow * C;
    // (p.y16, mode 1 only: the result leaves as fp16 — the next iteration's X16 input; same rows, half the bytes)
    const auto rs_y = p.y16 ? __builtin_amdgcn_make_buffer_rsrc((void*)((char*)p.y + brow * C * 2), 0, len * C * 2, 0x00020000)
                            : __builtin_amdgcn_make_buffer_rsrc((void*)yu, 0, len * C * 4, 0x00020000);
    const auto rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.ya ? p.ya + brow * C : (unsigned short*)yu), 0, len * C * 2, 0x00020000);
    const int eoff0 = (t0 * C + c4 * 4) * 4;
    auto eoff = [&](int m, int u) {                 // byte offset of (slab m, access u) or out of range
        const int sr = u * RSTEP + r0;              // staged row: slab m of time-wave sr / 32
        const int o = (sr >> 5) * TW + m * 32 + (sr & 31);
        return o < TTe ? eoff0 + o * (C * 4) : (int)0x80000000;
    };
    // The residual rows (and, modes 2 / 3, the stage sum) of a slab are requested XD - 1 (SD - 1) slabs ahead: one slab at C = 128, none at
    // C = 256 (registers).  Round 6 stamps had this epilogue at 34 k cycles of a 90 k-cycle tile at C = 128 — a chain of exposed round trips; a
    // lookahead of 3 - 5 slabs (an fp16 row costs half the registers) shortens wave 0's phase by 27 - 40 % and leaves every
    // launch where it was (the co-resident workgroup fills the gaps either way): the shallow ring stays.  LABNOTES round 6 (b).
    constexpr int XD = NT == 1 ? 2 : 1, SD = XD;
    static_assert(XD <= MTT, "the lookahead ring is no deeper than the tile has slabs");
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    typedef typename std::conditional<X16, u32x2, u32x4>::type xrow_t;
    xrow_t xin[XD][PER];
    u32x4 sold[SD][PER];
    auto fetch_x = [&](int m, xrow_t (&xi)[PER]) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int off = eoff(m, u);
            if constexpr (X16) xi[u] = __builtin_amdgcn_raw_buffer_load_b64(rs_x, off == (int)0x80000000 ? off : off >> 1, 0, VP_XI_AUX);
            else xi[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, VP_XI_AUX);
        }
    };
    auto fetch_s = [&](int m, u32x4 (&so)[PER]) {
        // (mode 1 never reads them; defined here all the same: left undefined, the register allocator keeps a value for them alive from the top of
        // the tile through both contractions — 16 / 32 registers, spilled in the largest instantiations)
#pragma unroll
        for (int u = 0; u < PER; ++u) so[u] = mode < 2 ? u32x4{0, 0, 0, 0} : __builtin_amdgcn_raw_buffer_load_b128(rs_y, eoff(m, u), 0, VP_LD_AUX);
    };
#pragma unroll
    for (int m = 0; m < XD - 1; ++m) fetch_x(m, xin[m]);
#pragma unroll
    for (int m = 0; m < SD - 1; ++m) fetch_s(m, sold[m]);
#pragma unroll
    for (int m = 0; m < MTT; ++m) {
        if (m) __syncthreads();
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *(f32x4*)(smem + (wt * 32 + SH::row(lane, q)) * EP + ((wc * NT + n) * 32 + SH::chan(lane, q)) * 4) = SH::quad(acc[m][n], q);
        if (m + XD - 1 < MTT) fetch_x(m + XD - 1, xin[(m + XD - 1) % XD]);
        if (m + SD - 1 < MTT) fetch_s(m + SD - 1, sold[(m + SD - 1) % SD]);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int off = eoff(m, u);
            f32x4 xr;
            if constexpr (X16) {
                const unsigned w0 = xin[m % XD][u][0], w1 = xin[m % XD][u][1];   // (scalar copies: see the staging loop)
                const f16x2_t g0 = __builtin_bit_cast(f16x2_t, w0), g1 = __builtin_bit_cast(f16x2_t, w1);
                xr = f32x4{(float)g0[0], (float)g0[1], (float)g1[0], (float)g1[1]};
            } else xr = __builtin_bit_cast(f32x4, xin[m % XD][u]);
            f32x4 o = *(const f32x4*)(smem + (r0 + u * RSTEP) * EP + c4 * 16) + xr;   // x = xt + x
            if (mode >= 2) o += __builtin_bit_cast(f32x4, sold[m % SD][u]);                                                 // xs += x
            if (mode == 3) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = o[e] / p.div;
            }
            if (p.y16) {   // (no saturation: a value beyond the fp16 range is stored as +-inf, reaches conv_post as a non-finite sum: the always-on detector)
                const u32x2 pk = {pack2<EL_F16>(o[0], o[1]), pack2<EL_F16>(o[2], o[3])};
                __builtin_amdgcn_raw_buffer_store_b64(pk, rs_y, off == (int)0x80000000 ? off : off >> 1, 0, VP_ST_AUX);
            } else if (!(mode == 3 && p.ya && p.drop_y))   // the stage's consumers read only the bf16 copy
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_y, off, 0, VP_ST_AUX);
            if (mode == 3 && p.ya) {
                const u32x2 pk = {pack2bf(lrelu(o[0], p.slope), lrelu(o[1], p.slope)), pack2bf(lrelu(o[2], p.slope), lrelu(o[3], p.slope))};
                __builtin_amdgcn_raw_buffer_store_b64(pk, rs_a, off == (int)0x80000000 ? off : off >> 1, 0, VP_ST_AUX);
            }
        }
    }
    if constexpr (!PS) break;
    if (p.tile_ctr && tid0 == 0) tiles.publish_claim((int)gridDim.x, claim);
    __syncthreads();   // the epilogue's staging rows alias the tile the next iteration stages into
    j = p.tile_ctr ? tiles.claimed() : j_static;
    }   // (tiles of this workgroup)
}

bool vpair_supported(int C, int K, int dil) {
    return (C == 128 || C == 256) && (K & 1) && K >= 3 && K <= 11 && dil >= 1 && dil <= 5;
}

template <int CC, int TT, int EL, bool GUARD = false, int WT = 1, bool X16 = false>
static hipError_t vpair_launch_tt(const VPairParams& p, hipStream_t stream) {
    if constexpr (EL == EL_F16 && !X16) {
        if (p.x16) return vpair_launch_tt<CC, TT, EL, GUARD, WT, true>(p, stream);
    }
    if ((p.x16 && !X16) || (p.y16 && (EL != EL_F16 || p.mode != 1))) return hipErrorInvalidValue;
    if ((long long)p.T * CC * 4 >= (1LL << 31)) return hipErrorInvalidValue;   // 32-bit byte offsets inside an utterance's buffer resource
    if constexpr (EL == EL_F16 && !GUARD) {
        // the census (GUARD) instantiation of the same configuration.  C = 256: 96-row tiles where the release path takes 128-row ones — the
        // guarded 128-row kernel does not fit 256 VGPRs on MfmaShape<16> (41 spilled) and is never instantiated.  The shape is fixed per
        // width and the census counts over the rows each tile OUTPUTS (every in-utterance row once per launch), so neither an output bit
        // nor the count depends on the tile size; a 96-row tile needs less LDS than the 128-row one, so whatever fits there fits here.
        if (p.ovf) return vpair_launch_tt<CC, (CC == 256 && TT == 128) ? 96 : TT, EL, true, WT, X16>(p, stream);
    }
    constexpr int PITCH = CC * 2 + 16;
    const int h1 = p.dil * (p.K - 1) / 2, h2 = (p.K - 1) / 2;
    const int TTe = TT - 2 * h2;
    // staged rows, rounded up to the staging loop's step, or one spare tap for c1's activation prefetch, whichever reaches further;
    // the xt phase needs TT + (K-1) + 1 rows, the epilogue 32 fp32 rows
    constexpr int RSTEP = 256 / (CC / 4);
    size_t rows = (size_t)TT + 2 * h1 + std::max(p.dil + 1, RSTEP);
    if (rows < (size_t)TT + p.K + 1) rows = TT + p.K + 1;
    size_t lds = rows * PITCH;
    const size_t ep = (size_t)WT * 32 * (CC * 4 + 16);
    if (ep > lds) lds = ep;
    VPairParams q = p;
    q.tile_rows = (int)rows;
    q.pre_off = (int)lds;                          // the tile table (rb_tiles.h) lies behind the tile
    constexpr bool PS = !(CC == 128 && TT == 128 && WT == 1);
    if (PS) lds += rb_table_bytes(p.B);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    constexpr auto kern = vpair_kernel<CC, TT, EL, GUARD, WT, X16>;
    if (const hipError_t e = rb_allow_full_lds<kern>(); e != hipSuccess) return e;
    if (!PS) {
        hipLaunchKernelGGL(kern, dim3((p.T + TTe - 1) / TTe, p.B), dim3(256), lds, stream, q);
        return hipGetLastError();
    }
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    // (by registers: the kernel's launch bound, two workgroups per CU for every persistent instantiation)
    const int grid = rb_resident_grid(cus, lds, 256, 2, (long long)p.B * ((p.T + TTe - 1) / TTe));
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, q);
    return hipGetLastError();
}

template <int EL>
static hipError_t vpair_launch_el(const VPairParams& p, int C, hipStream_t stream) {
    // small batches (B = 1: one sentence): the default tiles would leave most CUs without one and the launch takes as long as ONE tile
    // -> half-size tiles (more halo rows recomputed, twice the weight stream per row, but twice the CUs at work)
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    auto tiles_of = [&](int tt) { return (long long)p.B * ((p.T + (tt - (p.K - 1)) - 1) / (tt - (p.K - 1))); };
    if (C == 256) {
        if (2 * tiles_of(128) <= cus) return vpair_launch_tt<256, 64, EL>(p, stream);
        // 128-row tiles, or 96-row ones where only those leave room for TWO workgroups per CU (one workgroup = one wave per SIMD exposes
        // every latency of the memory phases: k = 7 with dilation 5, k = 11 with dilation 3)
        auto lds_of = [&](int tt) { return ((size_t)tt + (size_t)p.dil * (p.K - 1) + std::max(p.dil + 1, 4)) * (256 * 2 + 16) + rb_table_bytes(p.B); };
        if (2 * lds_of(128) > 160 * 1024 && 2 * lds_of(96) <= 160 * 1024) return vpair_launch_tt<256, 96, EL>(p, stream);
        return vpair_launch_tt<256, 128, EL>(p, stream);
    }
    // 256-row tiles while two workgroups still fit a CU's 160 KB of LDS (all but k = 11 with dilation 5)
    const size_t rows256 = (size_t)256 + (size_t)p.dil * (p.K - 1) + std::max(p.dil + 1, 8);
    const bool big = (rows256 * (128 * 2 + 16) + rb_table_bytes(p.B)) * 2 <= 160 * 1024;
    if (2 * tiles_of(256) <= cus) return vpair_launch_tt<128, 128, EL>(p, stream);
    if (big) return vpair_launch_tt<128, 256, EL>(p, stream);
    // k = 11 with dilation 5: 192-row tiles (two workgroups per CU, persistent) instead of 128-row ones (three, one tile each)
    return vpair_launch_tt<128, 192, EL>(p, stream);
}

hipError_t vpair_launch(const VPairParams& p, int C, hipStream_t stream) {
    if (!vpair_supported(C, p.K, p.dil)) return hipErrorInvalidValue;
    return p.el == EL_F16 ? vpair_launch_el<EL_F16>(p, C, stream) : vpair_launch_el<EL_BF16>(p, C, stream);
}

} // namespace dtts
