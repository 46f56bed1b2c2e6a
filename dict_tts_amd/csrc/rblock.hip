// Fused HifiGAN ResBlock1 (modules/hifigan/hifigan.py:27-58), 16-bit MFMA: every k at C = 64 / 32, k = 3 at C = 128 / 256.
// The MFMA instruction is a per-width choice (rblock.h: rblock_mfma_shape; rb_common.h: MfmaShape): the kernel is written against the trait.
//
// Unfused, a ResBlock is six convolutions that each stream the whole activation through HBM; at C <= 64 their
// arithmetic intensity (C*k/2 FLOP/B) is far below the MFMA/HBM ridge, i.e. the vocoder's last two stages (36 % of
// its FLOPs) are HBM-bound.  Here one workgroup keeps a time tile resident for all six convolutions:
//   * the fp32 residual stream x lives in REGISTERS in MFMA accumulator layout (D[co][t]),
//   * the bf16 leaky_relu copy that feeds the next convolution lives in ONE LDS buffer (A and the intermediate
//     xt time-share it: conv reads -> barrier -> overwrite -> barrier),
//   * weights stream from L2 through a register ring of SH::RD k-steps (22..90 KB per conv, shared by every workgroup),
//   * the tile carries a halo of 6*(k-1) rows per side (sum of the six receptive half-widths at dilations (1, 3, 5); more
//     for larger dilations: rblock_halo) that is recomputed;
//     rows outside the utterance are forced to zero after every activation = the reference's zero padding.
// HBM traffic per ResBlock drops from ~9 passes to: read x once, read-modify-write the stage accumulator once.
// PS = 1 (all but C = 32): persistent workgroups walk the batch's valid tiles, the next tile's x is fetched straight into the
// residual registers (accumulator layout, no LDS transposition) slab by slab as the epilogue releases them.
#include "rblock.h"
#include "rb_common.h"
#include "rb_tiles.h"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace dtts {

#ifdef RB_STAMP   // per-phase clock stamps (tools/rb_stamps.py; a variant build, never the release library): sums over the tiles of every workgroup,
                  // wave 0 (table 0) and the last wave (table 1), one row per (C, k): s_memrealtime ticks of 10 ns
__device__ unsigned long long rb_stamps[2][12][16];
extern "C" __attribute__((visibility("default"))) int dtts_debug_rb_stamps(unsigned long long* host, int reset) {
    hipError_t e = hipMemcpyFromSymbol(host, HIP_SYMBOL(rb_stamps), sizeof(rb_stamps));
    if (e == hipSuccess && reset) {
        static unsigned long long z[2][12][16];
        e = hipMemcpyToSymbol(HIP_SYMBOL(rb_stamps), z, sizeof z);
    }
    return (int)e;
}
#define RB_T(k) do { const unsigned long long _n = __builtin_amdgcn_s_memrealtime(); tq[k] += _n - t_last; t_last = _n; } while (0)
#else
#define RB_T(k)
#endif

// (leaky_relu(x) and leaky_relu(xt) time-share ONE LDS buffer.  The form with a buffer each — two workgroup barriers per iteration instead of four —
// was slower: LABNOTES (O), tools/experiments/rblock_two_buffers.patch)
// SH: the MFMA shape of every contraction of the kernel (rb_common.h MfmaShape; rblock.h rblock_mfma_shape picks it per width): all row / channel
// arithmetic of the accumulator layout goes through its helpers, and the packs arrive in its fragment order.
template <int C, int MT, int NT, int WT, int WC, int EL, int PS, bool GUARD, class SH = MfmaShape<32>>
__global__ __launch_bounds__(64 * WT * WC, (64 * WT * WC <= 256) ? 2 : 1) void rblock_kernel(const RBlockParams p) {
    static_assert(WC * NT * 32 == C, "channel tiling must cover C");
    typedef typename SH::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int THREADS = 64 * WT * WC;
    constexpr int W = 32 * MT * WT;
    constexpr int PITCH = C * 2 + 16;
    constexpr int NKG = C / SH::CI;
    // (the contractions keep ONE activation-fragment set, rb_common.h: with a double buffer the 640-row C = 64 instantiation sat at 256 VGPRs with 13 of
    // them spilled; the single set takes 249 and spills nothing.  LABNOTES round 5 (Y))
    constexpr int EP = C * 4 + 16;                 // fp32 staging row
    constexpr int F4 = C / 4, SROWS = WT * 32;
    constexpr size_t ACT_BYTES = (size_t)(W + 2 * RB_GUARD) * PITCH;
    char* act = smem;                                    // leaky_relu(x), then leaky_relu(xt): time-shared
    char* stage = smem + ACT_BYTES;                      // epilogue transposition

    // per-thread coordinates; PS refreshes them through an opaque move at every tile (see the tile loop)
    int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int wt = wave % WT, wc = wave / WT;
    const int H = rblock_halo(p);
    const int TT = W - 2 * H;
    // fused conv_post (p.wav): the tile's TT valid rows give TT - (PK - 1) output samples, so tiles step by that and start
    // (PK - 1) / 2 rows early
    constexpr int PK = 7, PH = (PK - 1) / 2;
    const int TTo = p.wav ? TT - 2 * PH : TT;

    // ---- persistent workgroups.  The valid tiles of the batch (ceil(len_b / TTo) per utterance) are numbered through, workgroup w
    // takes tiles w, w + G, w + 2G, ...: a table of the per-utterance tile counts' prefix sums lives in LDS.  While a tile is
    // computed the NEXT tile's residual stream is already on its way into registers, so the exposed HBM round trip and the
    // LDS transposition of a per-tile x load disappear from every tile but the workgroup's first.
    const RbTiles tiles{(int*)(smem + p.pre_off), p.B};
    // zero the guard bands (once; the fused conv_post's fp32 output tile aliases them: again after every tile there)
    auto zero_guard_bands = [&](int t) {
        for (int idx = t; idx < 2 * RB_GUARD * (PITCH / 16); idx += THREADS) {
            const int r = idx / (PITCH / 16), c = idx % (PITCH / 16);
            const int row = r < RB_GUARD ? r : W + r;
            *(uint4*)(act + row * PITCH + c * 16) = make_uint4(0, 0, 0, 0);
        }
    };
    zero_guard_bands(tid);
    int total = 0, j = blockIdx.x;
    if constexpr (PS) {
        tiles.build(p.lens, p.T, TTo, tid, THREADS);
        total = tiles.total();
        if (j >= total) return;
    }
    const int G = gridDim.x;

    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    constexpr int RPP = THREADS / F4;              // rows one cooperative access of the workgroup covers (32 at C <= 64, 16 at C >= 128)
    constexpr int PER = SROWS / RPP;               // accesses per staging pass of SROWS = 32 rows per time-wave
    static_assert(THREADS % F4 == 0 && SROWS % RPP == 0, "row-coalesced staging");
    int c4 = tid % F4, r0 = tid / F4;   // r0 in [0, RPP)
    // staged row s = r0 + RPP * u of pass m <-> tile row: 32-row slab m of time-wave s / 32
    auto tile_row = [&](int m, int u) { const int sr = r0 + RPP * u; return ((sr >> 5) * MT + m) * 32 + (sr & 31); };

    // the residual stream of a tile, fp32, straight into accumulator layout (quad q of a lane = 4 consecutive channels of row SH::row(lane, q): one
    // 16 B access.  An access of the wave covers 32 rows x 32 contiguous bytes on MfmaShape<32>, 16 rows x 64 on MfmaShape<16>).
    // Buffer loads over the utterance [0, len) x C return zeros for rows outside it (t < 0 wraps to a huge unsigned offset) = the zero padding.
    // (row / chan are a lane part plus a quad part in both shapes: the quad part is an immediate offset of the access)
    auto load_x = [&](acc_t (&d)[NT], int m, int bb, int base, int ln) {   // 32-row slab m of this wave
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (long long)bb * p.T * C), 0, ln * C * 4, 0x00020000);
        const int o0 = ((base + wt * MT * 32 + SH::row(lane, 0)) * C + wc * NT * 32 + SH::chan(lane, 0)) * 4;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o0 + (m * 32 * C + n * 32 + SH::row(0, q) * C + SH::chan(0, q)) * 4, 0, RB_X_AUX);
                SH::set_quad(d[n], q, __builtin_bit_cast(f32x4, v));
            }
    };

    int b = 0, len, t0;
    if constexpr (PS) {
        tiles.locate(j, b);
        len = tiles.len_of(b);
        t0 = tiles.first_row(j, b, TTo) - (p.wav ? PH : 0);
    } else {   // one tile per workgroup: grid (tiles, utterances)
        b = blockIdx.y;
        // (readfirstlane: hipcc loads lens[b] with a vector load — the kernel also stores through other pointers, so no scalar load)
        len = __builtin_amdgcn_readfirstlane(p.lens ? p.lens[b] : p.T);
        t0 = blockIdx.x * TTo - (p.wav ? PH : 0);
        if (t0 + (p.wav ? PH : 0) >= len) return;
    }
    acc_t xr[MT][NT];
    if constexpr (PS) {
#pragma unroll
        for (int m = 0; m < MT; ++m) load_x(xr[m], m, b, t0 - H, len);
    } else {
        // one tile per workgroup (C = 32): coalesced whole-row loads, transposed into accumulator layout through the staging buffer
        // (the 32 B per row and instruction of the direct form cost 3 % at C = 32).  All MT*PER 16 B loads of a thread are issued
        // before the first LDS round trip: one exposed HBM latency per tile.
        const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (long long)b * p.T * C), 0, len * C * 4, 0x00020000);
        const int g0 = ((t0 - H + r0) * C + c4 * 4) * 4;
        u32x4 ld[MT][PER] = {};   // (every element is loaded below; without the initialiser hipcc schedules the GUARD instantiation differently)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int u = 0; u < PER; ++u) ld[m][u] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, g0 + (tile_row(m, u) - r0) * (C * 4), 0, RB_X_AUX);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m) __syncthreads();
#pragma unroll
            for (int u = 0; u < PER; ++u) *(u32x4*)(stage + (r0 + RPP * u) * EP + c4 * 16) = ld[m][u];
            __syncthreads();
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    SH::set_quad(xr[m][n], q, *(const f32x4*)(stage + (wt * 32 + SH::row(lane, q)) * EP + ((wc * NT + n) * 32 + SH::chan(lane, q)) * 4));
        }
    }

    const int kg_stride = (C / 32) * SH::WF * 64;   // uint4 elements of a k-step's weights
    // work items of a workgroup: (tile, ResBlock r) — r runs over the launch's p.nrb ResBlocks on the SAME tile before the next tile
    int r = 0;

#ifdef RB_STAMP
    unsigned long long tq[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_last = __builtin_amdgcn_s_memrealtime();
#endif
#pragma unroll 1
    for (;;) {
    if constexpr (PS) {
        // the thread index passes through an opaque move every tile: everything derived from it is recomputed per tile (a few VALU
        // instructions) instead of being hoisted out of the tile loop by hipcc and spilled to scratch for lack of registers
        tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        wt = wave % WT, wc = wave / WT;
        c4 = tid % F4, r0 = tid / F4;
    }
    const int xlane = (RB_GUARD + wt * MT * 32 + SH::row(lane, 0)) * PITCH + SH::chan(lane, 0) * 4;
    const size_t wlane = (size_t)(wc * NT) * SH::WF * 64 + lane;
    if constexpr (PS) r = __builtin_amdgcn_readfirstlane(r);
    else r = 0;                                      // (one tile per workgroup: one ResBlock per launch)
    const RBlockParams::Set& R = p.rb[PS ? r : 0];
    const int Kr = R.K;                              // this ResBlock's kernel size (the tile's halo follows the launch's largest)
    // C = 32 (two k-groups per tap): the packs' zero padding to a multiple of four steps would be 25 / 12.5 / 8 % of the MFMAs at k = 3 / 7 / 11:
    // those configurations run the real steps only (rb2_contract, uniform exit at tap boundaries)
    constexpr bool REAL_STEPS = (C == 32);
    static_assert(!REAL_STEPS || SH::FRAG == 32, "rb2_contract is written for 32x32x16");
    static_assert(REAL_STEPS || NKG >= 4 || (NKG == 2 && SH::FRAG == 16), "whole groups of four k-steps, or rb_contract's half group");
    const int S = (REAL_STEPS ? Kr : R.Kp) * NKG;   // k-steps (packed taps are zero padded so that Kp * NKG % 4 == 0)
    const bool last_rb = !PS || r + 1 == p.nrb;
    // what the epilogue does with the stage sum: one ResBlock per launch: p.mode; all of the stage's: write, accumulate.., finish
    const int mode = (!PS || p.nrb == 1 || r == 0) ? p.mode : (last_rb ? p.last_mode : 1);
    const bool wav_now = p.wav && last_rb;           // (the launcher accepts p.wav only on a launch that ends its stage: last_mode 2)
    t0 = __builtin_amdgcn_readfirstlane(t0);
    const int base_t = t0 - H;  // global time of local row 0
    const long long brow = (long long)b * p.T;
    // the workgroup's next tile
    // the workgroup's next tile: static (j + G), or — p.tile_ctr — DYNAMIC: the next unclaimed tile of the launch, taken from a
    // device counter (tiles 0 .. G-1 are the workgroups' first tiles, the counter hands out G, G+1, ...).  Workgroups slowed down by
    // whatever shares their CU (the next batch's text->mel kernels on the other stream, a neighbour's phase) then simply take fewer
    // tiles instead of setting the launch's finish time.  One lane issues the atomic at the top of the tile; its result is not
    // needed before the epilogue (the x prefetch), where it is broadcast through LDS behind a barrier that exists anyway.
    unsigned claim = 0;
    if (PS && p.tile_ctr && tid == 0 && last_rb) claim = atomicAdd(p.tile_ctr, 1u);
    int jn = j + G;
    bool has_next = PS && jn < total;
    int bn = b, lenn = len, t0n = 0;
    auto plan_next = [&]() {
        if (!last_rb) {                              // the same tile again, for the stage's next ResBlock
            has_next = true;
            jn = j;
            bn = b;
            lenn = len;
            t0n = t0;
            return;
        }
        has_next = PS && jn < total;
        bn = b;
        if (has_next) {
            tiles.locate(jn, bn);
            lenn = tiles.len_of(bn);
            t0n = tiles.first_row(jn, bn, TTo) - (p.wav ? PH : 0);
        }
    };
    if (!(PS && p.tile_ctr) || !last_rb) plan_next();
    // the stage sum: [B][T][C] like x — or, p.s_private (all ResBlocks in one launch WITH the fused conv_post, whose tiles overlap by
    // 2 PH rows): a private strip of TT rows per tile, so that no two workgroups read-modify-write the same rows
    const auto rs_s = p.s_private ? __builtin_amdgcn_make_buffer_rsrc((void*)p.S, 0, p.s_private, 0x00020000)
                                  : __builtin_amdgcn_make_buffer_rsrc((void*)(p.S + brow * C), 0, len * C * 4, 0x00020000);

    // bf16(leaky_relu(v + bias, 0.1)) of this wave's tiles -> LDS activation buffer, zero outside the utterance.
    // bias: this lane's distinct channel quads per co-tile (accumulator quad q takes bb[.][q / SH::QB]: on MfmaShape<16> the two row halves
    // share their channels), loaded into registers BEFORE the contraction it follows.
    constexpr int NBQ = 4 / SH::QB;
    auto load_bias = [&](f32x4 (&bb)[NT][NBQ], const float* bias) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < NBQ; ++q) bb[n][q] = *(const f32x4*)(bias + (wc * NT + n) * 32 + SH::chan(lane, q * SH::QB));
    };
    const bool all_inb = base_t >= 0 && base_t + W <= len;   // block-uniform: no row of the tile needs masking
    int n_ovf = 0;
    // MASKED = false: a tile wholly inside its utterance (block-uniform, most tiles) — no row needs the zero select: 2 of the ~11 VALU
    // instructions per four values less, in the phase that is VALU-bound (LABNOTES round 4 (C))
    auto write_act_impl = [&](char* dst, const acc_t (&v)[MT][NT], auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        // (MfmaShape<16>: the lane index passes through an opaque move at every rewrite.  A lane has two rows per slab there, and hipcc otherwise keeps
        // the 2 MT rows' masks and LDS addresses — the same in all six rewrites of a tile — alive through the contractions: spills at MT = 5)
        int ln = lane;
        if constexpr (SH::FRAG == 16) asm volatile("" : "+v"(ln));
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            // the row of a quad: one per lane on MfmaShape<32>, one per row half (SH::QB quads) on MfmaShape<16>
            int row[SH::QB];
            bool inb[SH::QB], counted[SH::QB];
#pragma unroll
            for (int rh = 0; rh < SH::QB; ++rh) {
                row[rh] = (wt * MT + m) * 32 + SH::row(ln, rh);
                const int t = base_t + row[rh];
                inb[rh] = !MASKED || (t >= 0 && t < len);
                // range guard: only the rows this tile OUTPUTS are counted.  Every in-utterance row is an output row of exactly one tile
                // and carries the exact activation there at each of the six stages, so the count is a census; halo rows (recomputed,
                // increasingly inexact towards the tile edge, their results discarded) are another tile's output rows.
                counted[rh] = inb[rh] && row[rh] >= H && row[rh] < H + TT;
            }
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    constexpr int QBM = SH::QB - 1;   // (quad q's row half: q % SH::QB)
                    const int co = (wc * NT + n) * 32 + SH::chan(ln, q);
                    const f32x4 v4 = SH::quad(v[m][n], q);
                    uint2 pk = act4<EL>(v4, 0.1f);
                    if constexpr (GUARD) n_ovf += counted[q & QBM] ? ovf4(v4, 0.1f) : 0;
                    if constexpr (MASKED) {
                        if (!inb[q & QBM]) pk = make_uint2(0, 0);
                    }
                    *(uint2*)(dst + (RB_GUARD + row[q & QBM]) * PITCH + co * 2) = pk;
                }
        }
    };
    auto write_act = [&](char* dst, const acc_t (&v)[MT][NT]) {
        if (all_inb) write_act_impl(dst, v, std::false_type{});
        else write_act_impl(dst, v, std::true_type{});
    };

    uint4 ring[SH::RD][NT * SH::WF];
    f32x4 bb[NT][NBQ];   // one live bias set
    RB_T(10);                                            // (tile bookkeeping, and — the first tile — the wait for x)
    rb_preload(ring, R.w1[0] + wlane, kg_stride);       // in flight during the first activation write
    load_bias(bb, R.b1[0]);
    write_act(act, xr);
    RB_T(0);
    __syncthreads();
    RB_T(1);

    acc_t acc[MT][NT];
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        // conv1: the first MFMA of every tile takes the bias pattern as its C operand (no accumulator init pass)
        acc_t cinit[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) SH::set_quad(cinit[n], q, bb[n][q / SH::QB]);
        load_bias(bb, R.b2[it]);       // lands while conv1 runs
        const int d = R.dil[it];
        if constexpr (REAL_STEPS) {
            // S > 0 always, which the compiler cannot know.  The two tests on S and the S == 0 arm (acc = cinit, by way of rb_contract) stay: without them,
            // or with the arm written out, hipcc allocates the C = 32 kernels' registers differently (LABNOTES: retired switches)
            if (S) rb2_contract<EL, MT, NT, NKG, PITCH, 4, true>(acc, ring, act, xlane - ((Kr - 1) / 2) * d * PITCH, R.w1[it] + wlane, S, d * PITCH, cinit);
            else rb_contract<EL, MT, NT, NKG, PITCH, true, 1>(acc, ring, act, 0, R.w1[it] + wlane, 0, 0, &cinit);
        } else
            rb_contract<EL, MT, NT, NKG, PITCH, true, 1, SH>(acc, ring, act, xlane - ((Kr - 1) / 2) * d * PITCH, R.w1[it] + wlane, S, d * PITCH, &cinit);
        rb_preload(ring, R.w2[it] + wlane, kg_stride);   // next conv's first weights fly during barrier + write
        RB_T(2);
        __syncthreads();               // every wave is done reading A
        RB_T(3);
        write_act(act, acc);           // xt (16-bit, activated): overwrites A
        RB_T(4);
        __syncthreads();
        RB_T(5);
        // conv2 accumulates straight into the residual registers: x = x + b2 + W2 * xt
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int q = 0; q < 4; ++q) SH::add_quad(xr[m][n], q, bb[n][q / SH::QB]);
        if (it < 2) load_bias(bb, R.b1[it + 1]);
        if constexpr (REAL_STEPS) {
            if (S) rb2_contract<EL, MT, NT, NKG, PITCH, 4, false>(xr, ring, act, xlane - ((Kr - 1) / 2) * PITCH, R.w2[it] + wlane, S, PITCH, cinit);
        } else
            rb_contract<EL, MT, NT, NKG, PITCH, false, 1, SH>(xr, ring, act, xlane - ((Kr - 1) / 2) * PITCH, R.w2[it] + wlane, S, PITCH);
        if (it < 2) rb_preload(ring, R.w1[it + 1] + wlane, kg_stride);
        if (PS && p.tile_ctr && last_rb && it == 2 && tid == 0) tiles.publish_claim(G, claim);   // the claimed tile, for everyone (read behind the barrier)
        RB_T(6);
        __syncthreads();               // every wave is done reading xt
        RB_T(7);
        if (it < 2) {
            write_act(act, xr);
            RB_T(0);
            __syncthreads();
            RB_T(1);
        }
    }

    if (PS && p.tile_ctr && last_rb) {
        jn = tiles.claimed();
        plan_next();
    }
    {
    // ---- epilogue: rows [H, H+TT) of the tile leave as whole rows through the fp32 staging buffer; the old
    // accumulator values (xs += ...) of all MT passes are fetched up front.  Buffer ops: rows >= len are dropped by the
    // range check, halo rows are sent out of range explicitly.
    const auto rs_a = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Sa ? p.Sa + brow * C : (unsigned short*)(p.S + brow * C)), 0,
                                                        len * C * 2, 0x00020000);
    // WAVE-PRIVATE transposition: each wave stages its own 32 rows x its own CW channels and reads the same block back as whole 128-byte
    // row segments (8 NT lanes per row): no workgroup barrier inside the epilogue (round 3: 2 MT - 1 of them), the waves drift through their
    // slabs and HBM round trips independently.  (The LDS serves one wave's accesses in order.)
    constexpr int CW = NT * 32, F4W = CW / 4, RPI = 64 / F4W, NRD = 32 / RPI;
    const int er = lane / F4W, ec = lane % F4W;                          // lane octet (one row per octet and access), 16-byte chunk of the wave's row segment
    const int goffw = (p.s_private ? (j * TT - H) * C : base_t * C) * 4 + (wc * CW + ec * 4) * 4;
    // Which of the slab's 32 rows an octet reads in access u.  Consecutive rows (u * 8 + er: rounds 3 - 5) put the 16-lane groups of a ds_read_b128
    // ({0-3, 12-15, 20-27}, ...) on overlapping 16-byte slots of the 256-byte bank row — 3-way at C >= 64, 2-way at C = 32: 12 / 8 LDS cycles per read instead
    // of 4, a quarter of the kernels' bank-conflict cycles (round 6: LABNOTES (c6), profiles/r06_lds_conflict_attrib.txt; the model reproduces the counter to 1 %).  Rows
    // base + {0, 16, 8, 24} for the four octets of a half-wave (base = 2 u + half) spread every group over all 16 slots for each row pitch in use (9 / 17 / 33 / 65
    // slots): conflict-free; an octet still moves one whole 128-byte row segment, so the global accesses coalesce as before.  Same values, same order per row.
    static_assert(F4W == 8 && RPI == 8 && NRD == 4, "the conflict-free row order below is for 8 lanes per row, 8 rows per access");
    // (C = 32 keeps consecutive rows: a row is 128 bytes there, so an access of 8 consecutive rows is ONE contiguous kilobyte of the stage sum — worth more than
    // the 4 LDS cycles: +1.1 % on both C = 32 launches with the permuted order, same box)
    const int erow_slab_base = C == 32 ? er : (er >> 2) + ((er & 1) ? 16 : 0) + ((er & 2) ? 8 : 0);
    auto srow = [&](int u) { return (C == 32 ? 8 : 2) * u + erow_slab_base; };                // row of the 32-row slab
    auto erow = [&](int m, int u) { return (wt * MT + m) * 32 + srow(u); };                   // local tile row of (slab m, access u)
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
            // (all ResBlocks in one launch: the sum was written by THIS workgroup a moment ago and sits in L2 / Infinity Cache: a cached read)
            if (mode >= 1) sold[m][u] = p.nrb > 1 ? __builtin_amdgcn_raw_buffer_load_b128(rs_s, eoff(m, u), 0, 0)
                                                  : __builtin_amdgcn_raw_buffer_load_b128(rs_s, eoff(m, u), 0, VP_LD_AUX);
        }
    RB_T(12);                                            // (epilogue: plan + stage-sum loads issued)
    // fused conv_post: the stage output leaky_relu(xs / num_kernels) stays in LDS as an fp32 tile ([TT rows][C], rows outside
    // the utterance zero = conv_post's zero padding) instead of going to HBM; the transposition buffer moves behind it
    constexpr int OP = C * 4;                      // otile row pitch (bytes)
    char* otile = smem;
    char* estage = wav_now ? smem + ((size_t)TT * OP > ACT_BYTES ? (size_t)TT * OP : ACT_BYTES) : stage;
    char* stg = estage + (wt * 32) * EP + (wc * CW) * 4;                 // this wave's block of the staging buffer
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) *(f32x4*)(stg + SH::row(lane, q) * EP + (n * 32 + SH::chan(lane, q)) * 4) = SH::quad(xr[m][n], q);
        // slab m of the residual registers is free: the NEXT tile's slab m starts its trip into them (no second register set, and
        // the loads are younger than the stage sum fetched above, so nothing below waits for them)
        if (has_next) load_x(xr[m], m, bn, t0n - H, lenn);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        RB_T(13);                                        // (slab: accumulators -> staging rows, next tile's loads issued)
#pragma unroll
        for (int u = 0; u < NRD; ++u) {
            const int off = eoff(m, u);
            f32x4 o = *(const f32x4*)(stg + srow(u) * EP + ec * 16);
            o += __builtin_bit_cast(f32x4, sold[m][u]);                // xs += resblock(x)  (hifigan.py:133-135); zeros in mode 0
            if (wav_now) {
                const int row = erow(m, u);                            // local tile row
                if (row >= H && row < H + TT) {
                    const int t = base_t + row;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (t >= 0 && t < len) ? lrelu(o[e] / p.div, p.slope) : 0.f;
                    *(f32x4*)(otile + (size_t)(row - H) * OP + (wc * CW + ec * 4) * 4) = o;
                }
                continue;
            }
            // (an intermediate sum of a fused launch is re-read by this workgroup's next ResBlock: stored cached)
            rb_stage_row(o, rs_s, rs_a, off, mode, p.div, p.slope, p.drop_S != 0, p.Sa != nullptr, p.nrb > 1 && !last_rb);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                               // slab m + 1 reuses this wave's staging block
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        RB_T(14);                                        // (slab: rows read back, + stage sum, stored)
    }
    if constexpr (C == 32) if (wav_now) {   // (the launcher rejects p.wav for other widths)
        __syncthreads();                                               // the fp32 output tile is whole
        rb_conv_post_tanh<C, THREADS, 3>(otile, p.post_w, p.post_b, p.wav + brow, t0, TTo, len, p.bad, tid);
    }
    }   // (epilogue)
    RB_T(8);                                             // epilogue (+ the fused conv_post)
#ifdef RB_STAMP
    tq[11] += 1;
#endif
    if constexpr (GUARD) {
        if (n_ovf) atomicAdd(p.ovf, (unsigned long long)n_ovf);
    }
    if (!has_next) break;
    r = last_rb ? 0 : r + 1;
    if (wav_now) {
        // the fp32 output tile aliases the activation buffer AND its guard bands: conv_post's reads are over behind this barrier, then
        // the bands are zero again before the next tile's first convolution reads them (the barrier after its first write_act orders
        // both).  Without it a workgroup's 2nd+ tile ran its outermost halo rows on fp32 bit patterns read as 16-bit operands: the
        // results of those rows are discarded (H covers the six receptive fields), but the range guard counted their Inf / huge values.
        __syncthreads();
        zero_guard_bands(threadIdx.x);
    }
    j = jn;
    b = bn;
    len = lenn;
    t0 = t0n;
    }   // (tiles of this workgroup)
#ifdef RB_STAMP
    {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0 && (w == 0 || w == WT * WC - 1)) {
            const int slot = (C == 32 ? 0 : C == 64 ? 1 : C == 128 ? 2 : 3) * 3 + (p.K == 3 ? 0 : p.K == 7 ? 1 : 2);
            for (int k = 0; k < 16; ++k) atomicAdd(&rb_stamps[w == 0 ? 0 : 1][slot][k], tq[k]);
        }
    }
#endif
}

// dynamic LDS of an rb_launch_cfg configuration for TT valid rows per tile, WITHOUT the persistent form's tile table
template <int C, int MT, int WT>
static size_t rb_lds_bytes(int TT, bool wav) {
    constexpr int W = 32 * MT * WT, PITCH = C * 2 + 16, EP = C * 4 + 16;
    constexpr size_t ACT = (size_t)(W + 2 * RB_GUARD) * PITCH;
    if (wav)   // fused conv_post (7 taps): the fp32 output tile may be larger than the activation tile it replaces
        return std::max((size_t)TT * C * 4, ACT) + (size_t)WT * 32 * EP;
    return ACT + (size_t)WT * 32 * EP;
}

// hipErrorOutOfMemory: the configuration's LDS (with the tile table of p.B utterances) exceeds 160 KB — the caller picks another one
template <int C, int MT, int NT, int WT, int WC, int EL, int PS, bool GUARD = false>
static hipError_t rb_launch_cfg(const RBlockParams& p, hipStream_t stream) {
    typedef MfmaShape<rblock_mfma_shape(C)> SH;   // one shape per width, whatever the tile size (rblock.h)
    constexpr int W = 32 * MT * WT;
    // two k-steps per tap end on rb_contract's half group: odd kernel sizes only, and the taps the pack was padded to
    for (int j = 0; j < p.nrb; ++j)
        if (!(p.rb[j].K & 1) || p.rb[j].Kp != rblock_padded_taps(C, p.rb[j].K)) return hipErrorInvalidValue;
    const int H = rblock_halo(p), TT = W - 2 * H;
    if (TT < 32) return hipErrorInvalidValue;
    if ((long long)p.T * C * 4 >= (1LL << 31)) return hipErrorInvalidValue;   // 32-bit byte offsets inside an utterance's buffer resource
    if (p.wav && (C != 32 || (p.nrb == 1 && p.mode != 2) || !p.post_w || !p.post_b)) return hipErrorInvalidValue;
    size_t lds = rb_lds_bytes<C, MT, WT>(TT, p.wav != nullptr);
    const int TTo = p.wav ? TT - 6 : TT;
    RBlockParams q = p;
    q.pre_off = (int)lds;
    if (PS) lds += rb_table_bytes(p.B);
    if (lds > 160 * 1024) return hipErrorOutOfMemory;
    // (the 640-row C = 64 tile has no guarded form: with the census's counters it does not fit the register file on MfmaShape<16> — 6 registers
    // spilled — and rb_launch_el sends a census launch to the 512-row tile instead)
    constexpr bool HAS_GUARD = !(C == 64 && MT == 5);
    if constexpr (EL == EL_F16 && !GUARD && HAS_GUARD) {
        if (p.ovf) return rb_launch_cfg<C, MT, NT, WT, WC, EL, PS, true>(p, stream);
    }
    if (EL == EL_F16 && !HAS_GUARD && p.ovf) return hipErrorInvalidValue;
    constexpr auto kern = rblock_kernel<C, MT, NT, WT, WC, EL, PS, GUARD, SH>;
    if (const hipError_t e = rb_allow_full_lds<kern>(); e != hipSuccess) return e;
    constexpr int THREADS = 64 * WT * WC;
    if (!PS) {
        hipLaunchKernelGGL(kern, dim3((p.T + TTo - 1) / TTo, p.B), dim3(THREADS), lds, stream, q);
        return hipGetLastError();
    }
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    const int grid = rb_resident_grid(cus, lds, THREADS, THREADS <= 256 ? 2 : 1, (long long)p.B * ((p.T + TTo - 1) / TTo));
    if (grid <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(THREADS), lds, stream, q);
    return hipGetLastError();
}

// whole-ResBlock fusion pays where the halo 6 (k - 1) is small against the tile that fits: every k at C <= 64 (512-row tiles), k = 3
// at C = 128 (256 rows) and C = 256 (128 rows); the larger kernels of the wide stages run per iteration (vpair.hip)
bool rblock_supported(int C, int K) {
    if (!(K & 1) || K < 3 || K > 11) return false;
    return C == 32 || C == 64 || ((C == 128 || C == 256) && K == 3);
}

// the one-launch forms (nrb > 1) run on rb_launch_cfg<32, 4, 1, 8, 1, ., 1> (C = 32) / <64, 4, 1, 4, 2, ., 1> (C = 64): rb_launch_el
int rblock_stage_tile_rows(int C, int halo) {
    return (C == 32 ? 1024 : 512) - 2 * halo;
}

bool rblock_stage_launch_fits(int C, int halo, int B, bool wav) {
    const int TT = rblock_stage_tile_rows(C, halo);
    if (C != 32 && C != 64) return false;
    const size_t lds = (C == 32 ? rb_lds_bytes<32, 4, 8>(TT, wav) : rb_lds_bytes<64, 4, 4>(TT, wav)) + rb_table_bytes(B);
    return TT >= 32 && lds <= 160 * 1024;
}

long long rblock_private_rows(int C, int halo, int B, int T) {
    if (C != 32) return 0;
    const int TT = rblock_stage_tile_rows(C, halo), TTo = TT - 6;    // with the fused conv_post
    if (TTo < 32) return 0;
    return (long long)B * ((T + TTo - 1) / TTo) * TT;
}

// Taps of a pack (zero padded behind the real ones) such that the k-steps the kernel walks are whole groups of four.  Steps per tap: C / 16 on
// MfmaShape<32>, C / 32 on MfmaShape<16>.  Two steps per tap on MfmaShape<16> (C = 64) pad nothing: K is odd (rblock_supported), K - 1 taps
// are whole groups and rb_contract ends on a half group of two steps — one ring turn of RD = 2 — instead of multiplying a zero tap.
// (C = 32: the kernel runs the real steps, rb2_contract; the padding only keeps its prefetches inside the pack.)
int rblock_padded_taps(int C, int K) {
    const int sh = rblock_mfma_shape(C);
    const int nkg = C / (sh == 16 ? 32 : 16);
    if (sh == 16 && nkg == 2) return K;
    int kp = K;
    while ((kp * nkg) % 4) ++kp;
    return kp;
}

// Persistent workgroups everywhere but at C = 32 (same box: C = 64 -5 %, C = 128 -5 %, C = 256 -17 %; C = 32, two 4-wave workgroups
// per CU, +1 %: that one keeps one tile per workgroup).
template <int EL>
static hipError_t rb_launch_el(const RBlockParams& p, int C, hipStream_t stream) {
    // C = 32: k >= 7 on 1024-row tiles (8 waves over time, one persistent workgroup per CU: the 6 (k - 1)-row halo costs 12 % of a
    // k = 11 tile instead of 23 %; -8 % on that launch), k = 3 on 512-row tiles, two 4-wave workgroups per CU, one tile each (the
    // 1024-row form is 14 % slower there).
    // small batches (B = 1: one sentence): when the default tiles leave more than half of the CUs without one, the launch takes as long
    // as ONE tile -> half-size tiles (more halo recomputed, but twice the CUs at work)
    const int cus = rb_device_cus();
    if (cus <= 0) return hipErrorInvalidDevice;
    auto few = [&](int W) {   // tiles of W rows (valid: W - 2 rblock_halo, the fused conv_post 6 less): at most half the CUs get one
        const int tt = W - 2 * rblock_halo(p) - (p.wav ? 6 : 0);
        return tt >= 32 && 2 * (long long)p.B * ((p.T + tt - 1) / tt) <= cus;
    };
    if (p.nrb < 1 || p.nrb > 3) return hipErrorInvalidValue;
    if (p.nrb > 1) {   // every ResBlock of the stage in one launch: the persistent full-size configurations only
        if (C == 32) return rb_launch_cfg<32, 4, 1, 8, 1, EL, 1>(p, stream);
        if (C == 64) return rb_launch_cfg<64, 4, 1, 4, 2, EL, 1>(p, stream);
        return hipErrorInvalidValue;
    }
    // RB_TRY: a persistent configuration whose LDS cannot hold the tile table of this many utterances (the fused conv_post's 1024-row tile
    // above ~940 utterances, the 128-row C = 256 tile above ~1730) falls through to the next one down
    if (C == 32 && p.K >= 7 && !few(1024)) RB_TRY((rb_launch_cfg<32, 4, 1, 8, 1, EL, 1>(p, stream)));
    if (C == 64 && few(512)) return rb_launch_cfg<64, 4, 1, 2, 2, EL, 1>(p, stream);     // 256-row tile, 4 waves
    if (C == 128 && few(256)) return rb_launch_cfg<128, 4, 1, 1, 4, EL, 1>(p, stream);   // 128-row tile, 4 waves
    if (C == 256 && few(128)) return rb_launch_cfg<256, 2, 1, 1, 8, EL, 1>(p, stream);   // 64-row tile
    if (C == 32) return rb_launch_cfg<32, 4, 1, 4, 1, EL, 0>(p, stream);      // 512-row tile, 4 waves over time
    // C = 64, k >= 7: 640-row tiles (MT = 5; the halo 12 (k - 1) is 11 / 19 % of the tile instead of 14 / 23 %: -4.8 % at k = 11, nothing at k = 3
    // where 13 spilled registers cost what the halo gives); tune bit 14: 512-row tiles for every k (round 3).  The range-guard census (p.ovf, fp16
    // operands) takes the 512-row tile as well: its 640-row kernel would spill.  One MFMA shape per width, so the bits — and the count, a census
    // of output rows — do not depend on the tile size.
    if (C == 64 && p.K >= 7 && !p.small_tile && !(EL == EL_F16 && p.ovf)) RB_TRY((rb_launch_cfg<64, 5, 1, 4, 2, EL, 1>(p, stream)));
    if (C == 64) RB_TRY((rb_launch_cfg<64, 4, 1, 4, 2, EL, 1>(p, stream)));    // 512-row tile, 8 waves (4 time x 2 channel)
    if (C == 64) return rb_launch_cfg<64, 4, 1, 2, 2, EL, 1>(p, stream);       // (the tile table of a very large batch) 256-row tile
    if (C == 128) RB_TRY((rb_launch_cfg<128, 4, 1, 2, 4, EL, 1>(p, stream)));  // 256-row tile, 8 waves (2 time x 4 channel)
    if (C == 128) return rb_launch_cfg<128, 4, 1, 1, 4, EL, 1>(p, stream);     // (ditto) 128-row tile
    if (C == 256) RB_TRY((rb_launch_cfg<256, 4, 1, 1, 8, EL, 1>(p, stream)));  // 128-row tile, 8 waves over channels
    if (C == 256) return rb_launch_cfg<256, 2, 1, 1, 8, EL, 1>(p, stream);     // (ditto) 64-row tile
    return hipErrorInvalidValue;
}

hipError_t rblock_launch(const RBlockParams& p, int C, int frag, hipStream_t stream) {
    if (C != 32 && C != 64 && C != 128 && C != 256) return hipErrorInvalidValue;
    if (frag != rblock_mfma_shape(C)) return hipErrorInvalidValue;   // (every configuration of a width runs MfmaShape<rblock_mfma_shape(C)>: rb_launch_cfg)
    return p.el == EL_F16 ? rb_launch_el<EL_F16>(p, C, stream) : rb_launch_el<EL_BF16>(p, C, stream);
}

} // namespace dtts
