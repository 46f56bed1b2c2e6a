// Fused HifiGAN ResBlock1 kernel for the NARROW stages (C = 16 / 8: the last two stages of the V2 generators): see rbn.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "voc_el.h"
#include "rblock.h"

namespace dtts {

// the contract of RBlockParams (rblock.h) for one ResBlock per launch
struct RBnParams {
    const float* x;        // stage input, fp32 [B][T][C] (the transposed conv's output)
    float* S;              // stage accumulator xs, fp32 [B][T][C]
    unsigned short* Sa;    // bf16 leaky_relu(xs / num_kernels, slope): next stage's input (mode 2 only), or null
    const uint4* w1[3];    // convs1[m] / convs2[m] packed 16-bit weights in the tap-folded fragment order (RBN_FRAG), Kp taps
    const uint4* w2[3];
    const float* b1[3];    // (zero padded to 16 channels and beyond: pack_conv)
    const float* b2[3];
    int dil[3];
    int K, Kp;
    const int* lens;       // [B] valid rows, or null (every row of T)
    int B, T;
    int mode;              // what the launch does with the stage sum: 0: xs = r ; 1: xs += r ; 2: xs = (xs + r) / div, and emit Sa
    int drop_S;            // mode 2 with Sa: do not write the fp32 xs (nothing reads it after the stage)
    float div, slope;
    // fused conv_post + tanh (last stage, mode 2): the stage output never reaches HBM, the waveform is written instead
    float* wav;            // [B][T] or null
    const float* post_w;   // conv_post weight as [7 taps][C] fp32
    const float* post_b;   // [1]
    int el;                // 16-bit operand type: EL_BF16 or EL_F16; the packed weights are in that type
    unsigned* tile_ctr;    // device counter (zero at launch) for dynamic tile claiming, or null = static w, w + G, ...
    unsigned* bad;         // always-on detector of the fused conv_post: device counter of NON-FINITE pre-tanh values, or null
    unsigned long long* ovf;   // fp16 range guard: device counter of unrepresentable activations (launches the GUARD instantiation), or null
    int pre_off;           // (set by the launcher) byte offset of the tile table in dynamic LDS
    int halo, guard;       // (set by the launcher) rblock_halo_of / rbn_guard of this ResBlock
};

// Fragment order of the packs (pack.hip: pack_conv `frag`): the A operand of v_mfma_f32_16x16x32 with the TAPS folded into the contraction
// index, k = (tap within the step) * C + ci.  Per k-step (32 / C taps) 64 lanes x 8 elements: lane = 16 * kq + co, element e <-> k = 8 kq + e;
// output channels >= C are zero rows.
constexpr int RBN_FRAG = 2;

// ---- the tile rule (restated by tests/rbn_shapes.py) ----------------------------------------------------------------------------------
__host__ __device__ inline int rbn_taps_per_step(int C) { return 32 / C; }
// taps of a pack: zero padded behind the real ones to whole k-steps (k = 3 / 7 / 11 -> 4 / 8 / 12 at both widths)
__host__ __device__ inline int rbn_padded_taps(int C, int K) {
    const int tps = rbn_taps_per_step(C);
    return (K + tps - 1) / tps * tps;
}
// zero rows on both sides of the LDS tile: a contraction reads row + (tap - (K - 1) / 2) * d for tap 0 .. Kp - 1 (the padded taps multiply
// zero weights, but what they read must be finite), so the reach is (K - 1) / 2 * d below the tile and (Kp - 1 - (K - 1) / 2) * d above it
__host__ __device__ inline int rbn_guard(int C, int K, const int* dil) {
    int d = dil[0] > dil[1] ? dil[0] : dil[1];
    d = d > dil[2] ? d : dil[2];
    d = d > 1 ? d : 1;
    return (rbn_padded_taps(C, K) - 1 - (K - 1) / 2) * d;
}
// LDS rows of the three tile sizes, largest first.  A tile of W rows outputs TT = W - 2 halo rows; with the fused conv_post (7 taps) TT - 6 samples.
constexpr int RBN_ROWS[3] = {1024, 512, 256};
// dynamic LDS of a tile of W rows without the tile table: the six packs, the 16-bit activation tile with its guard bands (row pitch 2 C bytes) and,
// with the fused conv_post, the fp32 output tile (TT rows of 4 C bytes)
__host__ __device__ inline size_t rbn_lds_bytes(int C, int W, int Kp, int halo, int guard, bool wav) {
    return (size_t)6 * (Kp / rbn_taps_per_step(C)) * 1024 + (size_t)(W + 2 * guard) * (C * 2) + (wav ? (size_t)(W - 2 * halo) * C * 4 : 0);
}

// (C, K, dilations) the kernel runs for EVERY batch size up to DTTS_MAX_VOCODER_BATCH: widths 16 / 8, odd K 3 .. 11, dilations >= 1, and the smallest
// tile keeps at least 32 output rows (with the fused conv_post's 6 taken off) with its LDS and the largest tile table inside 160 KB.
// build_vocoder and rbn_launch both call this.
bool rbn_supported(int C, int K, int d0, int d1, int d2);
// frag: the fragment order every pack of the launch is in (0 = mixed); hipErrorInvalidValue, and nothing runs, unless it is RBN_FRAG
hipError_t rbn_launch(const RBnParams& p, int C, int frag, hipStream_t stream);

} // namespace dtts
