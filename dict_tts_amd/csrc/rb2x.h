// Fused HifiGAN ResBlock2 (two dilated convolutions, a residual add after each): see rb2x.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "voc_el.h"

namespace dtts {

struct RB2xParams {
    const float* x;        // stage input, fp32 [B][T][C] (the transposed conv's output)
    float* S;              // stage accumulator xs, fp32 [B][T][C]
    unsigned short* Sa;    // bf16 leaky_relu(xs / num_kernels, slope): next stage's input (mode 2 only), or null
    const uint4* w[2];     // convs[0] / convs[1] packed 16-bit weights, Kp taps (zero padded: rblock_padded_taps) + slack
    const float* b[2];
    int dil[2];
    int K, Kp;
    const int* lens;       // [B] valid rows, or null (every row of T)
    int B, T;
    int mode;              // what the launch does with the stage sum: 0: xs = r ; 1: xs += r ; 2: xs = (xs + r) / div, and emit Sa
    int drop_S;            // mode 2 with Sa: do not write the fp32 xs (nothing reads it after the stage)
    float div, slope;
    // fused conv_post + tanh (last stage, mode 2, C = 32): the stage output never reaches HBM, the waveform is written instead
    float* wav;            // [B][T] or null
    const float* post_w;   // conv_post weight as [7 taps][C] fp32
    const float* post_b;   // [1]
    int el;                // 16-bit operand type: EL_BF16 or EL_F16; the packed weights are in that type
    unsigned* tile_ctr;    // device counter (zero at launch) for dynamic tile claiming, or null = static w, w + G, ...
    unsigned* bad;         // always-on detector of the fused conv_post: device counter of NON-FINITE pre-tanh values, or null
    unsigned long long* ovf;   // fp16 range guard: device counter of unrepresentable activations (launches the GUARD instantiation), or null
    int pre_off;           // (set by the launcher) byte offset of the tile table in dynamic LDS
    int halo, guard;       // (set by the launcher) rb2x_halo / rb2x_guard of this ResBlock
};

// ---- the tile rule (restated by tests/rb2x_shapes.py) -------------------------------------------------------------------------------
// rows of halo per side of a tile: the sum of the two convolutions' receptive half-widths.  Row r of the tile is exact after the first
// convolution when r is at least (K - 1) / 2 * d0 rows from either edge, and after the second when it is (K - 1) / 2 * (d0 + d1) away.
__host__ __device__ inline int rb2x_halo(int K, int d0, int d1) { return (K - 1) / 2 * (d0 + d1); }
// zero rows on both sides of the LDS tile.  A contraction reads row + (tap - (K - 1) / 2) * d for tap 0 .. K: tap K is the activation
// fragment prefetched one k-step behind the last real one (its product is never taken), so the reach is (K - 1) / 2 * d below the tile
// and (K + 1) / 2 * d above it; the bands are the larger dilation's upper reach on both sides.
__host__ __device__ inline int rb2x_guard(int K, int d0, int d1) { return (K + 1) / 2 * (d0 > d1 ? d0 : d1); }
// LDS rows W of a width's tiles: the configuration every batch size can launch (`base`) and the larger one tried first where the halo
// is worth it (`wide`: K >= 7 at C = 32, halo >= 16 at C = 128 / 256; it falls back to `base` when its LDS, with the tile table of the
// batch, exceeds 160 KB).  A tile of W rows outputs TT = W - 2 halo rows; with the fused conv_post (7 taps) TT - 6 samples.
__host__ __device__ inline int rb2x_base_rows(int C) { return C <= 64 ? 512 : (C == 128 ? 256 : 128); }
__host__ __device__ inline int rb2x_wide_rows(int C) { return C == 32 ? 1024 : (C == 64 ? 512 : (C == 128 ? 384 : 192)); }
__host__ __device__ inline bool rb2x_wide_wanted(int C, int K, int halo) { return C == 32 ? K >= 7 : (C >= 128 && halo >= 16); }
// dynamic LDS of a tile of W rows, without the tile table: the 16-bit activation tile with its guard bands (row pitch 2 C + 16 bytes);
// the epilogue's fp32 transposition rows (32 per time-wave, pitch 4 C + 16) lie inside the tile rows.  With the fused conv_post the fp32
// output tile (TT rows of 4 C bytes) takes the activation tile's place and the transposition rows follow whichever is larger.
__host__ __device__ inline size_t rb2x_lds_bytes(int C, int W, int time_waves, int halo, int guard, bool wav) {
    const size_t act = (size_t)(W + 2 * guard) * (C * 2 + 16);
    if (!wav) return act;
    const size_t ot = (size_t)(W - 2 * halo) * C * 4;
    return (ot > act ? ot : act) + (size_t)time_waves * 32 * (C * 4 + 16);
}

// (C, K, d0, d1) the fused kernel runs for EVERY batch size up to DTTS_MAX_VOCODER_BATCH: widths 32 / 64 / 128 / 256, odd K 3 .. 11,
// dilations >= 1, and the `base` tile keeps at least 32 output rows (38 at C = 32, where the fused conv_post takes 6) with its LDS and
// the largest tile table inside 160 KB.  build_vocoder and rb2x_launch both call this.
bool rb2x_supported(int C, int K, int d0, int d1);
hipError_t rb2x_launch(const RB2xParams& p, int C, hipStream_t stream);

} // namespace dtts
