// Fused HifiGAN ResBlock1 kernel for the narrow stages: see rblock.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "voc_el.h"

namespace dtts {

struct RBlockParams {
    const float* x;        // stage input, fp32 [B][T][C] (the transposed conv's output)
    float* S;              // stage accumulator xs, fp32 [B][T][C]
    unsigned short* Sa;    // bf16 leaky_relu(xs / num_kernels, slope): next stage's input (mode 2 only)
    // the ResBlocks of this launch: one (rb[0]), or — nrb = 2..3, C <= 64 — ALL ResBlocks of the stage on the same tile (one launch per
    // stage: x is read from HBM once per tile, re-read from L2 / Infinity Cache by the other ResBlocks, and the stage sum is
    // read-modify-written through the cache instead of HBM: 7-8 passes over the stage's tensors become ~2)
    struct Set {
        const uint4* w1[3];   // convs1[m] / convs2[m] packed weights, Kp taps (zero padded)
        const uint4* w2[3];
        const float* b1[3];
        const float* b2[3];
        int dil[3];
        int K, Kp;
    } rb[3];
    int nrb;
    const int* lens;       // [B] valid rows
    int B, T;
    int K;                 // the LARGEST kernel size of the launch (the tile's halo: rblock_halo)
    int mode;              // what the (first) ResBlock of the launch does with the stage sum: 0: xs = r ; 1: xs += r ; 2: xs = (xs + r) / div, and emit Sa
    int last_mode;         // nrb > 1: the same for the launch's LAST ResBlock (2 when it is the stage's last, else 1); those in between accumulate (1)
    int drop_S;            // mode 2 with Sa: do not write the fp32 xs (nothing reads it after the stage)
    float div, slope;
    // fused conv_post + tanh (last stage, mode 2, C = 32): the stage output never reaches HBM, the waveform is written instead
    float* wav;            // [B][T] or null
    const float* post_w;   // conv_post weight as [7 taps][C] fp32
    const float* post_b;   // [1]
    int el;                // 16-bit operand type: EL_BF16 (rb_common.h) or EL_F16; the packed weights are in that type
    unsigned* tile_ctr;    // persistent configurations: device counter (zero at launch) for dynamic tile claiming, or null = static w, w + G, ...
    int pre_off;           // (set by the launcher) byte offset of the tile-count table in dynamic LDS
    unsigned* bad;         // always-on detector of the fused conv_post: device counter of NON-FINITE pre-tanh values (an fp16 operand overflowed upstream), or null
    unsigned long long* ovf;   // fp16 range guard: device counter of unrepresentable activations (launches the GUARD instantiation), or null
    int small_tile;        // tune bit 14: C = 64 keeps 512-row tiles at k >= 7 (A/B against the default 640)
    int : 32;              // (an unused word: with s_private moved up into it hipcc merges the kernels' scalar argument loads differently)
    int s_private;         // 0, or the byte capacity of S when it holds one private TT-row strip per TILE (fused launch + fused conv_post)
};

// rows of halo per side of a tile for one ResBlock of kernel size K: the sum of its six convolutions' receptive half-widths,
// (K - 1) / 2 * (d0 + d1 + d2 + 3), and never less than 6 (K - 1) — exactly that for dilations (1, 3, 5)
__host__ __device__ inline int rblock_halo_of(int K, const int* dil) {
    const int need = (K - 1) / 2 * (dil[0] + dil[1] + dil[2] + 3);
    return need > 6 * (K - 1) ? need : 6 * (K - 1);
}
// the halo of a launch: the largest of its ResBlocks' (and at least 6 (p.K - 1))
__host__ __device__ inline int rblock_halo(const RBlockParams& p) {
    int h = 6 * (p.K - 1);
    for (int j = 0; j < p.nrb && j < 3; ++j) {
        const int need = rblock_halo_of(p.rb[j].K, p.rb[j].dil);
        h = need > h ? need : h;
    }
    return h;
}

// MFMA shape of rblock's contractions at width C (rb_common.h: MfmaShape): 16 = v_mfma_f32_16x16x32, 32 = v_mfma_f32_32x32x16.  ONE shape per
// width, whatever the tile size and whether one ResBlock or the whole stage runs in a launch: every launch configuration of a layer sums it in
// the same order (an utterance alone is bit-identical to the same utterance inside a batch).  The packs are in this fragment order.
// C = 64 runs the 16x16x32 form: the same MFMA cycles, operands and bits as 32x32x16, fewer joules in kernels that sit at the board's power limit
// (LABNOTES "rblock on the MFMA shape trait").  C = 128 / 256 (the k = 3 launches) are one line here, packs included: built, bit-identical and
// faster on the vocoder benchmark, but not yet kept — their own launches' trace was not collected (same LABNOTES section).  C = 32 is not a
// choice: its contraction (rb2_contract) is written for 32x32x16, and it is LDS-bound.
constexpr int rblock_mfma_shape(int C) { return C == 64 ? 16 : 32; }

bool rblock_supported(int C, int K);
int rblock_padded_taps(int C, int K);
// frag: the fragment order EVERY pack of the launch is in (pack.hip: pack_conv; 0 = mixed).  hipErrorInvalidValue, and nothing runs, unless it is
// rblock_mfma_shape(C): a kernel walks a pack in its own order or not at all.
hipError_t rblock_launch(const RBlockParams& p, int C, int frag, hipStream_t stream);
// the launches with ALL ResBlocks of a stage (nrb > 1; tune bits 9 / 12), for a launch halo of `halo` rows (rblock_halo):
// rows a fused launch with the fused conv_post needs in S (one private strip per tile), or 0 when the configuration does not fuse
long long rblock_private_rows(int C, int halo, int B, int T);
// valid rows per tile of that launch (conv_post not counted), and whether its LDS — incl. the tile table of B utterances — fits
int rblock_stage_tile_rows(int C, int halo);
bool rblock_stage_launch_fits(int C, int halo, int B, bool wav);

} // namespace dtts
