// HifiGAN's discriminators as a measurement (disc.hip, gconv.hip; dtts_text2mel_fetch(DTTS_OUT_DISC)): MultiPeriodDiscriminator and
// MultiScaleDiscriminator of modules/hifigan/hifigan.py run on B waveform pairs, and the fp64 sums behind generator_loss, discriminator_loss
// and feature_loss per utterance.  Activations are channels-last fp32 and hold the PRE-activation outputs: leaky_relu(0.1) is applied by
// whoever reads them (conv1d's staging, the grouped kernel's staging, conv_post, the feature sums).  y and y_hat run as one batch of 2B
// signals: sequence s < B is a recording, s >= B the generated waveform of pair s - B; a period discriminator's column j of signal s is
// sequence s * p + j.  Every launch addresses a sequence by its own lengths only, so an utterance's bits do not depend on the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/dicttts_hip.h"
#include "conv1d.h"

namespace dtts {

constexpr int DISC_PERIODS[5] = {2, 3, 5, 7, 11};
constexpr int DISC_MAX_P = 11;
constexpr float DISC_SLOPE = 0.1f;        // LRELU_SLOPE
constexpr int DISC_MPD_LAYERS = 6;        // 5 convolutions + conv_post
constexpr int DISC_MSD_LAYERS = 8;        // 7 convolutions + conv_post
constexpr int DISC_FM_TILE = 8192;        // FIXED: floats of one partial feature sum; an utterance's partial sums are joined in tile order
constexpr int DISC_THREADS = 256;
constexpr int GCONV_K = 41, GCONV_PAD = 20;

// one grouped convolution (k = 41, pad 20) packed for gconv_kernel: per (group, co-tile of 32, k-step of 8, lane) four floats, the B operand of
// four successive v_mfma_f32_32x32x2_f32: lane l, element e holds W[g * cog + 32 n + (l & 31)][ci][tap] with tap * cig + ci = 8 Q + 4 (l >> 5) + e
struct GroupedConv {
    float* w = nullptr;
    float* bias = nullptr;
    int C_in = 0, C_out = 0, groups = 1, stride = 1;
    int cig = 0, cog = 0, ntg = 1, nq = 0;   // channels per group in / out, co-tiles per group, k-steps (41 * cig / 8)
    std::vector<float> hw, hb;               // host copy [C_out][cig][41] / [C_out]: the block-diagonal dense form is packed from it on demand
};

struct GConvParams {
    const float* x;        // [nseq][T_in][C_in], pre-activation
    float* y;              // [nseq][T_out][C_out], pre-activation
    const float* w;
    const float* bias;
    const int* in_lens;    // [nseq]
    const int* out_lens;   // [nseq]
    int nseq, T_in, T_out, C_in, C_out, cig, cig_shift, cog, ntg, nq, stride;
    float slope;           // leaky_relu applied to x while staging
};

inline bool gconv_wide(int cog) { return cog > 32; }   // two co-tiles per group: 2 x 2 waves over 64 rows; else 4 waves over 128 rows
inline int gconv_tile_rows(int cog) { return gconv_wide(cog) ? DTTS_DISC_GROUP_TILE_WIDE : DTTS_DISC_GROUP_TILE; }
inline size_t gconv_lds_bytes(int cig, int cog, int stride) {
    return (size_t)((gconv_tile_rows(cog) - 1) * stride + GCONV_K) * (cig + 4) * sizeof(float);
}
hipError_t gconv_launch(const GConvParams& p, hipStream_t stream);   // gconv.hip

struct DiscMpd {
    float *w0 = nullptr, *b0 = nullptr;   // convs.0: [32][5], [32]
    PackedConv conv[4];                   // convs.1 .. 4 (ENG_F32)
    float* wpost = nullptr;               // conv_post as [3][1024]
    float bpost = 0.f;
};
struct DiscMsd {
    float *w0 = nullptr, *b0 = nullptr;   // convs.0 transposed: [15][128], [128]
    GroupedConv g[5];                     // convs.1 .. 5
    PackedConv c6;                        // convs.6 (ENG_F32)
    PackedConv gd[5];                     // DTTS_DISC_DENSE_GROUPED: convs.1 .. 5 as block-diagonal dense layers (packed by the first call that asks)
    bool gd_ready = false;
    float* wpost = nullptr;
    float bpost = 0.f;
};

// rows after a convolution of kernel k, stride s, padding pad (0 rows stay 0)
inline int disc_conv_rows(int r, int k, int s, int pad) { return r > 0 ? (r + 2 * pad - k) / s + 1 : 0; }

} // namespace dtts
