// The acoustic checkpoint's multi-window mel discriminator as a measurement (meldisc.hip; dtts_text2mel_fetch(DTTS_OUT_MELDISC)):
// modules/fastspeech/multi_window_disc.py::Discriminator in eval mode on clips of n_sig mels, and the fp64 sums behind the a / r / f terms of
// tasks/tts/dict_tts.py::_training_step per (signal, window).  A clip is (signal, start): `win` frames of that signal's mel from `start`, frames
// at or behind the signal's own length entering as zeros.  Activations are channels-last fp32 [clip][t][f][H] and hold the POST-LeakyReLU
// values; the norm that follows a block (blocks 2 and 3) is applied by whoever reads the map: the next convolution's staging or the head, to
// in-range elements only, so that the zero padding is padding of the normalised map.  Every launch addresses a clip by its own signal's length
// and start only: a clip's bits do not depend on the batch, the padding behind it or the workspace's history.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int MELDISC_WINS[DTTS_MELDISC_MAX_WIN] = {32, 64, 128};
constexpr int MELDISC_F = DTTS_MELDISC_MELS;   // freq_length
constexpr float MELDISC_SLOPE = 0.2f;          // LeakyReLU(0.2)
constexpr double MELDISC_IN_EPS = 1e-5;        // InstanceNorm2d's eps
constexpr int MELDISC_KC = 32;                 // input channels of one staged chunk of the implicit GEMM
constexpr int MELDISC_PITCH = MELDISC_KC + 4;  // floats per staged cell: 16 B aligned, neighbouring cells off a common bank
constexpr int MELDISC_TILE = 32;               // output positions of a workgroup: TR rows x FC columns of the map (one MFMA m-tile)
constexpr int MELDISC_THREADS = 256;

enum { MELDISC_NORM_NONE = 0, MELDISC_NORM_INSTANCE = 1, MELDISC_NORM_AFFINE = 2 };

// one window's Discriminator2DFactory, packed by dtts_finalize_weights(DTTS_PART_MELDISC)
struct MelDiscWin {
    float *w0 = nullptr, *b0 = nullptr;             // block 1 (c_in = 1): [9][H] (tap-major), [H]
    // blocks 2 and 3 for meldisc_conv_kernel: per (co-tile of 32, ci-chunk of 32, tap, q < 4, lane) four floats, the B operand of four
    // successive v_mfma_f32_32x32x2_f32: lane l, element e holds W[32 n + (l & 31)][32 ch + 8 q + 4 (l >> 5) + e][tap] (GroupedConv's permutation)
    float *wp[2] = {nullptr, nullptr}, *bp[2] = {nullptr, nullptr};
    int norm[2] = {0, 0};                           // MELDISC_NORM_* of the map blocks 2 / 3 leave
    float* gamma[2] = {nullptr, nullptr};           // instance norm: weight [H]
    float2* fixed[2] = {nullptr, nullptr};          // no norm / folded BatchNorm: (0, scale) [H], the same for every clip
    float* shift[2] = {nullptr, nullptr};           // bias of the norm / shift of the folded BatchNorm / 0 [H]
    float* wh = nullptr;                            // adv_layer channels-last: [t][f][H] (stack, sum) or [f][H] (none)
    float bh = 0.f;
};

struct MelConvParams {
    const float* x;      // [nclip][Tin][Fin][H] post-activation, norm pending
    float* y;            // [nclip][Tout][Fout][H] post-activation
    const float* w;      // MelDiscWin::wp
    const float* bias;
    const float2* nrm;   // (mean, scale) of x per (clip, channel); clip stride nrm_ld (0: one row for every clip)
    const float* shift;  // [H]
    const int* cst;      // [nclip] the clip's start frame, or -1: no such clip
    int nrm_ld, H, Tin, Fin, Tout, Fout, TR, FC, fc_shift, ntf, nch;
};

inline size_t meldisc_conv_lds(int TR, int FC) { return (size_t)(2 * TR + 1) * (2 * FC + 1) * MELDISC_PITCH * sizeof(float); }
// the tile shape with the fewest tiles over a Tout x Fout map (the first of equals)
inline void meldisc_tile_shape(int Tout, int Fout, int* TR, int* FC) {
    const int cand[4][2] = {{8, 4}, {4, 8}, {16, 2}, {2, 16}};
    long best = -1;
    for (const auto& c : cand) {
        const long n = (long)((Tout + c[0] - 1) / c[0]) * ((Fout + c[1] - 1) / c[1]);
        if (best < 0 || n < best) {
            best = n;
            *TR = c[0];
            *FC = c[1];
        }
    }
}

} // namespace dtts
