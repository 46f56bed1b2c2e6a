// The acoustic model's validation losses (losses.hip): the sums behind the masked mel losses l1 / mse / ssim of the reference's add_mel_loss
// (tasks/tts/tts_base.py:182-222, modules/commons/ssim.py) and behind the word-duration losses of add_dur_loss in eval mode
// (tasks/tts/ps_flow.py:99-139).  Two launches for the mel half (tiles, then an utterance's tiles added in index order), one for the
// durations.  An utterance's mel sums depend on T and on its own rows only (the image is zero outside [0, T) x [0, n_mel), pad rows inside
// are read as they are): bit-identical in any batch at the same T, and NOT the sums of the utterance alone at a shorter T.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int LOSS_TILE_ROWS = DTTS_LOSS_TILE_ROWS;   // FIXED: the tile sums of an utterance are joined in tile order (batch invariance)
constexpr int LOSS_WIN = 11, LOSS_HALO = LOSS_WIN / 2;
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_MAX_MEL = 128;
constexpr int LOSS_LDS_BYTES = 160 * 1024;

// create_window(11, 1) of modules/commons/ssim.py: the float32 Gaussian of sigma 1.5, divided by its float32 sum (the sum correctly
// rounded, as torch's reduction gives it for these eleven values), then the float32 outer product; widened to fp64 for the kernel
inline void loss_window(double w[LOSS_WIN * LOSS_WIN]) {
    float g[LOSS_WIN];
    double s = 0;
    for (int x = 0; x < LOSS_WIN; ++x) {
        g[x] = (float)std::exp(-(double)((x - LOSS_HALO) * (x - LOSS_HALO)) / (2.0 * 1.5 * 1.5));
        s += (double)g[x];
    }
    const float sf = (float)s;
    for (int x = 0; x < LOSS_WIN; ++x) g[x] = g[x] / sf;
    for (int i = 0; i < LOSS_WIN; ++i)
        for (int j = 0; j < LOSS_WIN; ++j) w[i * LOSS_WIN + j] = (double)(g[i] * g[j]);
}

struct LossMelParams {
    const float* pred;       // [B][pred_ld][n_mel]
    const float* tgt;        // [B][tgt_ld][n_mel]
    const double* win;       // [121], loss_window
    double* part;            // [B][ntile][3]: sum w |d|, sum w d^2, sum w (1 - ssim) of one tile
    long long* pcount;       // [B][ntile]: weighted elements of one tile
    float* map;              // [B][T][n_mel] out, or null
    int B, T, n_mel, pred_ld, tgt_ld, ntile;
    float bias;
};

struct LossMelReduceParams {
    const double* part;
    const long long* pcount;
    double* sums;            // [B][3]
    long long* count;        // [B]
    int B, ntile;
};

struct LossDurParams {
    const float* dur_pred;   // [B][T_w]
    const long long* m2w;    // [B][m2w_ld]
    const int* word_len;     // [B]
    double* sums;            // [B][5]
    int* dur_gt;             // [B][T_w] out, or null
    int B, T_w, T_mel, m2w_ld, log_scale;
};

// LDS of one tile: both biased images with their halo in fp64, one fp64 triple per thread for the tree, one weight per row
inline size_t loss_mel_lds_bytes(int n_mel) {
    const size_t img = (size_t)(LOSS_TILE_ROWS + 2 * LOSS_HALO) * (n_mel + 2 * LOSS_HALO);
    return (2 * img + 3 * LOSS_THREADS) * sizeof(double) + LOSS_TILE_ROWS * sizeof(int);
}
inline size_t loss_dur_lds_bytes(int T_w) { return (size_t)5 * LOSS_THREADS * sizeof(double) + ((size_t)T_w + 1) * sizeof(int); }

hipError_t loss_mel_launch(const LossMelParams& p, hipStream_t stream);
hipError_t loss_mel_reduce_launch(const LossMelReduceParams& p, hipStream_t stream);
hipError_t loss_dur_launch(const LossDurParams& p, hipStream_t stream);

} // namespace dtts
