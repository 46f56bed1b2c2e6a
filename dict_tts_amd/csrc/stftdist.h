// Multi-resolution STFT distance between two batches of waveforms (stftdist.hip): the figures `sc` / `mag` of the reference's vocoder
// validation (tasks/vocoder/hifigan.py:62-76 -> modules/hifigan/stft_loss.py), one launch per resolution plus one reduction launch.
#pragma once
#include <hip/hip_runtime.h>

#include "stft_core.h"

namespace dtts {

constexpr int STFT_MAX_RES = 4;
constexpr int STFT_WAVES = 4;             // waves of a tile, 16 frame pairs each.  FIXED: the tile sums of an utterance are joined in tile order,
                                          // so the tile size must not depend on the batch (an utterance alone = the same utterance in any batch)
constexpr int STFT_RED_DWORDS = 2 * 3 * STFT_WAVES;   // LDS behind the slabs: one fp64 triple per wave
constexpr float STFT_CLAMP = 1e-7f;       // stft_loss.py: torch.clamp(real ** 2 + imag ** 2, min=1e-7)

struct StftParams {
    const float* x;          // [B][wav_ld]
    const float* y;          // [B][wav_ld]
    const int* lens;         // [B] samples, or null = wav_ld
    double* part;            // [B][ntile][3]: sum d^2, sum p_y, sum |log m_y - log m_x| of one tile
    float* mag;              // [2][B][mag_cap][n_fft / 2 + 1] out, or null: the clamped magnitudes of x (0) and y (1)
    StftGeom g;              // the basis of the window, zero padded and centred to n_fft; tt = frame PAIRS per tile (<= 16 * STFT_WAVES)
    int B, wav_ld, mag_cap;
    int ybase;               // LDS dword at which the slab of y starts
    int red;                 // LDS dword (even) of the waves' fp64 triples, behind slab y: set by stft_launch
};

// the tiles of every resolution summed per utterance, in tile order
struct StftReduceParams {
    const double* part[STFT_MAX_RES];
    const int* lens;
    double* sums;            // [n_res][B][3]
    long long* count;        // [n_res][B] = T_b (n_fft / 2 + 1), 0 where len_b <= n_fft / 2
    int n_res, B, wav_ld;
    int hop[STFT_MAX_RES], n_fft[STFT_MAX_RES], tt[STFT_MAX_RES], ntile[STFT_MAX_RES];
};

// worst conflict degree of the kernel's slab read (ds_read_b32: 32 banks, the two 32-lane halves are separate groups): lanes 0 - 15 of a
// half read 16 rows of slab x, lanes 16 - 31 the same 16 rows of slab y, which starts at dword ybase; over every wave and phase
int stft_conflict_degree(int hop, int ps, int ybase);
// the layout the launcher takes: the skew and the start of slab y (the first dword >= one slab, + 0 .. 31) of the smallest degree
struct StftLayout { int ps, tt, ybase, degree; size_t lds_bytes; };
StftLayout stft_layout(int hop, int n_fft);

hipError_t stft_launch(StftParams p, hipStream_t stream);
hipError_t stft_reduce_launch(const StftReduceParams& p, hipStream_t stream);

} // namespace dtts
