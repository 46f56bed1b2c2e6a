// Band-limited resampling of a batch of waveforms (resample.hip; dtts_text2mel_fetch(DTTS_OUT_RESAMPLE)): resampy 0.4.2's resample_f with
// the windowed-sinc table of dtts_finalize_weights(DTTS_PART_RESAMPLE), which is what librosa 0.9.2's load / resample run for
// res_type = 'kaiser_best'.  The specification is in include/dicttts_hip.h; tests/wavprep_ref.py restates it in float64.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int RESAMPLE_TILE = DTTS_RESAMPLE_TILE;   // consecutive outputs of one workgroup, one per lane
constexpr int RESAMPLE_MAX_WAV = 1 << 26;
constexpr int RESAMPLE_MAX_WIN = 1 << 17;
constexpr int RESAMPLE_MAX_TABLE = 1024;
constexpr int RESAMPLE_MAX_WING = 2048;             // taps of one wing: (n_win - 1) / index_step

struct ResampleParams {
    const float* wav;        // [B][wav_ld]
    const int* lens;         // [B] or null
    const double2* tab;      // [n_win]: (win[i], interp_delta[i])
    float* out;              // [B][out_ld]
    int* out_lens;           // [B]
    double* out64;           // [B][out_ld] or null
    double ratio, inc, scale, tscale, num_table;   // tscale: what every table entry is multiplied by (ratio below 1, else 1: exact)
    int B, wav_ld, out_ld, n_win, index_step, wing, lds_n;   // wing = n_win / index_step >= the taps of a wing; lds_n: doubles of the staged span
};

// the doubles of LDS a tile's input span needs: its outputs' own samples, both wings and the truncations' slack
inline int resample_lds(double inc, int wing) { return (int)((double)RESAMPLE_TILE * inc) + 2 * wing + 6; }

hipError_t resample_launch(const ResampleParams& p, hipStream_t stream);

} // namespace dtts
