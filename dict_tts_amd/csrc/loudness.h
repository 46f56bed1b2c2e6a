// ITU-R BS.1770 integrated loudness of a batch of mono waveforms and their normalisation to a target (loudness.hip;
// dtts_text2mel_fetch(DTTS_OUT_LOUDNESS)): pyloudnorm 0.1.1's Meter.integrated_loudness / normalize.loudness and the reference's peak rule,
// as data_gen_utils.py::process_utterance(loud_norm=True) runs them.  The specification is in include/dicttts_hip.h; tests/wavprep_ref.py
// restates it in float64.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int LOUD_SEG = DTTS_LOUD_SEGMENT;   // samples of one segment of the recurrence.  FIXED: the cut of an utterance, hence its rounding
constexpr int LOUD_SLOTS = 6;                 // blocks one segment can meet: at most 5 (see loud_first_block), one to spare
constexpr int LOUD_MAX_WAV = 1 << 26;

// the two biquads, normalised by their a0: y = z1 + b0 x; z1 = (z2 + b1 x) - a1 y; z2 = b2 x - a2 y
struct LoudCoef {
    double b0a, b1a, b2a, a1a, a2a;   // the high shelf
    double b0b, b1b, b2b, a1b, a2b;   // the high pass
};

// one sample through the cascade; s = (z1, z2 of the shelf, z1, z2 of the high pass).  Written once for the host (M and its power) and the
// device, and never contracted
__host__ __device__ inline double loud_step(const LoudCoef& c, double s[4], double x) {
#pragma clang fp contract(off)
    const double ya = s[0] + c.b0a * x;
    s[0] = (s[1] + c.b1a * x) - c.a1a * ya;
    s[1] = c.b2a * x - c.a2a * ya;
    const double yb = s[2] + c.b0b * ya;
    s[2] = (s[3] + c.b1b * ya) - c.a1b * yb;
    s[3] = c.b2b * ya - c.a2b * yb;
    return yb;
}

// pyloudnorm's block count of an L-sample utterance: 0 below one block, else (int)(rint((L / rate - 0.4) / (0.4 * 0.25)) + 1)
__host__ __device__ inline int loud_n_blocks(int L, double rate) {
#pragma clang fp contract(off)
    if (L < 0 || (double)L < 0.4 * rate) return 0;
    const double T = (double)L / rate;
    return (int)(rint((T - 0.4) / (0.4 * 0.25)) + 1.0);
}

struct LoudParams {
    const float* wav;        // [B][wav_ld]
    const int* lens;         // [B] or null
    const int2* bounds;      // [>= the blocks of wav_ld samples]: (lo_j, hi_j), host-made
    double* seg_end;         // workspace [B][nseg_ld][4]: the end state of a segment run from zero
    double* seg_start;       // workspace [B][nseg_ld][4]: its true start state
    float* seg_max;          // workspace [B][nseg_ld]: max |x| of the segment
    float* utt_max;          // workspace [B]
    double* part;            // workspace [B][nseg_ld][LOUD_SLOTS]: the segment's share of the blocks it meets
    double* z;               // [B][blocks_ld] (the caller's, or workspace)
    int* n_blocks;           // [B] (the same)
    double* lufs;            // [B]
    double* gain;            // [B]
    int* status;             // [B]
    float* out;              // [B][wav_ld] or null (mode 0)
    LoudCoef c;
    double ms[4][4];         // M^S: the free response of the cascade over one segment
    double rate, target;
    int B, wav_ld, blocks_ld, nseg_ld, mode;
};

LoudCoef loud_coefficients(double rate);
void loud_segment_matrix(const LoudCoef& c, double ms[4][4]);
hipError_t loud_launch(const LoudParams& p, hipStream_t stream);

} // namespace dtts
