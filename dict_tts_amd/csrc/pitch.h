// F0 tracks of a batch of waveforms by Boersma's autocorrelation method (pitch.hip; dtts_text2mel_fetch(DTTS_OUT_PITCH)): Praat's
// "Sound: To Pitch (ac)" with the Hanning window, as the reference's data_gen_utils.py::get_pitch asks parselmouth for.  The
// specification is in include/dicttts_hip.h; tests/pitch_ref.py restates it in float64.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/dicttts_hip.h"

namespace dtts {

constexpr int PITCH_CAND = DTTS_PITCH_CANDIDATES;
constexpr int PITCH_MAX_NSW = DTTS_PITCH_MAX_WINDOW;
constexpr int PITCH_MAX_FRAMES = DTTS_PITCH_MAX_FRAMES;
constexpr int PITCH_MAX_WAV = 1 << 26;
constexpr int PITCH_LAGS = 7;      // consecutive lags a lane of pitch_acf owns.  ODD: the lanes' 8-byte LDS reads, 7 doubles apart, fall on 32 distinct bank pairs
constexpr int PITCH_JBLOCK = 8;    // products per lag between two refills of the lane's register window
constexpr int PITCH_PSI = 16;      // backpointer bytes per frame (15 slots, padded to a 16-byte row)

// what the sample rate and the pitch floor fix (the host's view; dict_tts_amd/pitch.py::geometry and tests/pitch_ref.py restate it)
struct PitchGeometry {
    int nsw, half, nper, halfper, maxlag, brent, n_lag, first;   // first = ceil(q): the shortest utterance with a frame
};

inline PitchGeometry pitch_geometry(int sample_rate, double floor_hz) {
    PitchGeometry g;
    const double q = (3.0 * (double)sample_rate) / floor_hz;     // the one real quotient
    const int nsw0 = (int)std::floor(q);
    g.first = (int)std::ceil(q);
    g.half = nsw0 / 2 - 1;
    g.nsw = 2 * g.half;
    g.nper = (int)std::floor((double)sample_rate / floor_hz);
    g.halfper = g.nper / 2 + 1;
    g.maxlag = g.nsw / 3 + 2 < g.nsw ? g.nsw / 3 + 2 : g.nsw;
    g.brent = g.nsw / 2;
    g.n_lag = g.brent + 1;
    return g;
}

// frames of an L-sample utterance: floor((L dx - 3 / floor) / dt) + 1 from integers
inline __host__ __device__ int pitch_frames(int L, int first, int hop) { return L >= first ? (L - first) / hop + 1 : 0; }

struct PitchParams {
    const float* wav;        // [B][wav_ld]
    const int* lens;         // [B] or null
    const double* win;       // [nsw]: the Hanning window w
    const double* wr;        // [n_lag]: its normalised autocorrelation
    double* gpeak;           // workspace [B]: the global peak
    double* acf;             // [B][frames_ld][n_lag]   (the caller's, or workspace)
    double* cand;            // [B][frames_ld][15][2]   (the same)
    int* n_cand;             // [B][frames_ld]          (the same)
    double* intensity;       // [B][frames_ld]          (the same)
    unsigned char* psi;      // workspace [B][frames_ld][PITCH_PSI]: the backpointers
    double* f0;              // [B][frames_ld]
    int* n_frames;           // [B]
    int* selected;           // [B][frames_ld] or null
    double sr, floor_hz, ceiling, vt, st, oc, oj, vu;   // oj, vu: already times corr = 0.01 / dt
    int B, wav_ld, frames_ld, hop;
    PitchGeometry g;
};

hipError_t pitch_stats_launch(const PitchParams& p, hipStream_t stream);
hipError_t pitch_acf_launch(const PitchParams& p, hipStream_t stream);
hipError_t pitch_candidates_launch(const PitchParams& p, hipStream_t stream);
hipError_t pitch_path_launch(const PitchParams& p, hipStream_t stream);

} // namespace dtts
