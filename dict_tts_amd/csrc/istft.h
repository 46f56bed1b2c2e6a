// STFT -> magnitude edit -> inverse STFT of a batch of waveforms (istft.hip): the reference's one post-filter on the vocoder's output,
// denoise(wav, v) (vocoders/vocoder_utils.py:7-15: librosa.stft, max(|S| - v, 0) with the phase kept, librosa.istft), and its two halves
// alone (_stft / _istft of utils/audio.py:35-42, Griffin-Lim's building blocks).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "stft_core.h"

namespace dtts {

constexpr int ISTFT_TILE = 32;          // frames per workgroup (one wave) of the inverse contraction: the only tile size it has
constexpr int ISTFT_GATHER = 256;       // output samples per workgroup of the overlap-add
constexpr double ISTFT_ENV_MIN = 1e-11; // torch.istft's criterion on the window envelope

// forward + edit: the shared contraction with re / im kept, S' = S max(|S| - floor, 0) / |S| written as [B][spec_cap][n_fft / 2 + 1][2]
struct SpecFwdParams {
    const float* wav;        // [B][wav_ld]
    const int* lens;         // [B] samples, or null = wav_ld
    int* frames;             // [B] out: T_b = 1 + len_b / hop
    float* spec;             // [B][spec_cap][n_fft / 2 + 1][2] out, rows < T_b
    StftGeom g;              // the basis of the (centred) window; tt and ntile are set by spectral_forward_launch
    int B, wav_ld, spec_cap;
    int csplit;              // workgroups per tile, each with n_fft / 64 / csplit bin blocks (istft_split)
    float floor;             // v >= 0; 0 = no edit (and no division)
};

// inverse DFT of every frame with the synthesis window folded in: fr[b][t][n] = w[n] irfft(S'[b][t])[n]
struct SpecInvParams {
    const float* spec;       // [B][spec_cap][n_fft / 2 + 1][2]
    const int* frames;       // [B] T_b (clamped to 0 .. tcap)
    float* fr;               // [B][spec_cap][n_fft] out, rows < T_b
    const float4* wi;        // istft_pack_inverse
    int B, spec_cap, tcap, n_fft, ntile;
    int csplit;              // workgroups per tile, each with n_fft / 64 / csplit pairs of sample blocks (istft_split)
};

// overlap-add in ascending frame order, division by the window envelope of the covering frames, n_fft / 2 samples dropped at both ends
struct SpecGatherParams {
    const float* fr;         // [B][spec_cap][n_fft]
    const int* frames;       // [B]
    const double* w2;        // [n_fft]: the window's squares
    float* out;              // [B][wav_ld]: samples < out_len_b = hop (T_b - 1) are written
    int* out_lens;           // [B] out, or null
    int B, spec_cap, tcap, wav_ld, hop, n_fft, nchunk;
};

// Wi[n][q] in the fragment order of the inverse contraction, fp64 rounded once: q = 0 -> w[n] / N (re[0]), q = 1 -> w[n] (-1)^n / N
// (re[N / 2], which rides in the im slot of bin 0), q = 2 k -> 2 w[n] cos(2 pi k n / N) / N, q = 2 k + 1 -> -2 w[n] sin(2 pi k n / N) / N.
// Order: [sample block pair c][super-group sg][part][lane][4]: parts 0 .. 3 = MFMA steps 0-3 .. 12-15 of sample block 2 c, 4 .. 7 = of
// block 2 c + 1; step j of super-group sg contracts q = 32 sg + 16 (lane >> 5) + j; sample n = 32 block + (lane & 31).
std::vector<float> istft_pack_inverse(int n_fft, const std::vector<float>& window);

// The smallest window envelope any kept sample of any utterance can see at this hop: that of a two-frame signal,
// min over p in [N / 2, N / 2 + hop) of w^2[p] (p < N) + w^2[p - hop] (p >= hop); every longer signal adds non-negative terms to it.
double istft_envelope_min(const std::vector<float>& window, int hop);

hipError_t spectral_forward_launch(SpecFwdParams p, int n_cu, hipStream_t stream);
int istft_split(long long tiles, int blocks, long long want);   // workgroups per tile: a power of two <= blocks

// The forward launcher's rule — what it refuses, the tile (stft_tile_waves), the split of a tile's bin blocks over workgroups — for ANY
// kernel pair K2 / K4 (two and four waves) of the signature (SpecFwdParams, extra ...): spectral_fwd_kernel, and Griffin-Lim's projection
// (griffinlim.hip), which is the same contraction with another epilogue and one more argument.  Written here and nowhere else.
template <int WT, auto Kern, class... X>
hipError_t spectral_fwd_cfg(SpecFwdParams p, int n_cu, hipStream_t stream, X... extra) {
    const size_t lds = stft_set_tile(p.g, WT, p.wav_ld);
    p.csplit = istft_split((long long)p.g.ntile * p.B, p.g.n_fft / 64, 4LL * n_cu);
    if (lds > (size_t)MELSPEC_LDS_BYTES || (long long)p.g.ntile * p.B * p.csplit > INT_MAX) return hipErrorInvalidValue;
    if (hipError_t e = stft_lds_limit<Kern>()) return e;
    hipLaunchKernelGGL(Kern, dim3((unsigned)(p.g.ntile * p.B * p.csplit)), dim3(64 * WT), lds, stream, p, extra...);
    return hipGetLastError();
}

template <auto K2, auto K4, class... X>
hipError_t spectral_forward_pick(const SpecFwdParams& p, int n_cu, hipStream_t stream, X... extra) {
    if (!stft_geom_ok(p.g, p.B, p.wav_ld)) return hipErrorInvalidValue;
    if (p.spec_cap < 1 + p.wav_ld / p.g.hop || !p.frames || !p.spec || ((uintptr_t)p.spec & 7)) return hipErrorInvalidValue;
    return stft_tile_waves(p.B, p.wav_ld, p.g.hop, p.g.n_fft, p.g.ps, n_cu) == 2 ? spectral_fwd_cfg<2, K2>(p, n_cu, stream, extra...)
                                                                                : spectral_fwd_cfg<4, K4>(p, n_cu, stream, extra...);
}
hipError_t istft_frames_launch(SpecInvParams p, int n_cu, hipStream_t stream);
hipError_t istft_gather_launch(const SpecGatherParams& p, hipStream_t stream);

} // namespace dtts
