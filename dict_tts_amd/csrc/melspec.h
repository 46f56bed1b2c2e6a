// Log-mel spectrogram of a batch of waveforms in one launch (melspec.hip): the vocoder's wav2spec direction
// (vocoders/base_vocoder.py:36-53 -> data_gen/tts/data_gen_utils.py:93-147 with vocoder='pwg', no loudness normalisation, no trimming).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

namespace dtts {

constexpr int MELSPEC_LDS_BYTES = 160 * 1024;
constexpr int MELSPEC_MAX_MELS = 128;
constexpr int MELSPEC_CHUNK = 4;   // MFMA steps (of two samples) per fp32 chain of the contraction; the chains are joined in fp64.  Divides 16.

struct MelspecParams {
    const float* wav;        // [B][wav_ld]
    const int* wav_lens;     // [B] samples, or null = wav_ld
    float* mel;              // [B][mel_cap][n_mels]
    int* mel_lens;           // [B] out, or null
    float* lin;              // [B][mel_cap][n_mels] out, or null: the mel values before the floor and the logarithm
    const float4* basis;     // melspec_pack_basis
    const float4* melpack;   // melspec_pack_mel
    int B, wav_ld, mel_cap, hop, n_fft, n_mels;
    int sg_lo, sg_hi;        // the 32-sample super-groups of the contraction that the (centred) window does not zero (both multiples of four)
    int tt;                  // frames per tile (<= 32 * waves: what fits the LDS at this hop)
    int ntile;               // tiles per utterance at wav_ld samples
    int ps;                  // slab skew: sample a of the tile lives at LDS dword a + (a >> ps)
    float eps;
};

// The one predicate of the supported set (finaliser and launcher): n_fft in {512, 1024, 2048}, 1 <= win <= n_fft, 1 <= hop <= n_fft,
// 1 <= n_mels <= 128.  *why names the offending value.
bool melspec_supported(int n_fft, int hop, int win, int n_mels, std::string* why = nullptr);

// worst conflict degree of the kernel's A-fragment read (ds_read_b32: 32 banks, the two 32-lane halves are separate groups) at this hop
// and skew, over every phase of the contraction index; tools/lds_conflicts_melspec.py restates it
int melspec_conflict_degree(int hop, int ps);
int melspec_skew_shift(int hop);   // the skew the launcher takes: the smallest degree, ties to the smaller pad

// LDS dwords of a tile of tt frames
inline size_t melspec_slab_dwords(int tt, int hop, int n_fft, int ps) {
    const size_t P = (size_t)(tt - 1) * hop + n_fft;
    return P + (P >> ps) + 1;
}
int melspec_tile_frames(int waves, int hop, int n_fft, int ps);

// fp64 on the host, rounded once to fp32, in the order the kernel walks them
std::vector<float> melspec_pack_basis(int n_fft, const std::vector<float>& window);
std::vector<float> melspec_pack_mel(int n_fft, int n_mels, const std::vector<float>& mel_basis);

hipError_t melspec_launch(const MelspecParams& p, int n_cu, hipStream_t stream);

} // namespace dtts
