// Log-mel spectrogram of a batch of waveforms in one launch (melspec.hip): the vocoder's wav2spec direction
// (vocoders/base_vocoder.py:36-53 -> data_gen/tts/data_gen_utils.py:93-147 with vocoder='pwg', no loudness normalisation, no trimming).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "stft_core.h"

namespace dtts {

constexpr int MELSPEC_MAX_MELS = 128;

struct MelspecParams {
    const float* wav;        // [B][wav_ld]
    const int* wav_lens;     // [B] samples, or null = wav_ld
    float* mel;              // [B][mel_cap][n_mels]
    int* mel_lens;           // [B] out, or null
    float* lin;              // [B][mel_cap][n_mels] out, or null: the mel values before the floor and the logarithm
    const float4* melpack;   // melspec_pack_mel
    StftGeom g;              // tt <= 32 * waves; tt and ntile are set by melspec_launch
    int B, wav_ld, mel_cap, n_mels;
    float eps;
};

// fp64 on the host, rounded once to fp32, in the order the kernel walks it
std::vector<float> melspec_pack_mel(int n_fft, int n_mels, const std::vector<float>& mel_basis);

hipError_t melspec_launch(const MelspecParams& p, int n_cu, hipStream_t stream);

} // namespace dtts
