// The d-vector speaker encoder (spkenc.hip; dtts_text2mel_fetch(DTTS_OUT_SPKENC)): Resemblyzer's VoiceEncoder — a 40-band power-mel front
// end at 16 kHz (n_fft 400, hop 160), partial utterances of 160 frames, nn.LSTM(40, 256, 3), relu(Linear(256, 256)), the row norm, the mean
// over an utterance's partials and the norm again.  A SEQUENCE is one partial (or, from mels, one row of the batch); sequences are numbered
// utterance after utterance, n = first[b] + i, by a prefix sum over the partial counts formed on the device.  Every launch addresses a
// sequence by its own table entries only and every sum has a fixed order, so a sequence's bits do not depend on its tile neighbours.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dicttts_hip.h"
#include "conv1d.h"

namespace dtts {

constexpr int SPK_NFFT = 400, SPK_HOP = 160, SPK_BINS = 201, SPK_MELS = 40, SPK_PART = 160, SPK_H = 256, SPK_G = 1024, SPK_LAYERS = 3;
constexpr int SPK_MEL_FRAMES = 16;              // frames of one workgroup of the front end
constexpr int SPK_MEL_CHAIN = 25;               // FIXED: consecutive n of one fma chain of the DFT (16 chains, summed 4 by 4 in order)
constexpr int SPK_MEL_THREADS = 448;            // >= 2 * SPK_BINS columns (re, im of every bin), a multiple of 64
constexpr int SPK_HP = SPK_H + 4;               // LDS row pitch of h: 16 B aligned, consecutive rows 4 banks apart
constexpr int SPK_TILE = 32;                    // rows of the MFMA tile = the most sequences of a workgroup

// W_hh packed for spkenc_lstm_kernel: wave w owns the hidden units [32 w, 32 w + 32) of all four gates.  Per (w, Q = k-step of 8, gate q,
// lane l) four floats, the B operand of four successive v_mfma_f32_32x32x2_f32: element e holds W_hh[q * 256 + 32 w + (l & 31)][8 Q + 4 (l >> 5) + e].
// A wave's loads of one (Q, q) are one contiguous 1 KiB piece, of one Q 4 KiB, of a step 128 KiB read front to back.
inline size_t spkenc_whh_index(int w, int Q, int q, int l, int e) { return ((((size_t)w * 32 + Q) * 4 + q) * 64 + l) * 4 + e; }

struct SpkLayer {
    PackedConv proj;           // W_ih as a k = 1 convolution with bias b_ih + b_hh (ENG_F32)
    float* whh = nullptr;      // packed as above
};

// partials of an utterance of L samples before the coverage rule, the zero-padded length and the mel frames (Resemblyzer's
// compute_partial_slices / embed_utterance / librosa's centred frames)
inline int spkenc_steps(int L, int frame_step) { return std::max(1, (L / SPK_HOP + 1) - SPK_PART + frame_step + 1); }
inline int spkenc_max_partials(int L, int frame_step) { return (spkenc_steps(L, frame_step) - 1) / frame_step + 1; }
inline int spkenc_frames_ld(int wav_ld, int frame_step) {
    const int stop = SPK_HOP * ((spkenc_max_partials(wav_ld, frame_step) - 1) * frame_step + SPK_PART);
    return 1 + std::max(wav_ld, stop) / SPK_HOP;
}

} // namespace dtts
