// Kernels of the PortaSpeech baseline's linguistic front (modules/portaspeech/model.py::PortaSpeech, dur_level: word): the phoneme
// encoder's relative-position self-attention and LayerNorm + ReLU, the word spans of ph2word / mel2word with the status word, phoneme ->
// word pooling, per-word duration sums, the sinusoidal word positions, and the attention of every mel frame over the phonemes of its
// own word.  All activations are channels-last fp32 [B][T][C]; no atomics, every sum in a fixed order: a row's bits depend on its own
// utterance alone, not on the batch or the padded widths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dtts {

constexpr int PS_MAX_WINDOW = 8;   // window_size of the relative attention (the reference's 4): 2 w + 1 <= 17 band slots
constexpr int PS_MAX_HIDDEN = 512; // lanes over the channels, at most 8 per lane (frame attention)

// y = relu(LayerNorm_C(x)), biased variance (ConvReluNorm: conv -> norm -> relu), every row
hipError_t ps_ln_relu_launch(const float* x, float* y, const float* gamma, const float* beta, float eps, int rows, int C, hipStream_t s);

// Relative-position multi-head self-attention on a fused qkv buffer [B][T][3C] (rel_transformer_encoder.py:127-158, window_size = w,
// heads_share): s_ij = q_i.k_j / sqrt(dk) + [|j - i| <= w] q_i.Ek[j - i + w] / sqrt(dk); keys j >= lens[b] masked; p = softmax_j;
// o_i = sum_j p_ij v_j + sum_{|j - i| <= w} p_ij Ev[j - i + w].  ek / ev: [2 w + 1][dk].  Query rows >= lens[b] are written as zeros.
// dk <= 96, w <= PS_MAX_WINDOW.
hipError_t ps_rel_attn_launch(const float* qkv, float* out, const int* lens, const float* ek, const float* ev, int window, int B, int T, int C,
                              int heads, hipStream_t s);

// One wave per utterance: checks txt_tokens / ph2word, writes the word spans wstart / wcnt [B][T_w + 1] (phonemes of word w: wstart[w] ..
// + wcnt[w]; index 0 unused), the phoneme positions ph_pos [B][T_ph] = rank in the word / phonemes of the word (0 where ph2word = 0 or
// past the live prefix) and ustat [B][4] = {0, 0, 0, 0} or {b + 1, code, value, position} (DTTS_PS_BAD_TOKEN / _ZERO_TOKEN / _BAD_PH2WORD;
// an utterance that fails gets empty spans, so nothing downstream indexes by its values).  Accepted: over the live prefix (len =
// #(txt > 0)) ph2word starts at 0 or 1 and grows by 0 or 1 per phoneme, up to T_w; past it it is 0.
hipError_t ps_scan_phonemes_launch(const int64_t* txt, const int64_t* ph2word, int n_phone, int B, int T_ph, int T_w, int* wstart, int* wcnt,
                                   float* ph_pos, long long* ustat, hipStream_t s);
// The same for the padded mel2word [B][T_mel]: fstart / fcnt [B][T_w + 1], ustat [B][4] with DTTS_PS_BAD_MEL2WORD (outside [0, T_w], or not
// non-decreasing over its non-zero prefix and zero behind it) or DTTS_PS_EMPTY_WORD (a frame of a word with wcnt = 0)
hipError_t ps_scan_frames_launch(const int64_t* m2w, const int* wcnt, int B, int T_mel, int T_w, int* fstart, int* fcnt, long long* ustat,
                                 hipStream_t s);
// status [4] = ustat of the first utterance that has one (or zeros); merge != 0: only where status[0] is still 0
hipError_t ps_status_launch(const long long* ustat, int B, int merge, int64_t* status, hipStream_t s);

// word_in[b, w - 1] = mean of ph_out[b, t] over the span of word w (ascending t, fp32; an empty word: a zero row)   (utils.py:3-17)
hipError_t ps_segment_mean_launch(const float* ph_out, const int* wstart, const int* wcnt, float* word_in, int B, int T_ph, int T_w, int C,
                                  hipStream_t s);
// dur_w[b, w - 1] = sum of dur_ph[b, t] over the span of word w (ascending t); ilens_w[b] = min(ilens_ph[b], T_w)   (model.py:316-323)
hipError_t ps_dur_sum_launch(const float* dur_ph, const int* wstart, const int* wcnt, const int* ilens_ph, float* dur_w, int* ilens_w, int B,
                             int T_ph, int T_w, hipStream_t s);

// out[row] = [src[row] | sin(pos f_i), cos(pos f_i)], [rows][2C]; freq [C / 2]   (attention's torch.cat([., pos], -1), SinusoidalPosEmb)
hipError_t ps_cat_phonemes_launch(const float* ph_out, const float* ph_pos, const float* freq, float* out, int rows, int C, hipStream_t s);
// per frame: e = pad0(weo)[mel2word], pos = rank of the frame in its word / frames of the word (0 where mel2word = 0);
// out[row] = [e | sin-pos], x_mask[row] = mel2word > 0
hipError_t ps_cat_frames_launch(const float* weo, const int64_t* m2w, const int* fstart, const int* fcnt, const float* freq, float* out,
                                float* x_mask, int B, int T_mel, int T_w, int C, hipStream_t s);

// Single-head attention of every frame over the phonemes of its word: q [B*T_mel][C] (scaled), kv [B*T_ph][2C] (k | v), a wave per frame,
// lanes over the channels, the span walked in ascending order with an online softmax (exact for a span of 1: weight 1, o = v).
// att [B*T_mel][C] = sum_t w_t v_t (zeros for a frame without a word or whose word has no phonemes); attn [B*T_mel][T_ph] or null: the
// weights, zeros outside the span and on frames with mel2word = 0.  C a multiple of 64, <= PS_MAX_HIDDEN.
hipError_t ps_frame_attn_launch(const float* q, const float* kv, const int64_t* m2w, const int* wstart, const int* wcnt, float* att, float* attn,
                                int B, int T_mel, int T_ph, int T_w, int C, hipStream_t s);

} // namespace dtts
