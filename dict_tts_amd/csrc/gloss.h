// The gloss encoder behind the dictionary's `dict_embed` (gloss.hip; dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)): the first layers of a RoFormer on a RAGGED batch
// of glosses, packed back to back as one sequence [sum_L][C] with offsets tok_off[n + 1] (the layout of the resident dictionary table).
// A row's arithmetic never depends on its neighbours: the dense layers run on conv1d_launch (k = 1, exact fp32 products, fixed order),
// the kernels here are the embedding stage, the rotary self-attention over a gloss's own tokens and the LayerNorm that keeps the running
// sum of the hidden states.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv1d.h"

namespace dtts {

constexpr int GLOSS_DK = 64;        // head width: the rotary table and the attention kernel's register tiles are built for it
constexpr int GLOSS_MAX_L = 64;     // tokens per gloss: a query row per lane of a wave
constexpr int GLOSS_QLD = 68;       // LDS row pitch (floats) of the q' / k' / ctx tile: a lane's own row reads as 16-byte pieces without conflicts

struct GlossLayer {
    PackedConv qkv, o, ffn1, ffn2;   // Wq | Wk | Wv packed as one 1x1 layer; attention.output.dense; intermediate.dense; output.dense
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;   // attention.output.LayerNorm, output.LayerNorm
};

// acc[r] = E = table[ids[r]] + (x[r] = LN(E + tt0)), x[r] likewise: the sum of the first two terms of the mean.  An id outside
// [0, vocab) gives a zero E row; status[0] = first offending row + 1, status[1] = its id (0 / 0: every id valid).  No atomics.
hipError_t gloss_embed_launch(const int64_t* ids, const float* table, int vocab, const float* tt0, const float* gamma, const float* beta, float eps,
                              float* x, float* acc, int64_t* status, int rows, int C, hipStream_t s);

// ctx [sum_L][C] = softmax(rot(q) rot(k)^T / 8) v per gloss and head of 64 channels, on qkv [sum_L][3 C] (q | k | v).  rot [64][32] holds
// (sin, cos)(p / 10000^(2 j / 64)) rounded from fp64.  L_ld >= every gloss's length (<= GLOSS_MAX_L) sizes the LDS tiles only.
hipError_t gloss_attn_launch(const float* qkv, float* ctx, const int* tok_off, const float2* rot, int n_gloss, int C, int L_ld, hipStream_t s);
size_t gloss_attn_lds(int L_ld);

// x[r] = LN(x[r]) in place (biased variance, as layernorm_launch), acc[r] += x[r]; with out: out[r] = acc[r] / div instead of storing acc
hipError_t gloss_ln_acc_launch(float* x, const float* gamma, const float* beta, float eps, float* acc, float* out, float div, int rows, int C,
                               hipStream_t s);

} // namespace dtts
