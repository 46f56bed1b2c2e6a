/*
 * libdicttts_hip.so — C ABI of the MI355X (gfx950) Dict-TTS inference hot path.
 *
 * The reference (Zain-Jiang/Dict-TTS) is pure Python/PyTorch and has no FFI; the two plugin points this
 * library sits behind are:
 *   - the acoustic model  PortaSpeech_dict.forward(..., infer=True)     modules/dict_tts/model.py:36-62
 *   - the vocoder         HifiGAN.spec2wav(mel[T,80]) -> wav[T*256]      vocoders/hifigan.py:54-62
 * The Python shims in dict_tts_amd/ (model.py, vocoder.py) keep those signatures and call the entry points
 * below through ctypes.  No torch types cross this boundary: plain pointers, sizes and a hipStream_t.
 *
 * Conventions
 *   - every function returns 0 on success or a negative DTTS_E_* code; the message is dtts_last_error().
 *   - "dev" pointers are DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()), contiguous,
 *     row-major in the reference's layouts.  "host" pointers are ordinary host memory.
 *   - a handle is single-owner and not thread-safe; all work is enqueued on the caller's stream.  The only
 *     host synchronisation on the path is the T_mel scalar read in dtts_text2mel_encode().
 */
#ifndef DICTTTS_HIP_H
#define DICTTTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the entry points declared here (DTTS_API) are exported. */
#if defined(__GNUC__)
#define DTTS_API __attribute__((visibility("default")))
#else
#define DTTS_API
#endif

typedef struct dtts_ctx* dtts_handle;
typedef void* dtts_stream; /* hipStream_t */

#define DTTS_OK 0
#define DTTS_E_INVAL (-22)   /* bad argument / shape                       */
#define DTTS_E_NOMEM (-12)   /* device allocation failed                   */
#define DTTS_E_NOENT (-2)    /* a required weight tensor was never loaded  */
#define DTTS_E_STATE (-1)    /* call order violated (e.g. decode before encode) */
#define DTTS_E_HIP (-5)      /* a HIP runtime call failed                  */

#define DTTS_F32 0
#define DTTS_I64 1
#define DTTS_F64 2 /* dtts_load_weight takes it for the "resample." tensors only */

/* Largest sense index (key_map / pinyin_map value) a word may carry: the S2PA kernel keeps 16 sense slots, index 0 = "no
 * sense".  zh-dict.json holds at most 6 pronunciations per character.  Larger indices are rejected (DTTS_E_INVAL) by dtts_dict_table_upload and, on the
 * tensor API, at the T_mel synchronisation of dtts_text2mel_encode; with teacher-forced mel2word (no synchronisation) they
 * are not checked and get weight 0. */
#define DTTS_MAX_SENSES 15

/* vocoder arithmetic (fp32 accumulation and an fp32 residual stream in every mode).
 *   DTTS_VOC_F16 (default): the fused kernels with fp16 MFMA operands in the ResBlocks and bf16 hi/lo split operands (three
 *     products) in the six serial convolutions (conv_pre, upsamplers, conv_post: 3 % of the FLOPs but 87 % of the 16-bit
 *     rounding noise, tools/precision_sim.py) — waveform RMS error vs the fp32 reference ~5e-5 (gate 1e-4);
 *     activations saturate at the fp16 maximum 65504.
 *   DTTS_VOC_BF16: the same kernels on bf16 operands throughout — RMS error ~1e-3 (fails the waveform gate), a few % faster.
 *   DTTS_VOC_BF16X3: every convolution on split operands on the generic kernel — fp32-class (~2e-6), several times slower. */
#define DTTS_VOC_BF16 0
#define DTTS_VOC_BF16X3 1
#define DTTS_VOC_F16 2

/* Model hyper-parameters.  Field <- reference hparams key (resolved values, SURVEY.md §5 "Config / flags"). */
typedef struct dtts_config {
    int32_t hidden_size;          /* hidden_size 192                         egs/egs_bases/tts/ps_flow.yaml:10 */
    int32_t num_heads;            /* num_heads 2                             egs/egs_bases/tts/base.yaml:70    */
    int32_t enc_ffn_kernel_size;  /* enc_ffn_kernel_size 5                   ps_flow.yaml:11                   */
    int32_t enc_layers;           /* 4, hard-coded at modules/dict_tts/layers/dict_encoder.py:104-128         */
    int32_t gloss_dim;            /* 768: key/value size of S2PAAttention    dict_encoder.py:18                */
    int32_t word_size;            /* word_size 8000                                                          */
    int32_t value_embedding_size; /* value_embedding_size 185                                                */
    int32_t n_phone;              /* rows of the unused phoneme embedding (len(phone_set)+3)                  */
    int32_t audio_num_mel_bins;   /* 80                                      base.yaml:50                      */
    int32_t latent_size;          /* 16                                      ps_flow.yaml:25                   */
    int32_t fvae_enc_dec_hidden;  /* 192                                                                      */
    int32_t fvae_kernel_size;     /* 5                                                                        */
    int32_t fvae_dec_n_layers;    /* 4                                                                        */
    int32_t fvae_enc_n_layers;    /* 8 (posterior encoder: the posterior pass, DTTS_OUT_POSTERIOR)             */
    int32_t prior_glow_hidden;    /* 64                                      ps_flow.yaml:32                   */
    int32_t glow_kernel_size;     /* 3                                                                        */
    int32_t prior_glow_n_blocks;  /* 4                                                                        */
    int32_t prior_glow_n_layers;  /* 4, hard-coded at modules/dict_tts/fvae_semantics.py:78-79                */
    int32_t dur_predictor_layers; /* 3                                       ps_flow.yaml:17-22                */
    int32_t dur_predictor_kernel; /* 5                                                                        */
    int32_t dur_chans;            /* 128, hard-coded at modules/portaspeech/model.py:164-169                  */
    int32_t frames_multiple;      /* 4                                       ps_flow.yaml:61                   */
    int32_t language_zh;          /* language == 'zh' -> add_pron_rule       layers/utils.py:109-115           */
    /* HifiGAN generator                                                    egs/egs_bases/tts/vocoder/hifigan.yaml:3-10 */
    int32_t upsample_initial_channel; /* 512 */
    int32_t n_upsamples;              /* 4   */
    int32_t upsample_rates[8];        /* 8,8,2,2   */
    int32_t upsample_kernel_sizes[8]; /* 16,16,4,4 */
    int32_t n_resblock_kernels;       /* 3   */
    int32_t resblock_kernel_sizes[4]; /* 3,7,11 */
    /* One row per resblock kernel size.  The block type of the generator (modules/hifigan/hifigan.py:109, config key `resblock`) is
     * encoded in the rows: three dilations >= 1 = ResBlock1 (`resblock: "1"`, state-dict names resblocks.N.convs1.M / convs2.M);
     * a row whose THIRD entry is 0 is a two-dilation row = ResBlock2 (`resblock: "2"`, the V3 family: (d0, d1, 0), names
     * resblocks.N.convs.{0,1}).  All used rows are of one kind and the first two dilations are >= 1, else dtts_create fails with
     * DTTS_E_INVAL.  DTTS_VOC_F16 / DTTS_VOC_BF16 run a ResBlock2 as one fused launch for widths 32 / 64 / 128 / 256, odd kernels
     * 3..11 and every pair (d0, d1) whose halo (K - 1) / 2 * (d0 + d1) leaves at least 32 output rows in a tile of 512 / 512 / 256 /
     * 128 rows within the LDS (dict_tts_amd/csrc/rb2x.h: rb2x_supported); other shapes run convolution by convolution in
     * DTTS_VOC_BF16 and DTTS_VOC_BF16X3 and are refused by dtts_finalize_weights in DTTS_VOC_F16.  tune_flags bits 9 / 12 / 14 / 15
     * concern ResBlock1 kernels only and do not change a ResBlock2 result.  A ResBlock1 runs as one fused launch at widths 32 / 64
     * (every odd kernel 3..11) and 128 / 256 (k = 3; other kernels per iteration), and at the narrow widths 16 / 8 of the V2 generators
     * (upsample_initial_channel 128) for odd kernels 3..11 and every dilation triple whose halo (K - 1) / 2 * (d0 + d1 + d2 + 3)
     * leaves at least 32 output rows in a 256-row tile under the fused conv_post (dict_tts_amd/csrc/rbn.h: rbn_supported); a last
     * stage of 32, 16 or 8 channels gets conv_post + tanh in its last ResBlock's launch.  tune_flags bits 9 / 12 / 14 / 15 do not
     * change a result at the narrow widths. */
    int32_t resblock_dilation_sizes[4][3]; /* (1,3,5) x3 */
    int32_t vocoder_precision;        /* DTTS_VOC_F16 (default) | DTTS_VOC_BF16 | DTTS_VOC_BF16X3; DTTS_VOC_F16 needs ResBlock widths 8 / 16 / 32 / 64 / 128 / 256 */
    /* FFT block stack (FFTBlocks, modules/fastspeech/tts_modules.py:458-493); width = hidden_size, heads = num_heads */
    int32_t fft_layers;               /* dec_layers 4                          egs/egs_bases/tts/base.yaml:68 */
    int32_t fft_kernel_size;          /* dec_ffn_kernel_size 9                 base.yaml:72                   */
    int32_t fft_use_pos_embed;        /* FFTBlocks(use_pos_embed=True)                                        */
    int32_t fft_use_last_norm;        /* FFTBlocks(use_last_norm=True)                                        */
    int32_t vocoder_unfused;          /* testing aid, DTTS_VOC_BF16 only: 1 = one kernel per convolution instead of the fused ResBlock kernels */
    int32_t decoder_fp32;             /* 1 = FVAE decoder WaveNet on exact fp32 MFMA (round 1); 0 (default) = bf16 hi/lo split operands */
    int32_t vocoder_range_guard;      /* DTTS_VOC_F16: 1 = start with the fp16 range guard on (dtts_vocoder_range_guard) */
    int32_t debug_redzone;            /* testing aid: 1 = memory-safety mode — every workspace buffer and weight pack sits between 4 KiB red
                                         zones, workspaces are filled with 0xFF (NaN) before each forward; dtts_debug_check verifies the zones.
                                         2 = the same, and (self-test of the whole-ResBlock launcher) every such launch of dtts_hifigan_forward declares
                                         its weight packs to be in the OTHER MFMA fragment order than they are in: the launcher must refuse them, the
                                         forward fails with DTTS_E_HIP before that kernel runs */
    int32_t tune_flags;               /* A/B switches of tuning experiments (tools/ab_libs.sh); 0 = the measured defaults.  The library never
                                         reads the process environment: arithmetic and layout follow this struct alone.
                                         The library honours exactly the bits that have a parity / bit-identity test behind them and
                                         refuses every other one (dtts_create: DTTS_E_INVAL):
                                           8  (arithmetic) prior flow launch by launch on the exact-fp32 kernels
                                           9  (schedule)   all ResBlocks of a C <= 64 stage in one launch (less HBM traffic, not faster)
                                           12 (schedule)   the first two ResBlocks of the C = 32 stage in one launch (neutral)
                                           13 (arithmetic) two-product fp16 ups.1 (eats waveform margin)
                                           14 (schedule)   512-row tiles for every k at C = 64
                                           15 (arithmetic) fp32 stream between the three iterations of the C >= 128, k >= 7 ResBlocks (round 5's
                                                           form; the default stores it as fp16: half the bytes, waveform error 5.3e-5 -> 6.7e-5)
                                         Bits 0-7, 10, 11, 16, 17 were closed experiments of earlier rounds; their code is retired
                                         (LABNOTES.md: retired switches) and the bits are refused like any other. */
} dtts_config;

/* Fill *cfg with the Biaobei Dict-TTS + HifiGAN defaults listed above. */
DTTS_API void dtts_default_config(dtts_config* cfg);
/* sizeof(dtts_config) as this library was compiled: a binding checks its own mirror of the struct against it. */
DTTS_API int dtts_config_sizeof(void);

/* Create / destroy a context on the current HIP device. */
DTTS_API int dtts_create(const dtts_config* cfg, dtts_handle* out);
DTTS_API void dtts_destroy(dtts_handle h);
DTTS_API const char* dtts_last_error(dtts_handle h); /* h may be NULL: message of the last failed dtts_create */

/*
 * Weight loading — replaces torch's load_state_dict for the two children the path uses:
 *   state_dict['model']      (utils/trainer.py:348-376, keys as in SURVEY.md §8a) -> names "model.<key>"
 *   state_dict['model_gen']  (vocoders/hifigan.py:16-32)                           -> names "vocoder.<key>"
 * One call per tensor, fp32 host data, the library copies it (caller keeps ownership).  Weight-norm pairs
 * arrive as <name>.weight_g / <name>.weight_v and are folded in dtts_finalize_weights (w = g*v/||v||, what
 * remove_weight_norm does at tasks/tts/ps_flow.py:262-268 and modules/hifigan/hifigan.py:144-151).
 * Unknown names (fvae.encoder.*, attn.*, enc_pos_proj.* ... — loaded but unused at inference) are accepted and ignored.
 */
DTTS_API int dtts_load_weight(dtts_handle h, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype);

#define DTTS_PART_ACOUSTIC 1
#define DTTS_PART_VOCODER 2
#define DTTS_PART_FFT 4 /* an FFTBlocks state dict loaded under "fft.<key>"  */
/* The log-mel front end (DTTS_OUT_MELSPEC below): "melspec.mel_basis" [n_mels][n_fft / 2 + 1] (librosa.filters.mel as
 * data_gen/tts/data_gen_utils.py:128-130 calls it) and "melspec.window" [win_length] (the periodic Hann window); n_fft, n_mels and win_length
 * follow from the shapes.  Supported: n_fft 512 / 1024 / 2048, 1 <= win_length <= n_fft, 1 <= n_mels <= 128, else DTTS_E_INVAL naming the
 * value.  Unlike the other parts this one is rebuilt by EVERY call that names it, from the tensors loaded last: finalising again with
 * other tensors replaces the plan (the old packs stay allocated until dtts_destroy: a launch in flight may still read them). */
#define DTTS_PART_MELSPEC 8
/* The multi-resolution STFT distance (DTTS_OUT_STFT_DISTANCE below): up to four plans, one per "stft.<i>.window" [n_fft], i = 0, 1, .. without a
 * gap.  Each window arrives as torch.stft applies it: the win_length samples (the reference: torch.hann_window(win_length), periodic) zero
 * padded to n_fft with (n_fft - win_length) / 2 zeros on the left.  n_fft is the tensor's length (512 / 1024 / 2048, else DTTS_E_INVAL naming
 * it); the samples outside the window's non-zero support are left out of the contraction.  Rebuilt by EVERY call that names it, like
 * DTTS_PART_MELSPEC.  DTTS_E_NOENT without "stft.0.window". */
#define DTTS_PART_STFT 16
/* STFT -> magnitude edit -> inverse STFT (DTTS_OUT_SPECTRAL below): ONE plan from "istft.window" [n_fft], the analysis AND synthesis window as
 * torch.stft / torch.istft apply it (the win_length samples zero padded and centred to n_fft, as "stft.<i>.window" is).  n_fft is the tensor's
 * length (512 / 1024 / 2048, else DTTS_E_INVAL naming it).  Rebuilt by EVERY call that names it, like DTTS_PART_MELSPEC.  DTTS_E_NOENT
 * without "istft.window".  Optional: "istft.inv_mel_basis" [n_fft / 2 + 1][n_mels <= 128], the pseudo-inverse of the mel filterbank that
 * DTTS_OUT_GRIFFIN_LIM's mel input goes through (another shape or a non-finite entry: DTTS_E_INVAL); a plan finalised without it has none. */
#define DTTS_PART_ISTFT 32
/* The band-limited resampler (DTTS_OUT_RESAMPLE below): the right half of a windowed sinc, "resample.filter" [n_win] and the table
 * precision "resample.num_table" [1] (samples per zero crossing), both loaded as DTTS_F64 (the only names dtts_load_weight takes that
 * dtype for).  resampy's kaiser_best is n_win = 32769, num_table = 512.  n_win - 1 must be a multiple of num_table; supported: num_table a
 * power of two <= 1024, n_win <= 2^17, finite entries, else DTTS_E_INVAL naming the value.  The plan is the table and
 * interp_delta[i] = win[i + 1] - win[i] (the last entry 0), made here on the host in fp64 with one subtraction per entry and uploaded as
 * pairs (win[i], interp_delta[i]).  Rebuilt by EVERY call that names it, like DTTS_PART_MELSPEC.  DTTS_E_NOENT without either tensor. */
#define DTTS_PART_RESAMPLE 64
/* HifiGAN's discriminators (DTTS_OUT_DISC below; state_dict['model_disc'] of a vocoder checkpoint): "disc.mpd.<i>.convs.<j>.{weight,bias}"
 * (i = 0 .. 4, j = 0 .. 4) and "disc.mpd.<i>.conv_post.{weight,bias}" = MultiPeriodDiscriminator.discriminators[i] (Conv2d weights
 * [C_out][C_in][k][1]), "disc.msd.<i>.convs.<j>.*" (i = 0 .. 2, j = 0 .. 6) and "disc.msd.<i>.conv_post.*" = MultiScaleDiscriminator's
 * (Conv1d weights [C_out][C_in / groups][k]).  The weights arrive PLAIN: weight norm and the first scale's spectral norm are folded by the
 * caller (dict_tts_amd/discriminators.py).  Channel widths, kernels, strides, groups and the periods 2, 3, 5, 7, 11 are those of
 * modules/hifigan/hifigan.py and not configurable: DTTS_E_INVAL naming the layer on any other shape, DTTS_E_NOENT naming the first missing
 * tensor.  Built once per context. */
#define DTTS_PART_DISC 128
/* The d-vector speaker encoder (DTTS_OUT_SPKENC below; Resemblyzer's VoiceEncoder, the source of the reference's spk_embed):
 * "spkenc.lstm.weight_ih_l<k>" [1024][40 | 256], "spkenc.lstm.weight_hh_l<k>" [1024][256], "spkenc.lstm.bias_ih_l<k>" / "bias_hh_l<k>" [1024]
 * (k = 0 .. 2; torch.nn.LSTM's state-dict keys, gate order i, f, g, o), "spkenc.linear.weight" [256][256], "spkenc.linear.bias" [256],
 * "spkenc.mel_basis" [40][201] (the Slaney filterbank 0 .. 8000 Hz at 16 kHz) and "spkenc.window" [400] (the periodic Hann window).  The
 * architecture is fixed: DTTS_E_INVAL naming the tensor on any other shape, DTTS_E_NOENT naming the first missing tensor.  The windowed DFT
 * basis is formed here on the host in fp64 and rounded once; W_hh is repacked into the operand order of the recurrent kernel.  Built once
 * per context. */
#define DTTS_PART_SPKENC 256
/* The acoustic checkpoint's multi-window mel discriminator (DTTS_OUT_MELDISC below; state_dict['mel_disc'] of a Dict-TTS checkpoint,
 * modules/fastspeech/multi_window_disc.py::Discriminator without cond_disc).  Window w = 0 .. n - 1 (32, 64, 128 frames), block l = 0 .. 2:
 *   "meldisc.<w>.conv.<l>.weight" [H][1 | H][3][3] and ".bias" [H]: the Conv2d of block l, PLAIN (spectral norm folded by the caller);
 *   "meldisc.<w>.norm.<l>.weight" / ".bias" [H] (l = 1, 2): InstanceNorm2d(H, affine=True), statistics taken per clip on the device; OR
 *   "meldisc.<w>.affine.<l>.scale" / ".shift" [H] (l = 1, 2): BatchNorm2d in eval mode folded by the caller to x * scale + shift; neither
 *   of the two = no norm (disc_norm: sn);
 *   "meldisc.<w>.adv.weight" [1][H * (win / 8) * 10] (disc_reduction stack / sum, flattened as (c, t, f)) or [1][H * 10] (none, (c, f) per
 *   time row), and ".bias" [1].
 * H and the window count are read from the tensors.  DTTS_E_NOENT names the first missing tensor; DTTS_E_INVAL names a hidden size that is
 * not a multiple of 32 in 32 .. DTTS_MELDISC_MAX_HIDDEN, a window count outside 1 .. 3 ("meldisc.3.*" present), a layer of another shape,
 * and an adv_layer whose width does not match its window (or differs in kind between windows).  Built once per context. */
#define DTTS_PART_MELDISC 512
/* The gloss encoder (DTTS_GLOSS_ENCODE below; the first layers of the RoFormer whose hidden states the reference's binariser averages into
 * the dictionary's `dict_embed`): "gloss.<key>" with <key> the Hugging Face state-dict key without its "roformer." prefix —
 *   "gloss.embeddings.word_embeddings.weight" [vocab][hidden], "gloss.embeddings.token_type_embeddings.weight" [>= 1][hidden] (row 0 is
 *   used), "gloss.embeddings.LayerNorm.weight" / ".bias" [hidden];
 *   per layer l = 0 .. n - 1, "gloss.encoder.layer.<l>." + "attention.self.query" / "key" / "value" / "attention.output.dense" ".weight"
 *   [hidden][hidden] and ".bias" [hidden], "attention.output.LayerNorm" / "output.LayerNorm" ".weight" / ".bias" [hidden],
 *   "intermediate.dense.weight" [ffn][hidden] + ".bias" [ffn], "output.dense.weight" [hidden][ffn] + ".bias" [hidden];
 *   "gloss.config" [4]: num_attention_heads, layer_norm_eps, rotary_value (0 / 1), hidden_act (0 = "gelu", the erf form; 1 = any other).
 * The number of layers is what was loaded (1 .. 64); the mean runs over n + 2 terms.  "encoder.embed_positions.weight" is not read: the
 * rotary table is made here, in fp64, rounded once.  Supported: hidden a multiple of 64 up to 8192, ffn (intermediate_size) a multiple of 4
 * up to 65536 (the feed-forward rows are read in 16-byte pieces), one ffn for all layers.  DTTS_E_INVAL naming the value: a hidden size that
 * is no multiple of 64, an intermediate_size that is no multiple of 4, heads of
 * another width than 64, a word-embedding width (embedding_size) other than the hidden size, rotary_value = 1, hidden_act != 0, a tensor
 * of another shape, and a tensor that a loaded layer lacks; DTTS_E_NOENT: no config / embeddings at all.  Built once per context. */
#define DTTS_PART_GLOSS 1024
/* The PortaSpeech baseline (DTTS_PS_ENCODE below; modules/portaspeech/model.py::PortaSpeech with dur_level: word, use_post_glow: false, no
 * speakers): "ps.<state-dict key>" for ph_encoder.* (emb, pre.*, encoder.* with emb_rel_k / emb_rel_v [1][2 w + 1][hidden / heads]),
 * word_encoder.* (FFTBlocks, FFN kernel 1), enc_pos_proj.*, dec_query_proj.*, dec_res_proj.*, attn.in_proj_weight, attn.out_proj.weight,
 * dur_predictor.* and fvae.* (weight norm folded here as for DTTS_PART_ACOUSTIC), and two tensors that are no state-dict keys:
 *   "ps.config" [2]: window_size (1 .. 8), word_enc_layers (1 .. 64);
 *   "ps.word_encoder.pos_table" [n_pos][hidden]: SinusoidalPositionalEmbedding.weights of the word encoder (row 0 = padding); an encode
 *   needs n_pos > T_w.
 * The encoder depth, widths and kernels come from these fields of dtts_config: enc_layers, hidden_size, num_heads, enc_ffn_kernel_size,
 * n_phone, dur_* and the FVAE fields.  DTTS_E_NOENT names the first missing tensor, DTTS_E_INVAL a tensor of another shape.  A context holds EITHER the Dict-TTS
 * acoustic part or this one: finalising the second is refused with DTTS_E_STATE.  Built once per context. */
#define DTTS_PART_PORTASPEECH 2048
/* Fold, repack into MFMA fragment order and upload.  Fails with DTTS_E_NOENT naming the first missing tensor. */
DTTS_API int dtts_finalize_weights(dtts_handle h, int parts);

/*
 * Acoustic model, phase 1 — replaces run_text_encoder (modules/dict_tts/model.py:84-110): S2PA dictionary
 * encoder, duration predictor, length regulator.  Inputs are the tensors of DictTTSDataset.collater
 * (tasks/tts/dataset_utils.py:264-302):
 *   word_tokens [B,T_w] i64 · keys, values [B,T_w,L_k,gloss_dim] f32 · key_map [B,T_w,L_k] f32 ·
 *   pinyin, pinyin_map [B,T_w,P] i64 · pron_modified [B,T_w] i64 (may be NULL = zeros) ·
 *   mel2word [B,T_m2w] i64 or NULL (teacher-forced durations, model.py:77).
 * On return *T_mel_host is the frame count padded to frames_multiple (model.py:98-100).  This call
 * synchronises the stream once to read that scalar when mel2word is NULL.
 */
DTTS_API int dtts_text2mel_encode(dtts_handle h, const int64_t* word_tokens_dev, const float* keys_dev, const float* values_dev,
                         const float* key_map_dev, const int64_t* pinyin_dev, const int64_t* pinyin_map_dev,
                         const int64_t* pron_modified_dev, const int64_t* mel2word_dev, int T_m2w, int B, int T_w, int L_k,
                         int P, int32_t* T_mel_host, dtts_stream stream);

/*
 * Resident dictionary: the reference ships keys + values [B,T_w,L_k,768] f32 host->device for every
 * batch (tasks/tts/dataset_utils.py:305-330 looks every character up in the ``dict_embed`` indexed dataset and pads) —
 * ~1.5 GB at B=60.  Uploaded once, the ragged table (one entry per dictionary word: gloss embeddings [L_e,768],
 * key_map [L_e], pinyin / pinyin_map [P_e]; items of data_gen/tts/binarizer_zh.py:301-309) stays in HBM and a batch
 * carries only ids.  All pointers are HOST pointers; values may be NULL (the reference stores value == key).
 * What stays resident is the PROJECTED table: K = k_transform(key), V = v_transform(value), hidden_size floats per row each
 * (modules/dict_tts/layers/dict_encoder.py:36-39 projects every gloss row of every batch; here once, on the device, at upload):
 * 2 * hidden_size * 4 = 1,536 B per gloss row instead of 3,072 (6,144 with separate values), and the id path computes
 * logits = K . q and context = Wo sum_l w_l V_l in the reference's own association order.  Consequences: the acoustic weights
 * must be finalized BEFORE this call (DTTS_E_STATE otherwise), and re-loading them requires a new upload.
 */
DTTS_API int dtts_dict_table_upload(dtts_handle h, int n_entries, const int32_t* tok_off_host, const float* keys_host,
                           const float* values_host, const float* key_map_host, const int32_t* pin_off_host,
                           const int64_t* pinyin_host, const int64_t* pinyin_map_host);
/*
 * dtts_text2mel_encode with the dictionary tensors replaced by entry ids [B,T_w] i32 (device): >= 0 a table entry,
 * -1 the BOS / last row the collater pads onto every sentence (zero vectors, key_map = pinyin_map = 1), -2 batch
 * padding.  L_k / P are the batch maxima the collated tensors would have had (they size dict_attn / pron_attn).
 * Results are identical to dtts_text2mel_encode on the tensors collated from the same table.
 * An entry with more gloss rows than L_k or more pinyin slots than P would lose the rest silently (the kernel clamps): with
 * predicted durations such a batch is rejected (DTTS_E_INVAL, naming both maxima) at the T_mel synchronisation; with
 * teacher-forced mel2word there is no synchronisation and NO check: the caller guarantees that L_k / P are the batch maxima
 * (and, on both APIs, that no sense index exceeds DTTS_MAX_SENSES, see there).  The maxima are taken over EVERY slot with an
 * entry id >= 0, also those of words past their utterance's end (word_tokens == 0), whose rows never reach an output: the
 * collated tensors would have been sized for them too.  Entry ids must be < n_entries; they are not checked.
 */
DTTS_API int dtts_text2mel_encode_ids(dtts_handle h, const int64_t* word_tokens_dev, const int32_t* entry_ids_dev,
                             const int64_t* pron_modified_dev, const int64_t* mel2word_dev, int T_m2w, int B, int T_w, int L_k,
                             int P, int32_t* T_mel_host, dtts_stream stream);

/*
 * Speaker conditioning — replaces spk_embed_proj and the add of modules/dict_tts/model.py:44-45,94-96 (multi-speaker checkpoints such as
 * the WenetSpeech configuration: use_spk_embed / use_spk_id with num_spk > 1).  The projection is an optional part of the acoustic weights:
 * "model.spk_embed_proj.weight" [hidden][256] + "model.spk_embed_proj.bias" [hidden] = nn.Linear(256, hidden) (use_spk_embed), or
 * "model.spk_embed_proj.weight" [num_spk][hidden] alone = Embedding(num_spk, hidden) (use_spk_id); dtts_finalize_weights(DTTS_PART_ACOUSTIC)
 * packs it when present and rejects any other shape (DTTS_E_INVAL).
 *
 * dtts_text2mel_speakers enqueues the projection of B speaker inputs (device: fp32 [B][256] for DTTS_SPK_EMBED, int64 [B] ids for
 * DTTS_SPK_ID) on `stream` at once and ARMS the next dtts_text2mel_encode / _encode_ids / _forward / _forward_ids on this handle, which
 * must be enqueued on the same stream with the same B: that encode computes word_encoder_out + spk_embed and feeds
 * (word_encoder_out + spk_embed) * nonpadding to the duration predictor and the decoder condition, as the reference does.  Every encode
 * consumes (disarms) the speakers, whether it succeeds or not; a later batch is never conditioned on them.  DTTS_E_INVAL: no speaker
 * weights, `kind` not the loaded form, B > DTTS_MAX_SPEAKER_BATCH, or (at the encode) a B that differs from the armed one.  Speaker ids
 * are bounds-checked on the device and reported at the T_mel synchronisation of the encode (DTTS_E_INVAL naming the utterance and the
 * id; the reference's nn.Embedding raises there); with teacher-forced mel2word (no synchronisation) they are not checked and an
 * out-of-range id gets a zero row.  DTTS_OUT_WORD_ENCODER_OUT of a conditioned encode is the reference's ret['word_encoder_out'] (padded
 * rows hold the speaker row); fetch it before arming the next batch (DTTS_E_STATE otherwise).
 */
#define DTTS_SPK_EMBED 1   /* fp32 [B][256] (use_spk_embed) */
#define DTTS_SPK_ID 2      /* int64 [B]      (use_spk_id)    */
#define DTTS_MAX_SPEAKER_BATCH 4096
DTTS_API int dtts_text2mel_speakers(dtts_handle h, int kind, const void* spk_dev, int B, dtts_stream stream);

/*
 * Acoustic model, phase 2 — replaces the gather-expand and run_decoder (model.py:105-121,
 * fvae_semantics.py:109-115): z_p [B,latent,T_mel/4] f32 is the prior sample (the reference draws it from the
 * CPU RNG; here it is an explicit input for parity runs) or NULL: N(0,1) drawn on the device (counter-based, a new stream
 * per call).  mel_out [B,T_mel,80] f32.
 */
DTTS_API int dtts_text2mel_decode(dtts_handle h, const float* z_p_dev, float* mel_out_dev, dtts_stream stream);

/*
 * Single-call forms and names of SURVEY.md 8(b).  dtts_text2mel_forward = dtts_text2mel_encode + dtts_text2mel_decode +
 * the two fetches every inference consumer needs, with the outputs in CAPACITY layout because T_mel is not known before the
 * call: mel_out [B, mel_cap, n_mel] (only rows < T_mel of each utterance are written), *T_mel_out (host) = padded frame
 * count, DTTS_E_INVAL if it exceeds mel_cap; z_p [B, latent, z_cap] with z_cap >= T_mel/4, or NULL = the library draws
 * N(0,1) on the device (counter-based; the reference's CPU-RNG draw, fvae_semantics.py:110-111, cannot be reproduced bit
 * for bit, so parity runs pass z_p); pron_attn [B,T_w,P] / dur [B,T_w] may be NULL.  dtts_text2mel_plan is the
 * two-phase entry (= dtts_text2mel_encode: returns T_mel after the duration kernel); dtts_load_weights = dtts_load_weight.
 */
DTTS_API int dtts_load_weights(dtts_handle h, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
DTTS_API int dtts_text2mel_plan(dtts_handle h, const int64_t* word_tokens_dev, const float* keys_dev, const float* values_dev,
                       const float* key_map_dev, const int64_t* pinyin_dev, const int64_t* pinyin_map_dev,
                       const int64_t* pron_modified_dev, const int64_t* mel2word_dev, int T_m2w, int B, int T_w, int L_k, int P,
                       int32_t* T_mel_host, dtts_stream stream);
DTTS_API int dtts_text2mel_forward(dtts_handle h, const int64_t* word_tokens_dev, const float* keys_dev, const float* values_dev,
                          const float* key_map_dev, const int64_t* pinyin_dev, const int64_t* pinyin_map_dev,
                          const int64_t* pron_modified_dev, const int64_t* mel2word_dev, int T_m2w, const float* z_p_dev, int z_cap,
                          int B, int T_w, int L_k, int P, float* mel_out_dev, int mel_cap, int64_t* T_mel_out_host,
                          float* pron_attn_dev, float* dur_dev, dtts_stream stream);
DTTS_API int dtts_text2mel_forward_ids(dtts_handle h, const int64_t* word_tokens_dev, const int32_t* entry_ids_dev,
                              const int64_t* pron_modified_dev, const int64_t* mel2word_dev, int T_m2w, const float* z_p_dev,
                              int z_cap, int B, int T_w, int L_k, int P, float* mel_out_dev, int mel_cap, int64_t* T_mel_out_host,
                              float* pron_attn_dev, float* dur_dev, dtts_stream stream);

/* Copy an intermediate of the last encode/decode into a caller buffer (device to device, on the stream). */
#define DTTS_OUT_PRON_ATTN 1        /* [B,T_w,P] f32      ret['pron_attn']          */
#define DTTS_OUT_DUR 2              /* [B,T_w] f32        ret['dur'] (log domain)   */
#define DTTS_OUT_MEL2WORD 3         /* [B,T_mel] i64                                */
#define DTTS_OUT_DICT_ATTN 4        /* [B,1,L_k,T_w] f32  ret['dict_attn']          */
#define DTTS_OUT_WORD_ENCODER_OUT 5 /* [B,T_w,hidden] f32                           */
#define DTTS_OUT_X_MASK 6           /* [B,T_mel,1] f32    ret['x_mask']             */
#define DTTS_OUT_CONTEXT 7          /* [B,T_w,hidden] f32 S2PA context              */
#define DTTS_OUT_MEL_LENS 8         /* [B] i32 frames with mel2word > 0 AFTER the padding to frames_multiple (the frames the
                                      reference's B = 1 inference vocodes: an utterance that reaches T_mel keeps its pad frames) */
/*
 * DTTS_OUT_POSTERIOR: not a copy but the teacher-forced posterior pass — PortaSpeech_dict.forward(infer=False) without gradients, as the
 * reference's validation_step runs it (modules/dict_tts/fvae_semantics.py:84-108) — on the batch of the last dtts_text2mel_encode /
 * _encode_ids, with its inputs and outputs named by a HOST argument block: dst = (dtts_posterior_args*), args->size = sizeof(*args).
 * It runs instead of dtts_text2mel_decode or in addition to it; the other items stay valid after it (X_MASK is rewritten with the same
 * values).  No host synchronisation; everything is enqueued on `stream`.  Device pointers, f32:
 *   tgt_mels [B][mel_ld][80] (mel_ld >= T_mel; 0 = exactly T_mel): the ground-truth mels; x_mask = (mel2word > 0) of the encode;
 *   eps [B][latent][eps_ld] (eps_ld >= T_mel/4; 0 = exactly T_mel/4), the posterior sample's noise, or NULL: drawn on the device from the
 *     context's noise stream (dtts_set_noise_seed makes it repeatable);
 *   mel_out [B][mel_cap][80] (mel_cap >= T_mel; 0 = exactly T_mel): the reconstruction decoder(z_q, x_mask, g); rows >= T_mel untouched;
 *   m_q, logs_q, z_p [B][latent][T_mel/4] (channel-first, as the reference returns them) and kl (a scalar): each optional (NULL = not
 *     written).  kl = sum((log q - log p) * x_mask_sqz) / sum(x_mask_sqz) / latent, reduced in a fixed order (same inputs, same bits).
 * DTTS_E_STATE before an encode, or when the checkpoint lacked fvae.encoder.* (the message names the missing tensor).  The pass has a
 * workspace of its own, reserved on its first call: the infer path's buffers and results are not touched.
 */
#define DTTS_OUT_POSTERIOR 9
typedef struct dtts_posterior_args {
    int32_t size;                 /* sizeof(dtts_posterior_args) */
    int32_t mel_ld, eps_ld, mel_cap;
    const float* tgt_mels_dev;
    const float* eps_dev;         /* or NULL */
    float* mel_out_dev;
    float* m_q_dev;               /* or NULL */
    float* logs_q_dev;            /* or NULL */
    float* z_p_dev;               /* or NULL */
    float* kl_dev;                /* or NULL */
} dtts_posterior_args;
/*
 * DTTS_OUT_MELSPEC: not a copy either, and needs NO encode — the vocoder's other direction, BaseVocoder.wav2spec (vocoders/base_vocoder.py:36-53
 * -> process_utterance, data_gen/tts/data_gen_utils.py:122-134, vocoder='pwg', no loudness normalisation, no trimming) for a batch, in one
 * launch on `stream`, no host synchronisation: dst = (dtts_melspec_args*), args->size = sizeof(*args).  Per utterance b of len_b =
 * wav_lens_dev[b] samples (clamped to [0, wav_ld]; NULL = wav_ld): n_fft / 2 zeros on both sides (librosa center=True, pad_mode='constant'),
 * T_b = 1 + len_b / hop frames of n_fft samples, the window of dtts_finalize_weights(DTTS_PART_MELSPEC) centred in the frame, |rfft|, the mel
 * basis, log10(max(eps, .)).  wav_dev f32 [B][wav_ld]; mel_dev f32 [B][mel_cap][n_mels], rows >= T_b of utterance b are left untouched;
 * mel_lens_dev i32 [B] receives T_b (or NULL); lin_dev (or NULL) receives the same rows before the floor and the logarithm.  The contraction is exact fp32 products, summed in fp32 over eight samples at a time and in fp64 across those, against a windowed DFT basis
 * computed in fp64; every utterance's result is bit-identical alone and inside any batch.  DTTS_E_STATE without a finalised plan;
 * DTTS_E_INVAL (naming the value) for a wrong size, a hop outside 1 .. n_fft, B <= 0, mel_cap < 1 + wav_ld / hop, or eps <= 0.
 */
#define DTTS_OUT_MELSPEC 10
typedef struct dtts_melspec_args {
    int32_t size;                 /* sizeof(dtts_melspec_args) */
    int32_t hop;                  /* hop_size: any integer in 1 .. n_fft */
    int32_t B, wav_ld, mel_cap;
    float eps;                    /* the floor under the logarithm (the reference: 1e-6) */
    const float* wav_dev;
    const int32_t* wav_lens_dev;  /* or NULL */
    float* mel_dev;
    int32_t* mel_lens_dev;        /* or NULL */
    float* lin_dev;               /* or NULL: f32 [B][mel_cap][n_mels], the mel values BEFORE max(eps, .) and the logarithm (accuracy tests) */
} dtts_melspec_args;
/*
 * DTTS_OUT_STFT_DISTANCE: not a copy, needs NO encode — the sums behind the reference's multi-resolution STFT figures `sc` / `mag`
 * (modules/hifigan/stft_loss.py as tasks/vocoder/hifigan.py:62-76 reports them; MultiResolutionSTFTLoss.forward(x, y): y is the recording and
 * the normaliser) for a batch of waveform PAIRS, one launch per resolution plus one reduction launch on `stream`, no host synchronisation, no
 * atomics: dst = (dtts_stft_args*), args->size = sizeof(*args).  Resolution i < n_res uses plan i of dtts_finalize_weights(DTTS_PART_STFT) at
 * hop[i].  Per utterance b of len_b = lens_dev[b] samples (clamped to [0, wav_ld]; NULL = wav_ld), as torch.stft(center=True,
 * pad_mode='reflect') of x[b, :len_b] and y[b, :len_b] alone: n_fft / 2 mirrored samples on both sides (the edge sample not repeated),
 * T_b = 1 + len_b / hop frames, n_fft / 2 + 1 bins, m = sqrt(max(re^2 + im^2, 1e-7)).
 *   sums_dev  f64 [n_res][B][3]: sum (m_y - m_x)^2, sum m_y^2, sum |log m_y - log m_x| over the utterance's T_b (n_fft / 2 + 1) values, so that
 *             sc = sqrt(sums[0] / sums[1]) and mag = sums[2] / count (pooled over a batch: add the sums and the counts first);
 *   count_dev i64 [n_res][B]: T_b (n_fft / 2 + 1); 0, with zero sums, where len_b <= n_fft / 2 (a length torch.stft refuses);
 *   mag_dev   f32 or NULL: the clamped magnitudes, resolution after resolution, each [2 (x, y)][B][mag_cap][n_fft_i / 2 + 1]; rows >= T_b
 *             are left untouched (tests and diagnosis; mag_cap >= 1 + wav_ld / hop[i] for every i).
 * The contraction is DTTS_OUT_MELSPEC's (exact fp32 products, fp32 over eight samples, fp64 across those); the sums are fp32 over 32 bins of
 * a frame, fp64 beyond, in a fixed order: the same inputs give the same bits, and an utterance's three sums are bit-identical alone and
 * inside any batch.  DTTS_E_STATE without a finalised plan; DTTS_E_INVAL (naming the value) for a wrong size, n_res outside 1 .. the number
 * of plans, a hop outside 1 .. n_fft, B <= 0, a mag_cap that is too small, or a NULL x / y / sums / count pointer.
 */
#define DTTS_OUT_STFT_DISTANCE 11
typedef struct dtts_stft_args {
    int32_t size;                 /* sizeof(dtts_stft_args) */
    int32_t n_res;                /* resolutions to run: plans 0 .. n_res - 1 */
    int32_t hop[4];               /* hop of each: any integer in 1 .. n_fft */
    int32_t B, wav_ld, mag_cap;   /* mag_cap: rows per utterance of mag_dev (ignored when mag_dev is NULL) */
    int32_t reserved;             /* 0 */
    const float* x_dev;           /* f32 [B][wav_ld]: the generated waveforms */
    const float* y_dev;           /* f32 [B][wav_ld]: the recordings (the normaliser of sc) */
    const int32_t* lens_dev;      /* or NULL */
    double* sums_dev;
    int64_t* count_dev;
    float* mag_dev;               /* or NULL */
} dtts_stft_args;
/*
 * DTTS_OUT_SPECTRAL: not a copy, needs NO encode — the reference's one post-filter on the vocoder's output, denoise(wav, v)
 * (vocoders/vocoder_utils.py:7-15: librosa.stft, max(|S| - v, 0) with the phase kept, librosa.istft; strength key vocoder_denoise_c,
 * egs/egs_bases/tts/base.yaml:112), and its two halves alone (_stft / _istft of utils/audio.py:35-42, Griffin-Lim's building blocks), for a
 * batch: dst = (dtts_spectral_args*), args->size = sizeof(*args).  mode = DTTS_SPECTRAL_FORWARD | DTTS_SPECTRAL_INVERSE is denoise, FORWARD
 * alone is _stft (with the edit when floor > 0), INVERSE alone is _istft of ANY spectrum, consistent or not.  The window and n_fft are those of
 * dtts_finalize_weights(DTTS_PART_ISTFT).  Per utterance b of len_b = lens_dev[b] samples (clamped to [0, wav_ld]; NULL = wav_ld):
 *   FORWARD  n_fft / 2 zeros on both sides (center=True, pad_mode='constant'), T_b = 1 + len_b / hop frames,
 *            S[t][k] = sum_n w[n] x_pad[t hop + n] e^(-2 pi i k n / n_fft), k = 0 .. n_fft / 2; then m = |S|, S' = S max(m - floor, 0) / m
 *            (0 where m = 0; floor = 0 leaves S as it is, without the division).  frames_dev[b] = T_b; rows >= T_b of spec_dev untouched.
 *   INVERSE  T_b = frames_dev[b] clamped to [0, 1 + wav_ld / hop]; y_t[n] = w[n] irfft(S'[t])[n] (the imaginary parts of bins 0 and n_fft / 2
 *            are never read), overlap-add at t hop in ascending frame order, each sample divided by the envelope sum_t w^2[n - t hop] over the
 *            frames that cover it, n_fft / 2 samples dropped at both ends: out_len_b = hop (T_b - 1) samples (0 for one frame); samples
 *            >= out_len_b of out_dev untouched; out_lens_dev[b] = out_len_b.
 *   wav_dev f32 [B][wav_ld] (FORWARD) · lens_dev i32 [B] or NULL (FORWARD) · frames_dev i32 [B] · spec_dev f32 [B][spec_cap][n_fft / 2 + 1][2],
 *   interleaved re, im (torch.view_as_real's layout), 8-byte aligned · out_dev f32 [B][wav_ld] (INVERSE) · out_lens_dev i32 [B] or NULL.
 *   With both mode bits spec_dev and frames_dev may be NULL: the spectrum and the frame counts then live in a workspace of the context
 *   (reserved on the first call, like the posterior pass's; it also holds the windowed frames [B][spec_cap][n_fft] of every INVERSE).
 * One launch (FORWARD), two (INVERSE: the frames' inverse DFT, then the overlap-add) or three on `stream`; no host synchronisation unless the
 * workspace grows; no atomics.  Both contractions are DTTS_OUT_MELSPEC's (exact fp32 products, fp32 over eight values, fp64 across those)
 * against bases computed in fp64; the overlap-add and the envelope are fp64, rounded once.  Every utterance's result is bit-identical alone
 * and inside any batch.  DTTS_E_STATE without a finalised plan; DTTS_E_INVAL (naming the value) for a wrong size, a mode outside 1 .. 3,
 * B <= 0, a hop outside 1 .. n_fft, a (window, hop) whose envelope does not stay above 1e-11 at every kept sample (torch.istft's criterion,
 * evaluated in fp64 on the host for a two-frame signal, whose envelope bounds every longer one's from below; the message names hop and the
 * smallest value; INVERSE only), spec_cap < 1 + wav_ld / hop, a floor that is negative or not finite, a NULL pointer the mode needs, or
 * an out_dev that is wav_dev or overlaps any of its B wav_ld samples (the buffers must be disjoint: nothing runs in place).
 */
#define DTTS_OUT_SPECTRAL 12
#define DTTS_SPECTRAL_FORWARD 1
#define DTTS_SPECTRAL_INVERSE 2
typedef struct dtts_spectral_args {
    int32_t size;                 /* sizeof(dtts_spectral_args) */
    int32_t mode;                 /* DTTS_SPECTRAL_FORWARD, DTTS_SPECTRAL_INVERSE or both */
    int32_t hop;                  /* any integer in 1 .. n_fft */
    int32_t B, wav_ld, spec_cap;  /* spec_cap: rows per utterance of the spectrum, >= 1 + wav_ld / hop */
    float floor;                  /* v >= 0: subtracted from every magnitude (FORWARD); the reference's default is 0.1 */
    const float* wav_dev;         /* FORWARD */
    const int32_t* lens_dev;      /* FORWARD, or NULL */
    int32_t* frames_dev;          /* written by FORWARD, read by INVERSE alone; NULL allowed with both bits */
    float* spec_dev;              /* written by FORWARD, read by INVERSE alone; NULL allowed with both bits */
    float* out_dev;               /* INVERSE */
    int32_t* out_lens_dev;        /* INVERSE, or NULL */
} dtts_spectral_args;
/*
 * DTTS_OUT_GRIFFIN_LIM: not a copy, needs NO encode — the reference's checkpoint-free way from magnitudes to a waveform, griffin_lim /
 * griffin_lim_torch (utils/audio.py:35-42, 136-158; griffin_lim_iters, egs/egs_bases/tts/base.yaml:57) with _mel_to_linear
 * (utils/audio.py:91-95) in front of it for mel input, for a batch: dst = (dtts_griffinlim_args*), args->size = sizeof(*args).  The
 * transforms are exactly DTTS_OUT_SPECTRAL's, with the window and n_fft of dtts_finalize_weights(DTTS_PART_ISTFT).  Per utterance b of
 * T_b = frames_dev[b] frames (clamped to [0, spec_cap]; NULL = spec_cap), bins = n_fft / 2 + 1:
 *   A      = |mag_dev[b][t][k]|, or from a log10-mel: max(1e-10, sum_j P[k][j] 10^mel_dev[b][t][j]) with P = "istft.inv_mel_basis"
 *            [bins][n_mels] (the pseudo-inverse of the mel filterbank, computed by the caller; loaded before the finalise; one fp32 FMA chain
 *            in ascending j per output)
 *   S      = A init (two fp32 products per bin; init_dev NULL = zero phase, S = A); y = INVERSE(S), hop (T_b - 1) samples
 *   n_iter times:  X = FORWARD(y) (T_b frames again);  S = A X / |X| (S = A where |X| = 0, as np.angle(0) = 0; bins 0 and n_fft / 2 are
 *            real and become +A or -A by the sign of X, +A for zero);  y = INVERSE(S)
 *   out_dev[b][0 .. hop (T_b - 1)) = y, samples past it untouched; out_lens_dev[b] = hop (T_b - 1); spec_out_dev (optional) receives
 *   the S that y was inverted from, rows >= T_b untouched.  No momentum (the reference has none).
 *   mag_dev f32 [B][spec_cap][bins] or mel_dev f32 [B][spec_cap][n_mels] (exactly one) · init_dev f32 [B][spec_cap][bins][2] interleaved
 *   re, im, 8-byte aligned, or NULL · frames_dev i32 [B] or NULL · out_dev f32 [B][wav_ld], wav_ld >= hop (spec_cap - 1) · out_lens_dev i32 [B]
 *   or NULL · spec_out_dev f32 [B][spec_cap][bins][2], 8-byte aligned, or NULL.
 * 1 + 2 + 3 n_iter launches on `stream` (target and start; frames' inverse DFT and overlap-add; per iteration the forward contraction with the
 * projection as its epilogue and the two of the inverse); no host synchronisation unless the workspace grows (it is DTTS_OUT_SPECTRAL's: A,
 * S, the windowed frames and the waveform between the iterations); no atomics.  Every utterance's result is bit-identical alone and inside
 * any batch; n_iter = 0 is DTTS_SPECTRAL_INVERSE of A init, bit for bit.  DTTS_E_STATE without a finalised plan, or with mel_dev and no
 * "istft.inv_mel_basis" in that plan (naming the tensor); DTTS_E_INVAL (naming the value) for a wrong size, B <= 0, spec_cap <= 0,
 * n_iter < 0, both or neither of mag_dev / mel_dev, an n_mels that is not the loaded basis's, a hop outside 1 .. n_fft or one that fails
 * DTTS_OUT_SPECTRAL's envelope criterion, wav_ld < hop (spec_cap - 1), a NULL out_dev with samples to write, or a misaligned pointer.
 */
#define DTTS_OUT_GRIFFIN_LIM 13
typedef struct dtts_griffinlim_args {
    int32_t size;                 /* sizeof(dtts_griffinlim_args) */
    int32_t B, spec_cap;          /* spec_cap: rows per utterance of every [B][spec_cap][..] tensor */
    int32_t hop;                  /* any integer in 1 .. n_fft that meets the envelope criterion */
    int32_t n_iter;               /* >= 0; the reference's griffin_lim_iters is 60 */
    int32_t wav_ld;               /* samples per row of out_dev, >= hop (spec_cap - 1) */
    int32_t n_mels;               /* with mel_dev: columns of mel_dev = columns of "istft.inv_mel_basis"; ignored with mag_dev */
    int32_t reserved;             /* 0 */
    const float* mag_dev;         /* target magnitudes, or NULL */
    const float* mel_dev;         /* log10-mel, or NULL: exactly one of the two */
    const float* init_dev;        /* the start's complex factor (e^(i phase) for Griffin-Lim proper), or NULL = 1 */
    const int32_t* frames_dev;    /* or NULL = spec_cap for all */
    float* out_dev;
    int32_t* out_lens_dev;        /* or NULL */
    float* spec_out_dev;          /* or NULL */
} dtts_griffinlim_args;
/*
 * DTTS_OUT_LOSSES: not a copy, needs NO encode — the sums behind the figures the reference's validation_step reports for the acoustic
 * model (tasks/tts/dict_tts.py:44-79,127-136): the masked mel losses l1 / mse / ssim of add_mel_loss (tasks/tts/tts_base.py:182-222,
 * modules/commons/ssim.py) and the word-duration losses of add_dur_loss in eval mode (tasks/tts/ps_flow.py:99-139), for a batch:
 * dst = (dtts_loss_args*), args->size = sizeof(*args).  Two halves, each optional: the MEL half runs iff mel_sums_dev is not NULL, the
 * DURATION half iff dur_sums_dev is not NULL (neither: DTTS_E_INVAL).  No gradients.
 *   MEL half, on the batch tensors as given: pred_dev f32 [B][pred_ld][n_mel] (mel_out), tgt_dev f32 [B][tgt_ld][n_mel] (the ground truth),
 *   T frames of each used (the leading dimensions >= T; 0 = exactly T), n_mel in 1 .. 128.  A frame's weight w is 1 iff its TARGET row is
 *   not all zero (weights_nonzero_speech: decided by the values, not by a length; a silent frame in mid-utterance has weight 0).  SSIM is
 *   the reference's: the 11 x 11 window of create_window (the float32 Gaussian of sigma 1.5, normalised in float32, its float32 outer
 *   product; built on the host), applied to the images pred + bias and tgt + bias, which are ZERO outside [0, T) x [0, n_mel) while the
 *   pad rows inside [0, T) are read as they are (after the bias they hold 6.0, not 0); C1 = 0.01^2, C2 = 0.03^2.  So an utterance's sums
 *   depend on T and on its own rows only: they are bit-identical whatever else the batch holds at the same T — and they are NOT what the
 *   utterance gives alone at a shorter T (there the window meets zeros where it meets 6.0 here).  That is the reference's definition.
 *     mel_sums_dev  f64 [B][3]: sum w |p - t|, sum w (p - t)^2, sum w (1 - ssim) over the utterance's T n_mel values;
 *     mel_count_dev i64 [B]:    sum w (weighted frames times n_mel); the reference's batch figure is sum_b sums / sum_b count;
 *     ssim_map_dev  f32 [B][T][n_mel] or NULL: the unweighted SSIM map (tests and diagnosis).
 *   The bias is added in fp64, the five window moments (x, y, x^2, y^2, xy; 121 taps each, rows then columns ascending) and the quotient
 *   are fp64: the float32 path of the reference forms E[x^2] - E[x]^2 of values near 6 against C2 = 9e-4 and loses the figure for close
 *   predictions.  One workgroup per utterance and tile of DTTS_LOSS_TILE_ROWS frames, then one launch that adds an utterance's tiles in
 *   index order; the weights multiply (a NaN in a frame of weight 0 reaches the sum, as in the reference).
 *   DURATION half: dur_pred_dev f32 [B][T_w] (ret['dur'], log domain for dur_scale 0), mel2word_dev i64 [B][m2w_ld] with T_mel columns
 *   used (m2w_ld >= T_mel; 0 = exactly T_mel), word_len_dev i32 [B], dur_scale 0 = log, 1 = linear.  Per utterance, for w = 1 .. T_w:
 *   d_w = frames with mel2word == w (mel2ph_to_dur; index 0 = padding and every value outside 0 .. T_w are IGNORED, where the reference's
 *   scatter_add fails); n_w = [w <= word_len]; dp = dur_pred n; g = log(d + 1) n (log) or d n (linear); then the second logarithm the
 *   reference applies when not training: dp2 = log(dp + 1), g2 = log(g + 1) for log scale, dp2 = dp, g2 = g for linear.
 *     dur_sums_dev f64 [B][5]: sum n |dp - g|, sum n, sum [g2 > 0] |dp2 - g2|, sum [g2 > 0], sum dp2 - sum g2 (signed; added per word as dp2 - g2), so that
 *                  wdur (eval) = sums[2] / sums[3] and sdur = mean_b |sums[4]| over a batch (add the sums first), sums[0] / sums[1] the
 *                  training-mode wdur;
 *     dur_gt_dev   i32 [B][T_w] or NULL: the counts d_w.
 *   Logarithms and sums are fp64, in a fixed order (the histogram uses integer LDS atomics, which no order can change); the logarithm of
 *   a non-positive argument follows IEEE (NaN / -inf), as the reference's does.
 * Two launches (MEL) plus one (DURATION) on `stream`; no host synchronisation unless the workspace of the tile sums grows; no atomics on
 * floating-point values: the same inputs give the same bits.  DTTS_E_INVAL (naming the value) for a wrong size, B <= 0, T <= 0, n_mel
 * outside 1 .. 128, a bias that is not finite, a leading dimension below its extent, T_w outside 1 .. DTTS_LOSS_MAX_WORDS, T_mel < 0,
 * dur_scale outside {0, 1}, a NULL input of a requested half, or a misaligned pointer.
 */
#define DTTS_OUT_LOSSES 14
#define DTTS_LOSS_TILE_ROWS 32      /* frames per tile of the MEL half.  FIXED: an utterance's tile sums are joined in tile order */
#define DTTS_LOSS_MAX_WORDS 16384   /* T_w of the DURATION half: the histogram of one utterance lives in LDS */
typedef struct dtts_loss_args {
    int32_t size;                 /* sizeof(dtts_loss_args) */
    int32_t B;
    int32_t T, n_mel;             /* MEL: frames of the batch tensor (the image height), mel bins 1 .. 128 */
    int32_t pred_ld, tgt_ld;      /* MEL: frames per utterance of pred_dev / tgt_dev, >= T; 0 = T */
    float bias;                   /* MEL: added to both images (the reference: 6.0) */
    int32_t T_w, T_mel, m2w_ld;   /* DURATION: words per utterance, columns of mel2word used, columns per row (>= T_mel; 0 = T_mel) */
    int32_t dur_scale;            /* DURATION: 0 = log, 1 = linear */
    int32_t reserved;             /* 0 */
    const float* pred_dev;        /* MEL */
    const float* tgt_dev;         /* MEL */
    double* mel_sums_dev;         /* MEL, or NULL: skip the half */
    int64_t* mel_count_dev;       /* MEL */
    float* ssim_map_dev;          /* MEL, or NULL */
    const float* dur_pred_dev;    /* DURATION */
    const int64_t* mel2word_dev;  /* DURATION */
    const int32_t* word_len_dev;  /* DURATION */
    double* dur_sums_dev;         /* DURATION, or NULL: skip the half */
    int32_t* dur_gt_dev;          /* DURATION, or NULL */
} dtts_loss_args;
/*
 * DTTS_OUT_DTW: not a copy, needs NO encode and no weights — dynamic time warping of B pairs of sequences, the reference's
 * utils/dtw.py::dtw (driven by scripts/pitch_dtw.py with the cost |x - y|) and accelerated_dtw with the cityblock cost, plus the F0
 * moments pitch_dtw.py prints: dst = (dtts_dtw_args*), args->size = sizeof(*args).  Free-running inference predicts its own durations,
 * so its mels and pitch tracks do not line up with the recordings frame for frame; this is the alignment the reference evaluates them by.
 *   Pair b: x = x_dev[b] [N][F], y = y_dev[b] [M][F] (x_ld / y_ld rows per utterance; N = x_lens_dev[b], M = y_lens_dev[b], a NULL lens
 *   pointer = the leading dimension), dtype 0 = f32, 1 = f64, F in 1 .. 128.
 *   COST.  F = 1: c(i, j) = |x_i - y_j| in the input's own precision (f32 inputs: a float32 subtract, then widened; f64: a float64
 *   subtract), which is what np.abs(x[i] - y[j]) gives for arrays of either dtype.  F > 1: the cityblock distance, each term
 *   |double(x_ik) - double(y_jk)| added in fp64 with k ascending (scipy's cdist).
 *   BAND.  window < 0: none (w = inf).  Otherwise cell (i, j) is live iff max(0, i - w) <= j <= min(M, i + w), every other cell is +inf.
 *   RECURRENCE, fp64: D[i][j] = c(i, j) + min(D[i-1][j-1], s D[i][j-1], s D[i-1][j]) with D[-1][-1] = 0 and the rest of row -1 and
 *   column -1 +inf; s = slope > 0 (the product is rounded before the min, as the reference's is; s = 1 issues no multiply).  One add of
 *   an exact minimum per cell: the result does not depend on the order in which the cells are visited, and equals the reference's in
 *   every bit.
 *   PATH.  The reference's _traceback from (N - 1, M - 1): the FIRST minimum of the UNSCALED (D[i-1][j-1], D[i-1][j], D[i][j-1]), i.e.
 *   diagonal, then i - 1, then j - 1 on ties (F0 tracks are full of exact ties: unvoiced frames are 0), until (0, 0); forward order.
 *     dist_dev     f64 [B]: D[N-1][M-1];
 *     path_dev     i32 [B][2][path_ld] or NULL: the row indices, then the column indices; path_ld >= x_ld + y_ld - 1; the entries
 *                  [path_len, path_ld) of both rows are written as -1;
 *     path_len_dev i32 [B], required with path_dev;
 *     acc_dev      f64 [B][x_ld][y_ld] or NULL: the whole accumulated-cost matrix D (tests and diagnosis); cells outside [0, N) x [0, M)
 *                  are left untouched;
 *     moments_dev  f64 [B][2][4] or NULL (F = 1 only): mean, population standard deviation, skewness m3 / m2^1.5 and Fisher kurtosis
 *                  m4 / m2^2 - 3 of x, then of y (np.std, scipy.stats.skew / kurtosis with bias=True): two passes in fp64, per lane in
 *                  index order, then a fixed tree.  Zero variance gives NaN for the last two.
 *   A BAD PAIR — a length <= 0 or above its leading dimension, or 0 <= window < |N - M| (the reference asserts) — cannot be refused on the
 *   host, the lengths live on the device: it gets dist = NaN, path_len = 0 (its path rows all -1) and NaN moments; its neighbours are
 *   unaffected.  Non-finite input values give unspecified numbers, but the traceback takes at most N + M - 2 moves, each decrementing an
 *   index that is > 0: it ends and stays inside its buffers whatever the data.
 * One wave per pair: a lane owns 16 consecutive rows, 64 lanes a strip of DTTS_DTW_STRIP_ROWS rows, and the wave sweeps the strip's
 * anti-diagonals; a second small launch follows the recorded 2-bit directions backwards; for F > 1 a launch before them fills the cost
 * workspace.  No host synchronisation unless a workspace grows; no floating-point atomics; a pair's outputs are bit-identical alone and
 * in any batch, at any leading dimension.  DTTS_E_INVAL (naming the value) for a wrong size, B <= 0, F outside 1 .. 128, a dtype outside
 * {0, 1}, a slope that is not finite and positive, a leading dimension outside 1 .. DTTS_DTW_MAX_LEN, path_ld < x_ld + y_ld - 1,
 * moments with F > 1, a NULL x_dev / y_dev / dist_dev, path_dev without path_len_dev, or a misaligned pointer.  The argument block is
 * checked before the handle, so that these refusals (reported through dtts_last_error(NULL) when h is NULL) can be exercised without a GPU.
 */
#define DTTS_OUT_DTW 15
#define DTTS_DTW_STRIP_ROWS 1024    /* rows one pass of the wave covers: 64 lanes of 16 rows */
#define DTTS_DTW_MAX_LEN 8192       /* largest x_ld / y_ld */
typedef struct dtts_dtw_args {
    int32_t size;                 /* sizeof(dtts_dtw_args) */
    int32_t B;
    int32_t F;                    /* features per row, 1 .. 128 */
    int32_t dtype;                /* 0 = f32, 1 = f64 (x_dev and y_dev) */
    int32_t x_ld, y_ld;           /* rows per utterance of x_dev / y_dev, 1 .. DTTS_DTW_MAX_LEN */
    int32_t window;               /* < 0: no band */
    int32_t path_ld;              /* entries per row of path_dev, >= x_ld + y_ld - 1 (ignored without path_dev) */
    double slope;                 /* s, finite and > 0 */
    const void* x_dev;            /* [B][x_ld][F] */
    const void* y_dev;            /* [B][y_ld][F] */
    const int32_t* x_lens_dev;    /* [B], or NULL = x_ld */
    const int32_t* y_lens_dev;    /* [B], or NULL = y_ld */
    double* dist_dev;             /* [B] */
    int32_t* path_dev;            /* [B][2][path_ld], or NULL */
    int32_t* path_len_dev;        /* [B], with path_dev */
    double* acc_dev;              /* [B][x_ld][y_ld], or NULL */
    double* moments_dev;          /* [B][2][4], or NULL */
} dtts_dtw_args;
/*
 * DTTS_OUT_PITCH: not a copy, needs NO encode and no weights — F0 tracks of B waveforms by Boersma's autocorrelation method (Praat's
 * "Sound: To Pitch (ac)" with the Hanning window), what the reference's data_gen_utils.py::get_pitch asks parselmouth for:
 * dst = (dtts_pitch_args*), args->size = sizeof(*args).  The tracks are what DTTS_OUT_DTW consumes (f64, with n_frames as the lengths).
 * All arithmetic is fp64; the float32 samples are widened on load.  Indices are 0-based; dx = 1 / sample_rate, dt = hop / sample_rate,
 * L = lens_dev[b] (NULL = wav_ld), floor = pitch_floor, ceiling = min(pitch_ceiling, sample_rate / 2).
 *   GEOMETRY.  q = (3.0 * sample_rate) / floor (one fp64 expression); nsw0 = floor(q), half = nsw0 / 2 - 1, nsw = 2 half (824 at
 *   22050 Hz, 80 Hz); nper = floor(sample_rate / floor), halfper = nper / 2 + 1; maxlag = min(nsw / 3 + 2, nsw); brent_ixmax = nsw / 2;
 *   n_lag = brent_ixmax + 1.  Frames: nF = (L - ceil(q)) div hop + 1 for L >= ceil(q), else none (= floor((L dx - 3 / floor) / dt) + 1,
 *   from integers).  Frame k is centred at the fractional sample c_k = (L - nF hop + hop - 1) / 2 + k hop; left = floor(c_k) (2 c_k is
 *   an integer), right = left + 1.
 *   FRAME.  localMean = the mean of x[max(0, right - nper) .. min(L - 1, left + nper)]; g[j] = x[right - half + j] - localMean for
 *   j = 0 .. nsw - 1; localPeak = max |g[j]| over j in [max(0, half - halfper), min(nsw, half + halfper)); intensity = localPeak >
 *   globalPeak ? 1 : localPeak / globalPeak, where globalPeak = max |x - mean(x)| over the utterance; f[j] = g[j] w[j] with
 *   w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (nsw + 1)); ac[l] = sum_j f[j] f[j + l] (j ascending, one accumulator per lag, whatever the
 *   batch); r[0] = 1, r[l] = ac[l] / (ac[0] wr[l]) with wr the window's own normalised autocorrelation (made on the host in float64).
 *   A frame with localPeak == 0 has r[l] = 0 for l >= 1 and only the unvoiced candidate.
 *   CANDIDATES (15 slots; slot 0 is the unvoiced candidate (0, 0)).  For l = 2 .. min(maxlag, brent_ixmax) - 1 ascending, a maximum is
 *   r[l] > voicing_threshold / 2 && r[l] > r[l-1] && r[l] >= r[l+1]; x0 = l + 0.5 (r[l+1] - r[l-1]) / (2 r[l] - r[l-1] - r[l+1]);
 *   first-pass frequency sample_rate / x0 and strength sinc30(x0), reflected (s > 1: 1 / s).  A free slot takes it; with none free it
 *   replaces the first slot >= 1 of the smallest s - octave_cost log2(floor / f) if its own figure is strictly larger.  Then every voiced
 *   slot is refined: x* = the maximiser of sinc70 near its integer lag l, inside [l - 1, l + 1] (where the interpolant's analytic
 *   derivative changes sign from + to -: a zero between two integer lags, or a kink on one, since the term set changes there; bracketed
 *   around the parabolic vertex and closed in on by a regula falsi to 1e-12 samples); frequency =
 *   sample_rate / x*, strength = sinc70(x*), reflected.  sincD(x) is Praat's NUM_interpolate_sinc of depth D on r taken symmetrically
 *   over -brent_ixmax .. brent_ixmax, D clipped to the samples on either side (never at brent_ixmax - maxlag >= 70).
 *   PATH.  corr = 0.01 / dt; a slot is voiced iff 0 < f < ceiling.  Local score: voicing_threshold + max(0, 2 - intensity (1 +
 *   voicing_threshold) / silence_threshold) for an unvoiced slot, strength - octave_cost log2(ceiling / f) for a voiced one.
 *   Transition cost: 0 between unvoiced slots, voiced_unvoiced_cost corr between a voiced and an unvoiced one, octave_jump_cost corr
 *   |log2(f1 / f2)| between voiced ones (the kernel takes one log2 per slot and uses differences: log2(ceiling) - log2 f, |log2 f1 -
 *   log2 f2|).  delta[k][c2] = max_c1 (delta[k-1][c1] - cost) + local[k][c2]; the first maximum in slot order
 *   wins every tie, the last frame's first maximum starts the backtrack.
 *     f0_dev        f64 [B][frames_ld]: the chosen slot's frequency, 0 where it is unvoiced by the rule above; 0 behind n_frames;
 *     n_frames_dev  i32 [B];
 *     acf_dev       f64 [B][frames_ld][n_lag] or NULL: r[0 .. brent_ixmax];
 *     cand_dev      f64 [B][frames_ld][15][2] or NULL: frequency and strength per slot (the raw frequency, over-ceiling ones
 *                   included), unused slots (0, 0);
 *     n_cand_dev    i32 [B][frames_ld] or NULL;
 *     intensity_dev f64 [B][frames_ld] or NULL;
 *     selected_dev  i32 [B][frames_ld] or NULL: the slot the path chose, -1 behind n_frames.
 *   frames_ld >= the frame count of a wav_ld-sample utterance.  Behind n_frames[b] the optional float outputs and n_cand are left
 *   untouched.  An utterance whose length is outside 1 .. wav_ld, or too short for one frame (Praat raises there), cannot be refused on
 *   the host: it gets n_frames = 0 and a zero row.  Non-finite samples give unspecified numbers; nothing is read behind an utterance's
 *   own length.
 * Four launches (utterance statistics; the autocorrelation, one workgroup per frame with the frame in LDS; the candidates, one wave per
 * frame; the path, one wave per utterance), no atomics, no host synchronisation unless the workspace grows or a new window length
 * uploads its tables; an utterance's outputs are bit-identical alone and in any batch, at any leading dimension.
 * SUPPORTED: sample_rate 8000 .. 48000, hop 1 .. 4096, pitch_floor >= 10 with nsw in 32 .. DTTS_PITCH_MAX_WINDOW (floor above 32.3 Hz at
 * 22050 Hz, above 70.3 Hz at 48000 Hz), pitch_ceiling > pitch_floor, voicing_threshold and silence_threshold > 0, the three costs >= 0, all
 * finite; wav_ld 1 .. 2^26, frames_ld <= DTTS_PITCH_MAX_FRAMES.  DTTS_E_INVAL (naming the field) for anything else, a wrong size, B <= 0,
 * a NULL wav_dev / f0_dev / n_frames_dev, or a misaligned pointer.  The argument block is checked before the handle, as DTTS_OUT_DTW's is.
 */
#define DTTS_OUT_PITCH 16
#define DTTS_PITCH_CANDIDATES 15     /* Praat's default; fixed */
#define DTTS_PITCH_MAX_WINDOW 2048   /* largest nsw (samples of one analysis window) */
#define DTTS_PITCH_MAX_FRAMES 8192   /* largest frames_ld (= DTTS_DTW_MAX_LEN, the consumer's limit) */
typedef struct dtts_pitch_args {
    int32_t size;                 /* sizeof(dtts_pitch_args) */
    int32_t B;
    int32_t wav_ld;               /* samples per row of wav_dev */
    int32_t frames_ld;            /* frames per row of the outputs */
    int32_t sample_rate, hop;     /* the time step is hop / sample_rate s */
    double pitch_floor, pitch_ceiling;                          /* Hz (the reference: 80, 750) */
    double voicing_threshold, silence_threshold;                /* (0.6; Praat's 0.03) */
    double octave_cost, octave_jump_cost, voiced_unvoiced_cost; /* (Praat's 0.01, 0.35, 0.14) */
    const float* wav_dev;         /* [B][wav_ld] */
    const int32_t* lens_dev;      /* [B], or NULL = wav_ld */
    double* f0_dev;               /* [B][frames_ld] */
    int32_t* n_frames_dev;        /* [B] */
    double* acf_dev;              /* [B][frames_ld][n_lag], or NULL */
    double* cand_dev;             /* [B][frames_ld][15][2], or NULL */
    int32_t* n_cand_dev;          /* [B][frames_ld], or NULL */
    double* intensity_dev;        /* [B][frames_ld], or NULL */
    int32_t* selected_dev;        /* [B][frames_ld], or NULL */
} dtts_pitch_args;
/*
 * DTTS_OUT_RESAMPLE: not a copy, needs NO encode — band-limited resampling of B waveforms from sr_in to sr_out, librosa 0.9.2's
 * resample(res_type = 'kaiser_best') = resampy 0.4.2's resample_f, with the filter of dtts_finalize_weights(DTTS_PART_RESAMPLE):
 * dst = (dtts_resample_args*), args->size = sizeof(*args).  All arithmetic is fp64 on the float32 samples; win / delta are the plan's
 * tables of n_win entries, num_table its precision, L = lens_dev[b] (NULL = wav_ld).
 *   ratio = (double)sr_out / sr_in; n_out = (int)(L ratio); scale = min(1, ratio); inc = 1 / ratio; index_step = (int)(scale num_table)
 *   (TRUNCATED, as resampy does: 235 for 48000 -> 22050, where scale num_table = 235.2).  For ratio < 1 every table entry is used
 *   times ratio: win_s[i] = win[i] ratio, delta_s[i] = delta[i] ratio (one multiplication each; ratio >= 1: the entries themselves).
 *   Output t = 0 .. n_out - 1:  tr = t inc; n = (int)tr; frac = scale (tr - n).
 *     LEFT WING   f = frac num_table; off = (int)f; eta = f - off; for i = 0 .. min(n + 1, (n_win - off) / index_step) - 1 ascending:
 *                 w = win_s[off + i index_step] + eta delta_s[off + i index_step]; acc += w x[n - i];
 *     RIGHT WING  frac' = scale - frac; f, off, eta from frac' in the same way; for k = 0 .. min(L - n - 1, (n_win - off) / index_step) - 1
 *                 ascending: w likewise; acc += w x[n + k + 1].
 *   One fp64 accumulator per output, starting at 0, the left wing first, whatever the batch or the leading dimensions.  tr, frac, f, eta
 *   and w are separate IEEE multiplications, subtractions and additions (never contracted: n and off are truncations of them); the tap
 *   product acc += w x is one fma.  out[t] = (float)acc: ONE rounding, where the reference rounds its float32 y[t] after every tap
 *   (the deliberate deviation).  out_lens[b] = ceil(L ratio), librosa's fix_length: the sample at index n_out is 0 when ceil > int, and
 *   so is everything behind out_lens[b] in the row.
 *     out_dev       f32 [B][out_ld];
 *     out_lens_dev  i32 [B];
 *     out64_dev     f64 [B][out_ld] or NULL: acc before its rounding (0 behind n_out).
 *   An utterance whose length is outside 1 .. wav_ld, or whose out_lens would exceed out_ld, gets out_lens = 0 and a zero row.  Nothing
 *   is read behind an utterance's own length.
 * One launch: a workgroup owns DTTS_RESAMPLE_TILE consecutive outputs of one utterance (a lane one output) and stages the input span
 * they read in LDS as fp64; the tables are read through L2.  No atomics, no workspace, no host synchronisation; an utterance's outputs
 * are bit-identical alone and in any batch, at any leading dimension.
 * SUPPORTED: sr_in, sr_out 8000 .. 48000, sr_in != sr_out, index_step >= 1, (n_win - 1) / index_step <= 2048 taps per wing,
 * wav_ld 1 .. 2^26, out_ld >= 1.  DTTS_E_INVAL (naming the field) for anything else, a wrong size, B outside 1 .. 65535, a NULL wav_dev /
 * out_dev / out_lens_dev or a misaligned pointer; the argument block is checked before the handle, as DTTS_OUT_DTW's is.  DTTS_E_NOENT
 * without a finalised filter.
 */
#define DTTS_OUT_RESAMPLE 17
#define DTTS_RESAMPLE_TILE 256 /* consecutive outputs of one workgroup (the shape cases of tests/wavprep_shapes.py derive from it) */
typedef struct dtts_resample_args {
    int32_t size;                 /* sizeof(dtts_resample_args) */
    int32_t B;
    int32_t wav_ld;               /* samples per row of wav_dev */
    int32_t out_ld;               /* samples per row of out_dev / out64_dev */
    int32_t sr_in, sr_out;
    const float* wav_dev;         /* [B][wav_ld] */
    const int32_t* lens_dev;      /* [B], or NULL = wav_ld */
    float* out_dev;               /* [B][out_ld] */
    int32_t* out_lens_dev;        /* [B] */
    double* out64_dev;            /* [B][out_ld], or NULL */
} dtts_resample_args;
/*
 * DTTS_OUT_LOUDNESS: not a copy, needs NO encode and no weights — ITU-R BS.1770 integrated loudness of B mono waveforms and, with
 * mode = 1, their normalisation to target_lufs: pyloudnorm 0.1.1's Meter.integrated_loudness and normalize.loudness, then the reference's
 * peak rule (data_gen_utils.py::process_utterance: loud_norm to -22 LUFS; `if abs(wav).max() > 1: wav = wav / abs(wav).max()`):
 * dst = (dtts_loudness_args*), args->size = sizeof(*args).  All of it is fp64 on the float32 samples, without contraction; rate =
 * sample_rate, L = lens_dev[b] (NULL = wav_ld; a length outside 0 .. wav_ld counts as 0).
 *   K-WEIGHTING.  Two biquads whose coefficients are made on the host in fp64, the high shelf first:
 *     w0 = 2 pi (fc / rate), alpha = sin w0 / (2 Q), c = cos w0;
 *     high shelf (G = 4.0 dB, Q = 1 / sqrt 2, fc = 1500 Hz), A = 10^(G / 40), r = sqrt A:
 *       b = A ((A + 1) + (A - 1) c + 2 r alpha), -2 A ((A - 1) + (A + 1) c), A ((A + 1) + (A - 1) c - 2 r alpha)
 *       a = (A + 1) - (A - 1) c + 2 r alpha, 2 ((A - 1) - (A + 1) c), (A + 1) - (A - 1) c - 2 r alpha;
 *     high pass (Q = 0.5, fc = 38 Hz): b = (1 + c) / 2, -(1 + c), (1 + c) / 2;  a = 1 + alpha, -2 c, 1 - alpha;
 *     both divided by their a0 (passband gain 1).  Each runs in the transposed direct form II from a zero state, as scipy's lfilter does:
 *     y = z1 + b0 x; z1 = (z2 + b1 x) - a1 y; z2 = b2 x - a2 y.
 *   BLOCKS.  T = L / rate; n_blocks = (int)(rint((T - 0.4) / (0.4 0.25)) + 1), round half even.  Block j covers [lo_j, min(hi_j, L)),
 *   lo_j = (int)(0.4 (j 0.25) rate), hi_j = (int)(0.4 (j 0.25 + 1) rate) (a host-made table); z_j = (sum of y^2 over it) / (0.4 rate):
 *   the divisor is the full block even where the end of the utterance cuts the last one.
 *   GATING.  l_j = -0.691 + 10 log10 z_j; absolute gate l_j >= -70; Gamma_r = -0.691 + 10 log10(mean of the gated z_j) - 10; the final
 *   set is l_j > Gamma_r && l_j > -70; LUFS = -0.691 + 10 log10(mean of z_j over the final set).  Both means run over ascending j with
 *   one accumulator.
 *   STATUS.  bit 0 (DTTS_LOUD_TOO_SHORT): L < 0.4 rate, where pyloudnorm raises: lufs = NaN, gain = 1, n_blocks = 0, the row is copied
 *   unchanged.  bit 1 (DTTS_LOUD_SILENT): no block passes the gates, where pyloudnorm returns -inf and its normalisation NaNs:
 *   lufs = -inf, gain = 1, copied unchanged.  bit 2 (DTTS_LOUD_PEAK): the peak rule fired.
 *   NORMALISE (mode 1).  gain = 10^((target_lufs - LUFS) / 20) in fp64; y = (float)gain x as ONE float32 multiplication (what numpy
 *   1.23.5's value-based casting makes of float64 scalar * float32 array); p = max |y| over the utterance = (float)gain max |x| (the
 *   product is monotone: no second pass); if p > 1: y = y / p, an IEEE float32 division.  Samples behind L are 0.
 *     lufs_dev f64 [B]; gain_dev f64 [B]; status_dev i32 [B]; out_dev f32 [B][wav_ld] (mode 1; may be wav_dev itself);
 *     z_dev f64 [B][blocks_ld] or NULL: the z_j (behind n_blocks untouched); n_blocks_dev i32 [B] or NULL.
 * The cascade is a linear recurrence on four state values, s' = M s + g x.  Every utterance is cut into segments of DTTS_LOUD_SEGMENT
 * samples anchored at its sample 0 (the cut never depends on the batch).  Launches: (1) a lane per segment runs it from a zero state and
 * leaves its end state e_k and max |x|; (2) a wave per utterance chains the true start states in segment order, s_{k+1} = M^S s_k + e_k
 * (M^S made on the host in fp64 by squaring M eight times), and joins the maxima; (3) a lane per segment runs it again from its true start state and
 * leaves, for each of the at most six blocks it meets, the sum of y^2 over their common samples in ascending order; (4) a lane per block
 * adds those partial sums in ascending segment order and divides, then a lane per utterance does the gating; (5, mode 1) an elementwise
 * launch applies the gain.  No atomics; no host synchronisation unless the workspace grows or a longer block table is uploaded; an
 * utterance's outputs are bit-identical alone and in any batch, at any leading dimension.
 * SUPPORTED: sample_rate 8000 .. 48000, wav_ld 1 .. 2^26, mode 0 / 1, a finite target_lufs, blocks_ld >= max(1, the block count of a
 * wav_ld-sample utterance).  DTTS_E_INVAL (naming the field) for anything else, a wrong size, B outside 1 .. 65535, a NULL wav_dev /
 * lufs_dev / gain_dev / status_dev, a NULL out_dev in mode 1 or a misaligned pointer; the argument block is checked before the handle.
 */
#define DTTS_OUT_LOUDNESS 18
#define DTTS_LOUD_SEGMENT 256 /* samples of one segment of the recurrence (the shape cases of tests/wavprep_shapes.py derive from it) */
#define DTTS_LOUD_TOO_SHORT 1
#define DTTS_LOUD_SILENT 2
#define DTTS_LOUD_PEAK 4
typedef struct dtts_loudness_args {
    int32_t size;                 /* sizeof(dtts_loudness_args) */
    int32_t B;
    int32_t wav_ld;               /* samples per row of wav_dev and out_dev */
    int32_t blocks_ld;            /* entries per row of z_dev */
    int32_t sample_rate;
    int32_t mode;                 /* 0 = measure only, 1 = measure and normalise */
    double target_lufs;           /* (the reference: -22; trim_long_silences: -20) */
    const float* wav_dev;         /* [B][wav_ld] */
    const int32_t* lens_dev;      /* [B], or NULL = wav_ld */
    double* lufs_dev;             /* [B] */
    double* gain_dev;             /* [B] */
    int32_t* status_dev;          /* [B] */
    float* out_dev;               /* [B][wav_ld] (mode 1), or NULL */
    double* z_dev;                /* [B][blocks_ld], or NULL */
    int32_t* n_blocks_dev;        /* [B], or NULL */
} dtts_loudness_args;
/*
 * DTTS_OUT_DISC: not a copy, needs NO encode — the sums behind what tasks/vocoder/hifigan.py logs for a vocoder (a_p / a_s, r_p / f_p /
 * r_s / f_s, fm_f / fm_s; modules/hifigan/hifigan.py: generator_loss, discriminator_loss, feature_loss) for B waveform pairs, with the
 * discriminators of dtts_finalize_weights(DTTS_PART_DISC): dst = (dtts_disc_args*), args->size = sizeof(*args).  y is the recording, y_hat
 * the generated waveform; pair b has L = lens_dev[b] samples of both (NULL = wav_ld).  Every utterance is scored AS IF ALONE AT ITS OWN
 * LENGTH: nothing of a neighbour, of the padding behind L or of the batch enters, and its sums are bit-identical alone and in any batch.
 *   Discriminator d = 0 .. 4: MultiPeriodDiscriminator.discriminators[d] (periods 2, 3, 5, 7, 11): the waveform reflect padded on the right
 *   to a multiple of p (index L + k reads sample L - 2 - k), folded to [rows][p]; per column Conv(1 -> 32 -> 128 -> 512 -> 1024, k = 5,
 *   stride 3, pad 2), Conv(1024 -> 1024, k = 5, pad 2), each followed by leaky_relu(0.1), then conv_post (1024 -> 1, k = 3, pad 1).
 *   d = 5 .. 7: MultiScaleDiscriminator.discriminators[d - 5] on the waveform pooled d - 5 times by AvgPool1d(4, 2, padding = 1) (the edges
 *   divide by 4 too): Conv1d 1 -> 128 (k = 15), 128 -> 128 (k = 41, s 2, g 4), 128 -> 256 (k = 41, s 2, g 16), 256 -> 512 (k = 41, s 4,
 *   g 16), 512 -> 1024 (k = 41, s 4, g 16), 1024 -> 1024 (k = 41, g 16), 1024 -> 1024 (k = 5), leaky_relu(0.1) after each, conv_post
 *   (1024 -> 1, k = 3).  All of it in fp32 with exact fp32 products; D is the flattened conv_post output.
 *     sums_dev f64 [B][8][4]: sum (1 - D(y))^2, sum D(y)^2, sum (1 - D(y_hat))^2, sum D(y_hat)^2 over the n outputs of discriminator d;
 *     counts_dev i64 [B][8]: n.  fm_dev f64 [B][8][8] / fm_counts_dev i64 [B][8][8] (DTTS_DISC_FM): per feature map l (the activated
 *     output of convolution l, conv_post's output last; 6 maps for d < 5, 8 for d >= 5, the rest untouched) sum |fmap(y) - fmap(y_hat)|
 *     and its element count.  d_dev f32 [8][2][B][d_ld] or NULL: the D outputs themselves (y, then y_hat), in the reference's flattened
 *     order.  status_dev i32 [B]: DTTS_DISC_TOO_SHORT where L is outside DTTS_DISC_MIN_LEN .. wav_ld (the reference's reflect padding
 *     raises below 6 samples): that pair's counts are 0 and its sums 0.  Rows of discriminators `which` leaves out stay untouched.
 * The host forms mean (1 - D)^2 = sums / counts per discriminator and averages over the discriminators (a_*, r_*, f_*), and
 * fm = 2 * sum over d and l of fm / fm_counts; pooled figures divide the sums over the batch by the counts over the batch, which equals the
 * reference's batch means when all lengths are equal.  All fp64 sums run in a fixed order without atomics.  The discriminators run one after
 * another on `stream` over one reused workspace, the batch in chunks of utterances that keep it below DTTS_DISC_WS_BYTES (a single
 * utterance may exceed it); no host synchronisation unless the workspace grows.
 * DTTS_E_INVAL (naming the field): a wrong size, B outside 1 .. 65535, wav_ld outside DTTS_DISC_MIN_LEN .. 2^24, `which` without
 * DTTS_DISC_MPD or DTTS_DISC_MSD or with unknown bits, DTTS_DISC_FM without fm_dev / fm_counts_dev, d_dev with d_ld below
 * (wav_ld + 63) / 64 + 16 entries (abi.disc_d_ld), a NULL y_dev / y_hat_dev / sums_dev / counts_dev / status_dev, a misaligned pointer; the
 * argument block is checked before the handle, as DTTS_OUT_DTW's is.  DTTS_E_STATE before dtts_finalize_weights(DTTS_PART_DISC).
 */
#define DTTS_OUT_DISC 19
#define DTTS_DISC_MPD 1
#define DTTS_DISC_MSD 2
#define DTTS_DISC_FM 4
#define DTTS_DISC_DENSE_GROUPED 8 /* measurement aid (tools/disc_bench.py): the scale discriminators' grouped layers run as block-diagonal DENSE layers
                                   * on the dense kernels (16 x / 4 x the work), the form the library had before its grouped kernel; same results up
                                   * to summation order.  The first such call packs those layers on the host and synchronises. */
#define DTTS_DISC_N 8            /* discriminators: 5 periods, then 3 scales */
#define DTTS_DISC_MAX_FMAPS 8    /* feature maps of a scale discriminator (a period discriminator has 6) */
#define DTTS_DISC_MIN_LEN 6      /* shortest waveform the reference's MultiPeriodDiscriminator accepts (period 11 pads 5 samples by reflection) */
#define DTTS_DISC_TOO_SHORT 1
#define DTTS_DISC_DENSE_TILE 32  /* output rows per tile of the dense layers; DTTS_DISC_GROUP_TILE: of the grouped kernel's narrow / wide form */
#define DTTS_DISC_GROUP_TILE 128
#define DTTS_DISC_GROUP_TILE_WIDE 64
#define DTTS_DISC_WS_BYTES (3ll << 30)
typedef struct dtts_disc_args {
    int32_t size;                 /* sizeof(dtts_disc_args) */
    int32_t B;
    int32_t wav_ld;               /* samples per row of y_dev / y_hat_dev */
    int32_t which;                /* DTTS_DISC_MPD | DTTS_DISC_MSD | DTTS_DISC_FM */
    int32_t d_ld;                 /* entries per row of d_dev */
    int32_t reserved;             /* 0 */
    const float* y_dev;           /* [B][wav_ld] */
    const float* y_hat_dev;       /* [B][wav_ld] */
    const int32_t* lens_dev;      /* [B], or NULL = wav_ld */
    double* sums_dev;             /* [B][8][4] */
    int64_t* counts_dev;          /* [B][8] */
    double* fm_dev;               /* [B][8][8], or NULL */
    int64_t* fm_counts_dev;       /* [B][8][8], or NULL */
    float* d_dev;                 /* [8][2][B][d_ld], or NULL */
    int32_t* status_dev;          /* [B] */
} dtts_disc_args;
/*
 * DTTS_OUT_SPKENC: not a copy, needs NO encode — utterance embeddings (d-vectors) of B recordings with the encoder of
 * dtts_finalize_weights(DTTS_PART_SPKENC): dst = (dtts_spkenc_args*), args->size = sizeof(*args).  What Resemblyzer 0.1.1's
 * VoiceEncoder.embed_utterance computes, restated:
 *   mode DTTS_SPKENC_FROM_WAV: utterance b is L = lens_dev[b] samples (NULL = wav_ld; clamped to 0 .. wav_ld) of wav_dev[b], taken AS 16 kHz.
 *     Partials (compute_partial_slices): n_frames = L / 160 + 1, steps = max(1, n_frames - 160 + frame_step + 1), one partial of 160
 *     frames = 25600 samples at frame i for i = 0, frame_step, 2 frame_step, ... < steps; the last one is dropped iff there is more than one
 *     and (L - 160 i) / 25600 < min_coverage (fp64).  frame_step = round(16000 / rate / 160) is the caller's (77 at rate 1.3).  The
 *     waveform is zero padded to the last partial's end, L' = max(L, 160 (i_last + 160)).
 *     Mel (librosa.feature.melspectrogram(sr 16000, n_fft 400, hop 160, n_mels 40), POWER, no logarithm): 1 + L' / 160 centred frames;
 *     frame f covers samples 160 f - 200 .. 160 f + 199 of the padded waveform, outside 0 .. L' - 1 zero (DTTS_SPKENC_PAD_CONSTANT) or
 *     mirrored without repeating the edge (DTTS_SPKENC_PAD_REFLECT).  X[k] = sum_n (w[n] e^(-2 pi i k n / 400)) x[n] over a basis rounded
 *     once from fp64, per component 16 fp32 fma chains of 25 consecutive n, added four by four in order and the four sums in order;
 *     P[k] = re^2 + im^2; mel[m] = sum_k basis[m][k] P[k], one chain in k order.
 *   mode DTTS_SPKENC_FROM_MELS: wav_dev holds B sequences of mels [B][wav_ld][40] (wav_ld = frames per sequence, 1 .. DTTS_SPKENC_MAX_T),
 *     each its own utterance of one partial; lens_dev and mel_dev must be NULL, frame_step / min_coverage / pad_mode are not used.
 *   Per partial (VoiceEncoder.forward): three LSTM layers of 256 units from zero state — gates = (W_hh h_{t-1}, one fp32 chain over k) +
 *     (W_ih x_t + (b_ih + b_hh)), i, f, o = sigmoid from exp(-|x|), g = tanh from expm1(-2 |x|) with the sign restored (finite at saturation), c_t = f c + i g,
 *     h_t = o tanh(c_t) — then relu(linear(h_T of layer 2)) divided by its L2 norm.  Per utterance: the mean over its partials (an fp64 sum
 *     in partial order, rounded to fp32 once) divided by its L2 norm.  A ZERO vector divides to NaN, exactly as the reference's does (all
 *     256 relu outputs dead): the NaN is the result, it is not hidden.
 * Outputs: embed_dev f32 [B][256]; n_partials_dev i32 [B]; optionally, with P = dtts_spkenc_max_partials and F = dtts_spkenc_frames_ld
 * of (wav_ld, frame_step) (FROM_MELS: P = 1), partials_dev f32 [B][P][256] (the unit embeddings of the partials), mel_dev f32 [B][F][40]
 * and hseq_dev[l] f32 [B][P][T][256] (T = 160, FROM_MELS: wav_ld), every layer's hidden sequence; rows behind an utterance's partials or
 * frames stay untouched.  Nothing is read behind lens_dev[b].  Every sequence's arithmetic is independent of the others: an utterance's
 * embedding is bit-identical alone and in any batch, at tile_m = 16 and 32 (the sequences of one workgroup of the recurrent kernel;
 * 0 = 16 while a chunk's sequences fit 16 per compute unit, DTTS_SPKENC_TILE_M beyond).  No atomics; a workgroup never waits on another.  The batch runs in chunks of utterances that keep the one
 * workspace below DTTS_SPKENC_WS_BYTES (a single utterance may exceed it); no host synchronisation unless the workspace grows.
 * DTTS_E_INVAL (naming the field): a wrong size, mode, B outside 1 .. 65535, wav_ld outside 1 .. 2^24 (FROM_MELS: 1 .. DTTS_SPKENC_MAX_T),
 * frame_step outside 1 .. 4096, min_coverage outside (0, 1], pad_mode, tile_m, reserved != 0, a NULL wav_dev / embed_dev / n_partials_dev, a misaligned
 * pointer; the argument block is checked before the handle, as DTTS_OUT_DTW's is.  DTTS_E_STATE before
 * dtts_finalize_weights(DTTS_PART_SPKENC).
 */
#define DTTS_OUT_SPKENC 20
#define DTTS_SPKENC_FROM_WAV 0
#define DTTS_SPKENC_FROM_MELS 1
#define DTTS_SPKENC_PAD_CONSTANT 0
#define DTTS_SPKENC_PAD_REFLECT 1
#define DTTS_SPKENC_TILE_M 32       /* the most sequences per workgroup of the recurrent kernel: the rows of its MFMA tile */
#define DTTS_SPKENC_MAX_T 4096
#define DTTS_SPKENC_WS_BYTES (1ll << 30)
typedef struct dtts_spkenc_args {
    int32_t size;                 /* sizeof(dtts_spkenc_args) */
    int32_t B;
    int32_t wav_ld;               /* samples per row of wav_dev (FROM_MELS: frames per sequence) */
    int32_t mode;                 /* DTTS_SPKENC_FROM_WAV / DTTS_SPKENC_FROM_MELS */
    int32_t frame_step;           /* frames between partials */
    int32_t pad_mode;             /* DTTS_SPKENC_PAD_CONSTANT / DTTS_SPKENC_PAD_REFLECT */
    int32_t tile_m;               /* 0, 16 or 32 */
    int32_t reserved;             /* 0 */
    double min_coverage;
    const float* wav_dev;         /* [B][wav_ld] (FROM_MELS: [B][wav_ld][40]) */
    const int32_t* lens_dev;      /* [B], or NULL = wav_ld */
    float* embed_dev;             /* [B][256] */
    int32_t* n_partials_dev;      /* [B] */
    float* partials_dev;          /* [B][P][256], or NULL */
    float* mel_dev;               /* [B][F][40], or NULL */
    float* hseq_dev[3];           /* [B][P][T][256] each, or NULL */
} dtts_spkenc_args;
/*
 * DTTS_OUT_MELDISC: not a copy, needs NO encode — the multi-window mel discriminator of dtts_finalize_weights(DTTS_PART_MELDISC) in eval
 * mode (Dropout2d is the identity) on clips of n_sig mels, and the sums behind the a / r / f terms of tasks/tts/dict_tts.py::_training_step:
 * dst = (dtts_meldisc_args*), args->size = sizeof(*args).  Signal s has L = lens_dev[s] frames (NULL = T_ld) of mel_dev[s]; frames at or
 * behind L enter as ZEROS whatever the buffer holds there.  Window w (32 << w frames) has clips_ld clip slots per signal: slot j starts at
 * starts_dev[w][s][j] (a negative entry = no clip) or, with starts_dev NULL, at j * hop[w].  A slot is a clip when start >= 0 and
 * start + win <= L (DTTS_MELDISC_WITHIN_LEN: the measurement) or start + win <= T_ld (without the flag: the reference's forward, whose
 * clips may run behind an utterance's own length).  Per clip, with H = mel_disc_hidden_size:
 *   block 1: Conv2d(1 -> H, 3 x 3, stride 2, pad 1) on the clip [win][80], LeakyReLU(0.2);  blocks 2, 3: Conv2d(H -> H, the same),
 *   LeakyReLU(0.2), then the norm (none / InstanceNorm2d, eps 1e-5, biased variance per (clip, channel) in fp64 by two passes / the folded
 *   BatchNorm affine); maps (win / 2, 40), (win / 4, 20), (win / 8, 10); the zero padding of a block is padding of the NORMALISED map.
 *   Blocks 2 and 3 contract over (channel chunk, tap, channel) on v_mfma_f32_32x32x2_f32 with exact fp32 products.  Head: stack / sum one
 *   D = adv . flatten(c, t, f) + bias per clip; none one D per remaining time row (win / 8 of them) over (c, f).
 * Outputs: sums_dev f64 [n_sig][3][2]: sum (1 - D)^2 and sum D^2 over the D of signal s's clips of window w; counts_dev i64 [n_sig][3] their
 * number (0: no clip fits, sums 0; windows >= n_win untouched); status_dev i32 [n_sig]: DTTS_MELDISC_BAD_LEN where L is outside 0 .. T_ld
 * (treated as 0 frames); d_dev f32 [n_win][n_sig][clips_ld][DTTS_MELDISC_D_LD] or NULL: the D of every clip (entry 0, or win / 8 entries
 * for none; other entries and slots without a clip untouched); h_dev[3 w + l] f32 [n_sig][clips_ld][t][f][H] or NULL: the output of block l
 * of window w as the reference's `h` holds it (after the norm), channels-last, for tests.  All sums run in fp64 in a fixed order without
 * atomics; a signal's results are bit-identical alone and in any batch.  The windows run one after another on `stream` over one reused
 * workspace, the signals in chunks that keep it below DTTS_MELDISC_WS_BYTES (one signal may exceed it); no host synchronisation unless the
 * workspace grows.  `reduction` does not change D: the host adds (sum) or stacks the windows; it must agree with the loaded adv_layer
 * (none <-> per-row heads).
 * DTTS_E_INVAL (naming the field): a wrong size, n_sig outside 1 .. 65535, T_ld outside 1 .. 2^20, n_win outside 1 .. 3, an unknown
 * reduction or flag, clips_ld outside 1 .. 65536 or n_sig * clips_ld above 2^24, starts_dev NULL with a hop[w] < 1 (w < n_win), a non-zero
 * reserved word, a NULL mel_dev / sums_dev / counts_dev / status_dev, a misaligned pointer; the block is checked before the handle.
 * DTTS_E_STATE before dtts_finalize_weights(DTTS_PART_MELDISC); DTTS_E_INVAL when n_win or the reduction's kind differs from the loaded model.
 */
#define DTTS_OUT_MELDISC 21
#define DTTS_MELDISC_STACK 0
#define DTTS_MELDISC_SUM 1
#define DTTS_MELDISC_NONE 2
#define DTTS_MELDISC_WITHIN_LEN 1   /* flags */
#define DTTS_MELDISC_BAD_LEN 1      /* status bit */
#define DTTS_MELDISC_MELS 80        /* freq_length: the only audio_num_mel_bins the reference's discriminator is built for */
#define DTTS_MELDISC_MAX_WIN 3      /* windows of 32, 64, 128 frames */
#define DTTS_MELDISC_D_LD 16        /* D entries per clip slot (128 / 8 time rows under disc_reduction: none) */
#define DTTS_MELDISC_MAX_HIDDEN 256
#define DTTS_MELDISC_WS_BYTES (1ll << 30)
typedef struct dtts_meldisc_args {
    int32_t size;                 /* sizeof(dtts_meldisc_args) */
    int32_t n_sig;
    int32_t T_ld;                 /* frames per row of mel_dev */
    int32_t n_win;                /* windows (disc_win_num) */
    int32_t reduction;            /* DTTS_MELDISC_STACK / SUM / NONE */
    int32_t flags;                /* DTTS_MELDISC_WITHIN_LEN */
    int32_t clips_ld;             /* clip slots per (window, signal) */
    int32_t hop[3];               /* frames between the starts of window w (starts_dev NULL) */
    int32_t reserved[2];          /* 0 */
    const float* mel_dev;         /* [n_sig][T_ld][80] */
    const int32_t* lens_dev;      /* [n_sig], or NULL = T_ld */
    const int32_t* starts_dev;    /* [n_win][n_sig][clips_ld], or NULL = j * hop[w] */
    float* d_dev;                 /* [n_win][n_sig][clips_ld][DTTS_MELDISC_D_LD], or NULL */
    double* sums_dev;             /* [n_sig][3][2] */
    int64_t* counts_dev;          /* [n_sig][3] */
    int32_t* status_dev;          /* [n_sig] */
    float* h_dev[9];              /* [3 w + l]: [n_sig][clips_ld][t][f][H], or NULL */
} dtts_meldisc_args;
DTTS_API int dtts_text2mel_fetch(dtts_handle h, int what, void* dst_dev, dtts_stream stream);

/*
 * Length regulator alone — replaces the integer part of add_dur + LengthRegulator.forward
 * (modules/dict_tts/model.py:78-81, modules/fastspeech/tts_modules.py:215-251): dur [B,T_w] f32 (log domain),
 * ilens [B] i32 valid words; d = clamp(round_half_even(exp(dur) - 1), 0), an utterance whose durations are all zero
 * gets ones.  Writes mel2word [B,cap] i64 (1-based word index, 0 = padding; columns beyond the longest utterance
 * are zero) and, on the host, the per-batch maximum frame count (unpadded).  Returns DTTS_E_INVAL if it exceeds cap.
 */
DTTS_API int dtts_length_regulate(dtts_handle h, const float* dur_dev, const int32_t* ilens_dev, int B, int T_w, int64_t* mel2word_dev,
                         int cap, int32_t* T_max_host, dtts_stream stream);

/*
 * Vocoder — replaces HifiGanGenerator.forward as used by HifiGAN.spec2wav (vocoders/hifigan.py:54-62), for a
 * batch: mel [B,T,80] f32 (the layout of ret['mel_out'] and of spec2wav's argument), lens [B] i32 valid
 * frames per utterance (NULL = T for all).  wav [B, T*hop] f32; utterance b is exactly what the reference
 * produces for mel[b,:lens[b]] alone, samples past lens[b]*hop are zero.  B <= DTTS_MAX_VOCODER_BATCH per call in the fused modes.
 */
#define DTTS_MAX_VOCODER_BATCH 2048
DTTS_API int dtts_hifigan_forward(dtts_handle h, const float* mel_dev, const int32_t* lens_dev, int B, int T, float* wav_dev,
                         dtts_stream stream);
DTTS_API int dtts_hifigan_hop(dtts_handle h); /* product of upsample_rates (256) */

/*
 * FastSpeech FFT block stack — replaces FFTBlocks.forward (modules/fastspeech/tts_modules.py:495-523) at inference:
 * x [B,T,hidden] f32 -> y [B,T,hidden] f32.  lens [B] i32 = valid frames per utterance, or NULL: derived from the
 * values as the reference does (frames whose |x| sums to zero are padding; padding must be a suffix).
 * pos_table [n_pos][hidden] f32 = SinusoidalPositionalEmbedding.weights (modules/commons/common_layers.py:110-127,
 * row 0 = padding) when the stack was built with use_pos_embed, n_pos > T; otherwise NULL.  Positions follow
 * make_positions(x[...,0]) (utils/tts_utils.py:6-18): a frame whose first channel is exactly 0 gets row 0.
 * Weights: dtts_load_weight("fft.<key of FFTBlocks.state_dict()>"), dtts_finalize_weights(h, DTTS_PART_FFT).
 */
DTTS_API int dtts_fft_blocks_forward(dtts_handle h, const float* x_dev, const int32_t* lens_dev, const float* pos_table_dev, int n_pos,
                            int B, int T, float* y_dev, dtts_stream stream);

/*
 * Gloss embeddings — dtts_text2mel_fetch(h, DTTS_GLOSS_ENCODE, (dtts_gloss_args*), stream), args->size = sizeof(*args): not a copy, needs NO
 * encode, and not one of the DTTS_OUT_* outputs of the text-to-mel path (it makes an INPUT of that path: the dictionary's embeddings); it
 * goes through the same dispatcher as the block items so that the library keeps its entry points.  Replaces get_encodings of the
 * reference's binariser (data_gen/tts/binarizer_zh.py) for n_gloss glosses at once, with the encoder of dtts_finalize_weights(DTTS_PART_GLOSS).  The glosses are packed back to back as ONE ragged sequence: gloss g owns rows
 * tok_off[g] .. tok_off[g + 1] - 1 of ids_dev ([CLS] .. [SEP] included) and of out_dev; L_g = its length, 1 .. DTTS_GLOSS_MAX_L.  Per gloss,
 * alone (no padded rows exist, a row's arithmetic never depends on another gloss):
 *   E = word_embeddings[ids]; h_0 = LN(E + token_type_embeddings[0]); h_(l+1) = layer l of h_l, a post-LN BERT layer whose q and k are
 *   rotated per head of 64 channels by the position's angle p / 10000^(2 j / 64) (pairs (2 j, 2 j + 1); v is not rotated), scores / 8,
 *   softmax over the gloss's own L_g keys, erf-GELU feed-forward; out = (E + h_0 + .. + h_n) / (n + 2), summed in that order in fp32.
 * Dense layers: exact fp32 products in a fixed order (a row's bits depend on the layer alone); LayerNorm with the biased variance.  No
 * atomics: a gloss's rows are bit-identical alone and at any place in any batch.  An id outside [0, vocab) gives a zero E row and
 * status_dev i64 [2] = {first offending row + 1, that id} (0, 0: every id valid; written by every call).
 * tok_off_dev is copied to the host and checked before the first launch (one stream synchronisation per call).  Workspace:
 * sum_L * (3 hidden + max(4 hidden, ffn)) floats.
 * DTTS_E_INVAL (naming the value): a wrong size, n_gloss < 1, L_max outside 1 .. DTTS_GLOSS_MAX_L, a sum_L that n_gloss glosses of 1 .. L_max
 * tokens cannot have or that exceeds what one call takes, a NULL or misaligned pointer — all checked before the handle — then
 * tok_off[0] != 0, a gloss of fewer than 1 or more than DTTS_GLOSS_MAX_L tokens, tok_off[n_gloss] != sum_L, an L_max that is not the
 * longest gloss's length.  DTTS_E_STATE before dtts_finalize_weights(DTTS_PART_GLOSS).
 */
#define DTTS_GLOSS_ENCODE 64
#define DTTS_GLOSS_MAX_L 64
typedef struct dtts_gloss_args {
    int32_t size;                 /* sizeof(dtts_gloss_args) */
    int32_t n_gloss;
    int32_t sum_L;                /* rows of ids_dev / out_dev */
    int32_t L_max;                /* the longest gloss's length */
    const int64_t* ids_dev;       /* [sum_L] */
    const int32_t* tok_off_dev;   /* [n_gloss + 1] */
    float* out_dev;               /* [sum_L][hidden] */
    int64_t* status_dev;          /* [2] */
} dtts_gloss_args;

/*
 * The PortaSpeech baseline's encode — dtts_text2mel_fetch(h, DTTS_PS_ENCODE, (dtts_ps_args*), stream), args->size = sizeof(*args): replaces
 * PortaSpeech.run_text_encoder (modules/portaspeech/model.py:239-288) with the part of dtts_finalize_weights(DTTS_PART_PORTASPEECH):
 *   phoneme TextEncoder (embedding * sqrt(hidden), ConvReluNorm prenet, post-LN relative-position Transformer) -> ph_encoder_out;
 *   phoneme -> word mean pooling, the word encoder (FFTBlocks), the duration predictor on ph_encoder_out and the per-word duration sums;
 *   length regulation (or the teacher-forced mel2word), padded to frames_multiple by repeating the last column;
 *   the single-head attention of every mel frame over the phonemes of its own word -> decoder_inp [B][T_mel][hidden].
 * It leaves the context encoded exactly as dtts_text2mel_encode does, with decoder_inp as the FVAE's condition: dtts_text2mel_decode,
 * DTTS_OUT_DUR / _MEL2WORD / _X_MASK / _MEL_LENS / _WORD_ENCODER_OUT and the three copy items below work afterwards; the Dict-TTS-only items
 * (DTTS_OUT_PRON_ATTN, _DICT_ATTN, _CONTEXT, _POSTERIOR) answer DTTS_E_STATE.  One stream synchronisation when mel2word_dev is NULL, none
 * otherwise.
 * Inputs: txt_tokens [B][T_ph] i64 (0 = padding, a suffix), ph2word [B][T_ph] i64 (1-based word of a phoneme: over the live prefix it
 * starts at 0 or 1 and grows by 0 or 1 per phoneme, so a word is a span and no word in front of the last one is empty — stricter than the
 * reference, which pools an empty word into a zero row: such a row inside an utterance would break the suffix padding the word encoder
 * derives from all-zero rows; 0 past the live prefix), mel2word [B][T_m2w] i64 or NULL (non-decreasing over its non-zero prefix, 0 behind it).
 * status_dev i64 [4], written by every call: {0, 0, 0, 0}, or {first offending utterance + 1, code, value, position} with code
 *   DTTS_PS_BAD_TOKEN     a token outside [0, n_phone);
 *   DTTS_PS_ZERO_TOKEN    a zero token inside the live prefix (the prefix mask and txt_tokens > 0 would differ);
 *   DTTS_PS_BAD_PH2WORD   a ph2word that, inside the live prefix, decreases, skips a word (a step > 1, or a first value > 1) or exceeds
 *                         T_w; that is negative; or that is non-zero past the prefix;
 *   DTTS_PS_EMPTY_WORD    a live frame whose word has no phonemes (the reference's fp32 sum q.k - 1e9 makes that row a batch-dependent
 *                         uniform average: refused by name, not imitated);
 *   DTTS_PS_BAD_MEL2WORD  a mel2word outside [0, T_w] or not of the form above.
 * The first three are checked at the call's synchronisation (DTTS_E_INVAL naming them); without one (mel2word given), and for the last
 * two, the caller reads status_dev after the call.  Nothing is read or written out of range for any such input.
 * Deviation: attn rows of frames with mel2word = 0 are written as zeros; the reference leaves meaningless softmax rows there, which never
 * reach decoder_inp.
 * DTTS_E_INVAL, checked before the handle: a wrong size, B / T_ph / T_w < 1, T_m2w < 0 or mel2word without T_m2w, a NULL txt_tokens /
 * ph2word / status_dev / T_mel_host, a misaligned pointer.  DTTS_E_STATE before dtts_finalize_weights(DTTS_PART_PORTASPEECH).
 * The copy items (dst = a device buffer, after a DTTS_PS_ENCODE): DTTS_PS_PH_ENCODER_OUT f32 [B][T_ph][hidden], DTTS_PS_ATTN f32
 * [B][T_mel][T_ph] (needs want_attn), DTTS_PS_DECODER_INP f32 [B][T_mel][hidden].
 */
#define DTTS_PS_ENCODE 65
#define DTTS_PS_PH_ENCODER_OUT 66
#define DTTS_PS_ATTN 67
#define DTTS_PS_DECODER_INP 68
#define DTTS_PS_BAD_TOKEN 1
#define DTTS_PS_ZERO_TOKEN 2
#define DTTS_PS_BAD_PH2WORD 3
#define DTTS_PS_EMPTY_WORD 4
#define DTTS_PS_BAD_MEL2WORD 5
typedef struct dtts_ps_args {
    int32_t size;                 /* sizeof(dtts_ps_args) */
    int32_t B, T_ph, T_w;
    int32_t T_m2w;                /* columns of mel2word_dev, or 0 */
    int32_t want_attn;            /* != 0: keep the attention weights for DTTS_PS_ATTN */
    const int64_t* txt_tokens_dev;
    const int64_t* ph2word_dev;
    const int64_t* mel2word_dev;  /* or NULL: predicted durations */
    int64_t* status_dev;          /* [4] */
    int32_t* T_mel_host;          /* out: frames per utterance, padded to frames_multiple */
} dtts_ps_args;

/*
 * Editing the resident dictionary — dtts_text2mel_fetch(h, DTTS_DICT_EDIT, (dtts_dict_edit_args*), stream), args->size = sizeof(*args): not a
 * copy and not one of the DTTS_OUT_* outputs (it changes an INPUT of the id path: the table of dtts_dict_table_upload); it goes through the
 * dispatcher of the block items so that the library keeps its entry points.  Replaces and appends entries of the resident table WITHOUT
 * uploading the dictionary again: afterwards the table is, bit for bit, what dtts_dict_table_upload would have built from the edited
 * dictionary (CSR offsets, K, V, key_map, pinyin, pinyin_map, the per-entry largest sense).  Entry order is kept; a replaced entry holds its new
 * rows, appended entries come at the end; ids of other entries do not change.  There is no deletion: replace with the '<UNK>' item.
 *   entry_id_host [n_edit] i32, strictly ascending: a value < n_entries replaces that entry; the values n_entries, n_entries + 1, ...
 *     (contiguous, after the replacements) append.  tok_off_host / pin_off_host [n_edit + 1]: the ragged offsets (from 0) of the edited
 *     entries' gloss rows and pinyin slots; an entry may have 0 rows or 0 slots.  key_map_host f32 [sum L], pinyin_host / pinyin_map_host
 *     i64 [sum P]: HOST arrays, as in the upload.
 *   keys / values f32 [sum L][gloss_dim]; values may be NULL = keys, as in the upload.  rows_on_device = 0: HOST pointers (staged on the
 *     device by the call); 1: DEVICE pointers, 16-byte aligned, written by work enqueued earlier on `stream` (for example the gloss
 *     encoder's output): the new rows never touch the host.
 * Only the sum L new rows are projected (k_transform / v_transform, the upload's kernels: a row's bits do not depend on its position or
 * on the row count); one segment-copy launch per array moves the unchanged runs of the old table and the projected rows into the new
 * arrays, which are built BESIDE the old ones (transient memory: twice the table), then swapped in.  The work runs on `stream`, behind
 * what the caller enqueued there; like the upload the call is synchronous for the host, and it synchronises the DEVICE once before it
 * releases the previous arrays (nothing may still be using them).  It is therefore an ADMINISTRATIVE call, made when the dictionary
 * changes, never per batch.  Encodes enqueued before the call read the old table, encodes after it the new one.
 * A refused or failed edit leaves the previous table in use and intact.  n_edit = 0 succeeds and does nothing.
 * DTTS_E_INVAL (naming the value), checked before the handle: a wrong size, n_edit < 0, a NULL array, ids that are negative or not strictly
 * ascending, offsets that do not start at 0 or decrease, more than INT_MAX / 2 rows, a sense index above DTTS_MAX_SENSES in key_map or
 * pinyin_map (the upload's wording), misaligned device rows; after it: appended ids that leave a gap behind n_entries, a table that would
 * exceed INT_MAX / 2 rows.  DTTS_E_STATE: acoustic weights not finalised, no table resident, another current HIP device than the
 * context's.  DTTS_E_NOMEM: the new arrays do not fit beside the old ones.
 *
 * Reading an entry back — dtts_text2mel_fetch(h, DTTS_DICT_ENTRY, (dtts_dict_entry_args*), stream): "what does the table hold for this
 * word".  n_entries, L_e and P_e are filled at once from the context's host copy of the offsets; each device destination that is not NULL
 * receives, by a copy enqueued on `stream`, the entry's projected rows K / V f32 [L_e][hidden], key_map f32 [L_e], pinyin / pinyin_map i64
 * [P_e].  entry = -1 only reports n_entries (0 without a table).  Call once with NULL destinations for the sizes, then with buffers.
 * DTTS_E_INVAL: a wrong size, a misaligned destination (both before the handle), an entry outside [-1, n_entries).  DTTS_E_STATE: no table
 * resident (entry >= 0).
 */
#define DTTS_DICT_EDIT 69
#define DTTS_DICT_ENTRY 70
typedef struct dtts_dict_edit_args {
    int32_t size;                    /* sizeof(dtts_dict_edit_args) */
    int32_t n_edit;
    int32_t rows_on_device;          /* 0: keys / values are host pointers; 1: device pointers, 16-byte aligned */
    int32_t reserved;
    const int32_t* entry_id_host;    /* [n_edit] */
    const int32_t* tok_off_host;     /* [n_edit + 1] */
    const int32_t* pin_off_host;     /* [n_edit + 1] */
    const float* key_map_host;       /* [sum L] */
    const int64_t* pinyin_host;      /* [sum P] */
    const int64_t* pinyin_map_host;  /* [sum P] */
    const float* keys;               /* [sum L][gloss_dim] */
    const float* values;             /* the same shape, or NULL = keys */
} dtts_dict_edit_args;
typedef struct dtts_dict_entry_args {
    int32_t size;                    /* sizeof(dtts_dict_entry_args) */
    int32_t entry;                   /* 0 .. n_entries - 1, or -1: only n_entries */
    int32_t n_entries, L_e, P_e;     /* out (host) */
    int32_t reserved;
    float* k_dev;                    /* [L_e][hidden] or NULL */
    float* v_dev;                    /* [L_e][hidden] or NULL */
    float* key_map_dev;              /* [L_e] or NULL */
    int64_t* pinyin_dev;             /* [P_e] or NULL */
    int64_t* pinyin_map_dev;         /* [P_e] or NULL */
} dtts_dict_entry_args;

/*
 * Output side — replaces the sample conversion of save_wav (utils/audio.py:11-16; called from after_infer,
 * tasks/tts/dict_tts.py:282-283) for a batch, on the device, so that the device->host copy is int16:
 * wav [B, T*hop] f32 as dtts_hifigan_forward wrote it, lens [B] i32 valid frames (NULL = T for all);
 * per utterance over its own lens[b]*hop samples: norm != 0 -> w / max|w| ; w * 32767 (fp32) ; truncating cast.
 * out [B, T*hop] i16, samples past an utterance's end are 0.
 */
DTTS_API int dtts_wav_to_int16(dtts_handle h, const float* wav_dev, const int32_t* lens_dev, int B, int T, int norm, int16_t* out_dev,
                      dtts_stream stream);

/* Seed of the device-side prior sample (z_p == NULL in dtts_text2mel_decode / _forward*).  Every context starts from a seed mixed from
 * the time, the process id, the device and a per-process instance count, so that data-parallel ranks and restarts draw different
 * noise (the reference draws from torch's global RNG, modules/dict_tts/fvae_semantics.py:110-111); setting it makes a run repeatable. */
DTTS_API int dtts_set_noise_seed(dtts_handle h, uint64_t seed);

/* fp16 range guard (DTTS_VOC_F16), the CENSUS form.  The ResBlock convolutions convert their activations to fp16: |v| > 65504 becomes
 * +-inf, where the reference computes in fp32 (modules/hifigan/hifigan.py:51-58).  While the guard is on, the fused ResBlock kernels run an
 * instantiation that COUNTS such activations at every one of the 72 conversion points (a few % slower); dtts_vocoder_clamped returns the
 * count accumulated since the last reset (it synchronises `stream`).  A testing / diagnosis aid: the always-on detector below needs no mode. */
DTTS_API int dtts_vocoder_range_guard(dtts_handle h, int enable);
DTTS_API int dtts_vocoder_clamped(dtts_handle h, int64_t* count, int reset, dtts_stream stream);

/* fp16 validity of DTTS_VOC_F16 as a DECISION, in two parts (the reference computes the ResBlocks in fp32, modules/hifigan/hifigan.py:51-58):
 *
 * (1) ALWAYS-ON detector.  The fp16 conversion of the ResBlock operands does not saturate: an activation beyond +-65504 becomes +-inf,
 *     every sum it enters is inf / NaN from there on, and it reaches conv_post as a non-finite pre-tanh value.  The conv_post epilogue of
 *     EVERY forward (release instantiations included, no mode to switch on) writes NaN for such a sample instead of tanh's plausible +-1
 *     and counts it; dtts_hifigan_forward copies the running count to pinned host memory behind its last kernel.  dtts_vocoder_nonfinite
 *     returns that word WITHOUT synchronising: once the caller has synchronised with the forward's stream (it must, to read the waveform)
 *     the value covers that forward.  The count is cumulative over the context's life; compare it with the value before the call.  A call
 *     that overflowed is therefore ALWAYS reported (dict_tts_amd/vocoder.py redoes it in DTTS_VOC_BF16X3, or raises when fp16 was demanded).
 * (2) STATIC bound, computed by dtts_finalize_weights from the folded weights.  worst_case: an upper bound of every value the ResBlocks round
 *     to fp16, for ANY mel with |mel| <= mel_abs_max (per-channel L1 propagation: |b| + sum|w| * bound_in through all 72 convolutions; the
 *     reference's log10-mel lies in [-6, 1.5], egs/egs_bases/tts/base.yaml:59-60).  worst_case < 65504 PROVES that no call in that range can
 *     overflow.  rms_estimate: the propagated root-mean-square of the largest such channel (independence assumed: an estimate, not a bound);
 *     a checkpoint whose estimate already nears 65504 / 16 should not be run in fp16 at all.  For trained generators the worst case is
 *     astronomically loose (it compounds sum|w| ~ 10-40 per convolution), so part (1) is what protects them.  Either pointer may be NULL.
 *     Other precisions: both 0 (bf16 has fp32's exponent range). */
DTTS_API int dtts_vocoder_nonfinite(dtts_handle h, int64_t* count);
DTTS_API int dtts_vocoder_fp16_bound(dtts_handle h, float mel_abs_max, double* worst_case, double* rms_estimate);

/* Memory-safety mode (dtts_config.debug_redzone = 1; a testing aid with no counterpart in the reference — the kernels behind this ABI
 * address raw HBM).  Every workspace buffer of the last encode / decode / vocoder / FFT-block call and every weight pack / table sits
 * between two 4 KiB red zones filled with 0xFF, and the workspaces are filled with 0xFF (NaN) before each forward.  dtts_debug_check
 * synchronises `stream` and counts the red-zone bytes that are no longer 0xFF (= an out-of-range WRITE; dtts_last_error names the first
 * damaged zone); an out-of-range or stale READ that is consumed shows up as NaN in the outputs.  DTTS_E_STATE without the mode. */
DTTS_API int dtts_debug_check(dtts_handle h, int64_t* damaged_bytes, dtts_stream stream);
/* self-test of the mode: damages one red-zone byte (as an off-by-one store would); the next dtts_debug_check must report it */
DTTS_API int dtts_debug_poke(dtts_handle h, dtts_stream stream);

/*
 * Instrumentation used by bench.py: accumulated device time (hipEvent pairs recorded on the caller's stream
 * around every launch of one kernel family) since the last reset.
 */
#define DTTS_TIMER_VOC_CONV 1   /* the vocoder's MFMA convolution kernel (dominant kernel) */
#define DTTS_TIMER_S2PA 2       /* the S2PA dictionary-attention kernel                    */
/* stage spans under the names of the reference's profile_infer timers (utils.Timer): one event pair per call, launches = calls */
#define DTTS_TIMER_STAGE_ENCODER 3      /* 'encoder'      modules/dict_tts/model.py:50  = dtts_text2mel_encode* (device span, incl. the T_mel sync wait) */
#define DTTS_TIMER_STAGE_DICT_ENCODER 4 /* 'dict_encoder' modules/dict_tts/model.py:86  = embedding, both encoders, S2PA                                   */
#define DTTS_TIMER_STAGE_FVAE 5         /* 'fvae'         modules/dict_tts/model.py:57  = dtts_text2mel_decode (gather-expand + prior flow + decoder)       */
#define DTTS_TIMER_STAGE_HIFIGAN 6      /* 'hifigan'      vocoders/hifigan.py:59        = dtts_hifigan_forward                                              */
#define DTTS_TIMER_DICT_SEG_COPY 7      /* DTTS_DICT_EDIT: the segment-copy launch that moves the K array (one per edit; tools/dict_edit_bench.py)                 */
#define DTTS_TIMER_COUNT 8
DTTS_API int dtts_timer_enable(dtts_handle h, int which);
DTTS_API int dtts_timer_read(dtts_handle h, int which, double* ms_total, int64_t* launches); /* synchronises */
DTTS_API int dtts_timer_reset(dtts_handle h);

#ifdef __cplusplus
}
#endif
#endif
