// Internal to libdicttts_hip.so (not installed): the context behind dtts_handle with its workspace arenas and timers, and what the host
// units share: error reporting, weight access and packing (pack.hip), parameter blocks, the builders dtts_finalize_weights calls.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <ctime>
#include <functional>
#include <unistd.h>
#include <map>
#include <string>
#include <vector>

#include "../../include/dicttts_hip.h"
#include "conv1d.h"
#include "ops.h"
#include "vconv.h"
#include "rblock.h"
#include "vpair.h"
#include "rb2x.h"
#include "rbn.h"
#include "flowstack.h"
#include "melspec.h"
#include "stftdist.h"
#include "istft.h"
#include "losses.h"
#include "dtw.h"
#include "pitch.h"
#include "resample.h"
#include "loudness.h"
#include "disc.h"
#include "spkenc.h"
#include "meldisc.h"
#include "gloss.h"
#include "portaspeech.h"
#include "dict_edit.h"

// dtts_config.tune_flags: the bits the library honours are listed at TUNE_RELEASE_MASK (context.hip)
#define DTTS_TUNE(h, bit) (((h)->tune & (bit)) != 0)

namespace dtts {

struct HostTensor {
    std::vector<float> f;
    std::vector<double> d;   // the "resample." tensors arrive as DTTS_F64 and keep their precision (f is empty then)
    std::vector<int64_t> shape;
    int64_t numel() const {
        int64_t n = 1;
        for (auto s : shape) n *= s;
        return n;
    }
};

// Memory-safety mode (dtts_config.debug_redzone, tests only): every workspace buffer sits between two RED ZONES of RZ bytes, the whole
// arena is filled with 0xFF (= NaN as fp32 / fp16 / bf16, -1 as an integer) before each forward, so that
//   * an out-of-range WRITE of a kernel damages a red zone (dtts_debug_check counts the bytes that are no longer 0xFF),
//   * an out-of-range or stale READ that is actually consumed shows up as NaN in the outputs (buffers are never zero by luck).
// Weight packs / tables (dev_alloc below) get the same red zones.  Off (the default): no red zones, no fills, no cost.
constexpr size_t RZ = 4096;

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool debug = false;
    struct Buf { size_t start, bytes; };
    std::vector<Buf> bufs;   // debug: the buffers handed out since the last reserve / rewind
    static constexpr int DBG_BUFS = 1024;   // debug mode budgets red zones for this many buffers per forward (the largest forward hands out < 100)
    hipError_t reserve(size_t n, hipStream_t s) {
        off = 0;
        bufs.clear();
        if (debug) n += (size_t)DBG_BUFS * (RZ + 256);   // red zones + alignment of up to DBG_BUFS buffers (alloc fails beyond: see below)
        if (n > cap) {
            if (base) {
                hipError_t e = hipDeviceSynchronize();
                if (e != hipSuccess) return e;
                (void)hipFree(base);
                base = nullptr;
                cap = 0;
            }
            n = n + n / 8 + (1 << 20);
            hipError_t e = hipMalloc((void**)&base, n);
            if (e != hipSuccess) return e;
            cap = n;
        }
        if (debug) return hipMemsetAsync(base, 0xFF, cap, s);
        return hipSuccess;
    }
    void rewind() {   // walk the same layout again (decode re-derives the buffers encode laid out)
        off = 0;
        bufs.clear();
    }
    template <class T>
    T* alloc(size_t count) {
        if (debug) off += RZ;
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        if (off + bytes + (debug ? RZ : 0) > cap) return nullptr;
        T* p = (T*)(base + off);
        if (debug) bufs.push_back({off, count * sizeof(T)});
        off += bytes;
        return p;
    }
    void release() {
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = off = 0;
        bufs.clear();
    }
};

struct EncLayer {
    PackedConv qkv, o, ffn1, ffn2;
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr;
};
struct Encoder {
    std::vector<EncLayer> l;
    float *lg = nullptr, *lb = nullptr;
};
// an FFT block stack (FFTBlocks / FastspeechDecoder): the context's "fft." part and the PortaSpeech baseline's word encoder
struct FftStack {
    std::vector<EncLayer> l;
    float *g = nullptr, *b = nullptr, *alpha = nullptr;   // the last LayerNorm (or null), pos_embed_alpha (or null = 1)
    int K = 9;                                            // FFN kernel size
    bool pos = true, last_norm = true;
};
// the buffers a stack runs in, rows = B * T: x, hb, att [rows][C], qkv [rows][3C], ff [rows][4C], lens [B], pos [rows]
struct FftBufs {
    float *x, *hb, *qkv, *att, *ff;
    int *lens, *pos;
};
// a layer of the baseline's relative-position phoneme encoder (post-LN): emb_rel_k / emb_rel_v [2 w + 1][d_k]
struct PsLayer {
    PackedConv qkv, o, ffn1, ffn2;
    float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr, *ek = nullptr, *ev = nullptr;
};
struct WNet {
    PackedConv cond;
    std::vector<PackedConv> in, rs;
    int hidden = 0, layers = 0;
};
struct Flow {
    PackedConv pre, post;
    WNet wn;
    int in_coff = 0, out_coff = 0;  // physical channel offsets of the logical x0 / x1 halves (flip parity)
};

struct TimerSlot {
    bool enabled = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    double ms_done = 0;
    int64_t launches = 0;
};

} // namespace dtts

struct dtts_ctx {
    dtts_config cfg;
    std::string err;
    std::map<std::string, dtts::HostTensor> w;
    std::vector<void*> allocs;
    bool debug_rz = false;                                   // dtts_config.debug_redzone
    int device = 0;                                          // the HIP device that was current at dtts_create: weights and workspaces live there
    int n_cu = 256;                                          // its compute units
    struct StaticBuf { char* p; size_t bytes; };
    std::vector<StaticBuf> rz_static;                         // debug: weight packs / tables (user pointer, payload bytes) between red zones
    bool acoustic_ready = false, vocoder_ready = false, fft_ready = false;
    // ---- FFT block stack
    dtts::FftStack fft;
    dtts::Arena a_fft;
    // ---- acoustic model
    float *word_emb = nullptr, *pinyin_emb = nullptr;
    dtts::Encoder sem, lin;
    dtts::PackedConv s2_q, s2_kT, s2_k, s2_v, s2_o;   // s2_kT: k_transform applied transposed to the query (tensor API); s2_k: to the table rows at upload
    std::vector<dtts::PackedConv> dur_conv;
    std::vector<float*> dur_g, dur_b;
    float *dur_w = nullptr, *dur_bias = nullptr;
    dtts::PackedConv g_pre, g_pre_poly, dec_pre, dec_out;   // g_pre_poly: the strided g_pre_net as a 3-tap convolution over 4-frame groups (vconv), or empty
    std::vector<dtts::Flow> flows;  // in execution (reversed) order
    float* fs_w = nullptr;    // packed weights of the fused prior-flow kernel (flowstack.hip), or null = launch by launch
    dtts::PackedConv fs_cond;       // cond_layer of ALL blocks as one 1x1 convolution (execution order)
    dtts::WNet dec_wn;
    // ---- vocoder
    dtts::PackedConv conv_pre, conv_post;
    std::vector<dtts::PackedConv> ups;
    std::vector<std::vector<dtts::PackedConv>> rb1, rb2;  // [resblock][3]
    std::vector<std::vector<dtts::PackedConv>> rbf1, rbf2;  // fused-ResBlock copies (taps zero padded), empty where unsupported
    // ResBlock2 generators (two-dilation rows: resblock_dilation_sizes[j][2] == 0): rb1[i] = convs.{0,1} for the per-convolution path,
    // rbf1[i] = the same, tap-padded, for the fused kernel (rb2x.hip); rb2 / rbf2 stay empty
    bool resblock2 = false;
    int hop = 1;
    int tune = 0;
    float *post_w = nullptr, *post_b = nullptr;   // conv_post as [taps][C] fp32 for the fused epilogue of the last ResBlock (rblock.hip), or null
    // ---- workspaces and per-call state
    dtts::Arena a_enc, a_dec, a_voc;
    unsigned* amax_bits = nullptr;  // dtts_wav_to_int16 scratch
    unsigned long long noise_counter = 0x5EEDull;   // device prior samples (z_p == NULL): one stream per call, offset by noise_seed
    unsigned long long noise_seed = 0;              // per context (dtts_create: time, pid, device, instance; dtts_set_noise_seed overrides)
    unsigned long long* ovf_dev = nullptr;          // fp16 range guard counter (DTTS_VOC_F16), device
    bool guard_on = false;
    bool debug_misorder = false;                             // dtts_config.debug_redzone = 2: the whole-ResBlock launches declare the other fragment order (self-test)
    // always-on overflow detector of the 16-bit vocoder modes: non-finite pre-tanh values counted by the conv_post epilogue (device), and the
    // pinned host word every dtts_hifigan_forward copies it to behind its last kernel (dtts_vocoder_nonfinite reads it without a sync)
    unsigned* bad_dev = nullptr;
    volatile unsigned* bad_host = nullptr;
    // static fp16 analysis of the ResBlock operands (build_vocoder): bound(M) <= wc_lin * M + wc_const for |mel| <= M (worst case, L1),
    // est_lin * M + est_const = the propagated RMS (an ESTIMATE under independence); 0 / 0 when the mode has no fp16 operands
    double wc_lin = 0, wc_const = 0, est_lin = 0, est_const = 0;
    bool voc_span = false;                          // DTTS_TIMER_VOC_CONV: one event pair spans the whole kernel family of a forward (below)
    int amax_cap = 0;
    int B = 0, T_w = 0, L_k = 0, P = 0, T_mel = 0;
    bool encoded = false;
    float *weo = nullptr, *dur = nullptr, *pron_attn = nullptr, *dict_attn = nullptr, *context = nullptr, *x_mask = nullptr;
    int64_t* m2w = nullptr;
    int *mel_lens = nullptr, *lens = nullptr;
    dtts::TimerSlot timers[DTTS_TIMER_COUNT];
    // ---- resident dictionary table (dtts_dict_table_upload)
    int t_entries = 0;
    int *t_off = nullptr, *t_poff = nullptr, *t_pmmax = nullptr;
    float *t_keys = nullptr, *t_values = nullptr, *t_key_map = nullptr;
    int64_t *t_pinyin = nullptr, *t_pinyin_map = nullptr;
    // host mirrors of t_off / t_poff [t_entries + 1] and t_pmmax [t_entries], filled by the upload and by every edit (dict_edit.hip): an edit
    // computes the new offsets on the host, DTTS_DICT_ENTRY answers L_e / P_e from them at once
    std::vector<int> m_off, m_poff, m_pmmax;
    // ---- speaker conditioning (dtts_text2mel_speakers; modules/portaspeech/model.py:159-163, modules/dict_tts/model.py:44-45,94-96)
    int spk_kind = 0;                        // 0 = no spk_embed_proj loaded, DTTS_SPK_EMBED (Linear 256 -> hidden), DTTS_SPK_ID (Embedding)
    int spk_n = 0;                           // DTTS_SPK_ID: rows of the table (num_spk)
    float *spk_w = nullptr, *spk_bias = nullptr;   // Linear: W^T [256][hidden] + bias [hidden]; Embedding: table [num_spk][hidden]
    dtts::Arena a_spk;                             // the projected rows [B][hidden] + the id-check flag words, written by dtts_text2mel_speakers
    float* spk_rows = nullptr;
    unsigned long long* spk_flag = nullptr;
    int spk_armed_B = 0;                     // > 0: the next encode adds spk_rows (and disarms)
    unsigned spk_gen = 0, enc_spk_gen = 0;   // arming count; the one the last encode consumed
    bool enc_spk = false;                    // the last encode was conditioned on spk_rows
    // ---- FVAE posterior pass (dtts_text2mel_fetch(DTTS_OUT_POSTERIOR); modules/dict_tts/fvae_semantics.py:84-108), packed when the checkpoint carries
    // fvae.encoder.*; otherwise post_missing names the first absent tensor and the call is refused.  A shape the pass does not support
    // still loads for inference: post_unsupported says why, and the posterior call is refused with it
    bool post_ready = false;
    std::string post_missing, post_unsupported;
    dtts::PackedConv post_pre;                     // encoder.pre_net.0: Conv1d(n_mel -> hidden, k = 8, s = 4, p = 2)
    dtts::WNet post_wn;                            // encoder.wn (fvae_enc_n_layers layers, conditioned on g_sqz)
    float *post_wt = nullptr, *post_bias = nullptr;   // encoder.out_proj as W^T [hidden][2 latent] + bias [2 latent]
    std::vector<dtts::Flow> flows_fwd;             // the prior flow's couplings in EXECUTION order of the forward direction (+m, not -m)
    float* fs_w_fwd = nullptr;               // the same blocks packed for the fused kernel's masked forward form (flowstack.hip: MASK), or null
    dtts::PackedConv fs_cond_fwd;                  //   with their cond_layers as one 1x1 convolution in forward execution order
    dtts::Arena a_post;
    // ---- log-mel front end (dtts_text2mel_fetch(DTTS_OUT_MELSPEC); melspec.hip): the plan of the last dtts_finalize_weights(DTTS_PART_MELSPEC)
    bool melspec_ready = false;
    dtts::StftBasisPlan ms;                             // windowed DFT basis in fragment order, n_fft, the super-groups the window keeps
    int ms_n_mels = 0, ms_win = 0;
    float* ms_melpack = nullptr;                        // mel basis in fragment order (melspec_pack_mel)
    int ms_skew_hop = 0, ms_skew = 8;                   // the slab skew chosen for the hop of the last call
    // ---- multi-resolution STFT distance (dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE); stftdist.hip): the plans of the last
    // dtts_finalize_weights(DTTS_PART_STFT), one per "stft.<i>.window", and the workspace of the per-tile sums
    struct StftPlan {
        dtts::StftBasisPlan core;
        int layout_hop = 0, ps = 31, tt = 1, ybase = 0; // the LDS layout chosen for the hop of the last call (stft_layout)
    };
    std::vector<StftPlan> stft_plans;
    dtts::Arena a_stft;
    // ---- STFT -> magnitude edit -> inverse STFT (dtts_text2mel_fetch(DTTS_OUT_SPECTRAL); istft.hip): the plan of the last
    // dtts_finalize_weights(DTTS_PART_ISTFT) and the workspace of the spectrum and the windowed frames between the launches
    bool istft_ready = false;
    dtts::StftBasisPlan is;                             // the forward half's plan
    float* is_wi = nullptr;                             // inverse basis (istft_pack_inverse), fragment order
    double* is_w2 = nullptr;                            // the window's squares [n_fft]
    std::vector<float> is_window;                       // host copy: the envelope criterion is checked per hop
    std::map<int, double> is_env;                       // hop -> smallest envelope value (istft_envelope_min), per plan
    int is_skew_hop = 0, is_skew = 8;                   // the slab skew chosen for the hop of the last forward call
    float* is_pinv = nullptr;                           // "istft.inv_mel_basis" transposed, [n_mels][n_fft / 2 + 1], or null (griffinlim.hip)
    int is_pinv_mels = 0;
    dtts::Arena a_spec;
    // ---- validation losses (dtts_text2mel_fetch(DTTS_OUT_LOSSES); losses.hip): the SSIM window in fp64 (uploaded by the first call) and the
    // workspace of the per-tile sums
    double* loss_win = nullptr;
    dtts::Arena a_loss;
    // ---- dynamic time warping (dtts_text2mel_fetch(DTTS_OUT_DTW); dtw.hip): the workspace of the direction codes and of the costs (F > 1)
    dtts::Arena a_dtw;
    // ---- F0 extraction (dtts_text2mel_fetch(DTTS_OUT_PITCH); pitch.hip): the window tables of every window length nsw seen so far (w [nsw], then
    // wr [n_lag], fp64, made on the host) and the workspace of the stages between the launches
    std::map<int, double*> pitch_tabs;
    dtts::Arena a_pitch;
    // ---- band-limited resampling (dtts_text2mel_fetch(DTTS_OUT_RESAMPLE); resample.hip): the plan of the last
    // dtts_finalize_weights(DTTS_PART_RESAMPLE): the pairs (win[i], interp_delta[i]) in fp64.  The unit has no workspace
    bool resample_ready = false;
    const double2* rs_tab = nullptr;
    int rs_n_win = 0, rs_num_table = 0;
    // ---- BS.1770 loudness (dtts_text2mel_fetch(DTTS_OUT_LOUDNESS); loudness.hip): the block bounds (lo_j, hi_j) of the rate of the last
    // call, as far as any call needed them, and the workspace of the segment states and partial sums
    const int2* loud_bounds = nullptr;
    int loud_bounds_rate = 0, loud_bounds_n = 0;
    dtts::Arena a_loud;
    // ---- HifiGAN's discriminators (dtts_text2mel_fetch(DTTS_OUT_DISC); disc.hip, gconv.hip): the packs of dtts_finalize_weights(DTTS_PART_DISC)
    // and the one workspace every discriminator reuses (two activation buffers, the D outputs, the partial feature sums, the row tables)
    bool disc_ready = false;
    dtts::DiscMpd mpd[5];
    dtts::DiscMsd msd[3];
    dtts::Arena a_disc;
    // ---- the d-vector speaker encoder (dtts_text2mel_fetch(DTTS_OUT_SPKENC); spkenc.hip): the packs of dtts_finalize_weights(DTTS_PART_SPKENC)
    // and the one workspace of a chunk of utterances (tables, mel, the projection, two hidden sequences, the partials)
    bool spkenc_ready = false;
    dtts::SpkLayer spk_layer[3];
    float *spk_lin_wt = nullptr, *spk_lin_b = nullptr;   // linear.weight transposed [k][o], linear.bias
    float *spk_fb = nullptr, *spk_basis = nullptr;       // mel basis [40][201]; windowed DFT basis [400][402]
    dtts::Arena a_spkenc;
    // ---- the multi-window mel discriminator (dtts_text2mel_fetch(DTTS_OUT_MELDISC); meldisc.hip): the packs of
    // dtts_finalize_weights(DTTS_PART_MELDISC) and the one workspace of a chunk of signals (clip table, three maps, statistics, D rows)
    bool meldisc_ready = false, meldisc_per_row = false;   // per_row: disc_reduction none (a head per remaining time row)
    int meldisc_H = 0, meldisc_nwin = 0;
    dtts::MelDiscWin meldisc[DTTS_MELDISC_MAX_WIN];
    const float2* meldisc_ident = nullptr;                 // (0, 1) [H]
    const float* meldisc_zero = nullptr;                   // 0 [H]
    dtts::Arena a_meldisc;
    // ---- the gloss encoder (dtts_text2mel_fetch(DTTS_GLOSS_ENCODE); gloss.hip): the packs of dtts_finalize_weights(DTTS_PART_GLOSS) and the one workspace of a
    // call (the hidden rows, the attention block's output, the running sum, and q | k | v + ctx sharing their rows with the feed-forward's)
    bool gloss_ready = false;
    std::vector<dtts::GlossLayer> gloss_layers;
    float *gloss_word = nullptr, *gloss_tt0 = nullptr, *gloss_eg = nullptr, *gloss_eb = nullptr;   // word_embeddings, token_type row 0, embeddings.LayerNorm
    const float2* gloss_rot = nullptr;                     // (sin, cos) [64][32]
    int gloss_vocab = 0, gloss_C = 0, gloss_F = 0;
    float gloss_eps = 0.f;
    dtts::Arena a_gloss;
    // ---- the PortaSpeech baseline (dtts_text2mel_fetch(DTTS_PS_ENCODE); portaspeech.hip): the packs of dtts_finalize_weights(DTTS_PART_PORTASPEECH)
    // beside the duration predictor and the FVAE it shares with the Dict-TTS part (dur_*, g_pre, flows, dec_*), and the workspace of an
    // encode, which keeps the dense condition of the decode (decoder_inp) and the three items a fetch may copy
    bool ps_ready = false;
    int ps_window = 4;
    float* ps_emb = nullptr;                          // ph_encoder.emb [n_phone][hidden]
    dtts::PackedConv ps_pre[3], ps_pre_proj;          // the prenet's convolutions and its 1x1 projection
    float *ps_pre_g[3] = {nullptr, nullptr, nullptr}, *ps_pre_b[3] = {nullptr, nullptr, nullptr};
    std::vector<dtts::PsLayer> ps_layers;
    dtts::FftStack ps_word;                           // word_encoder
    float* ps_pos_table = nullptr;                    // its sinusoid table [ps_n_pos][hidden]
    int ps_n_pos = 0;
    float* ps_freq = nullptr;                         // sin_pos frequencies [hidden / 2]
    dtts::PackedConv ps_enc_pos, ps_dec_qr, ps_q, ps_kv, ps_out;   // enc_pos_proj; dec_query_proj | dec_res_proj; attn's Wq; Wk | Wv; out_proj
    dtts::Arena a_ps, a_psf;                          // the phoneme / word side, and the frames' (sized once T_mel is known)
    bool ps_encoded = false;                          // the last successful encode was the baseline's: decode reads ps_g
    float *ps_g = nullptr, *ps_ph_out = nullptr, *ps_attn = nullptr;
    int ps_T_ph = 0;
};

namespace dtts {

// context.hip: records the message (h == null: for dtts_last_error(NULL)) and returns `code`
int fail(dtts_ctx* h, int code, const char* fmt, ...);

// ---- what the *_forward of every fetch unit opens with: the refusals of an argument block, each in its one wording (tests match the texts).
// A method returns 0 where there is nothing to refuse, else the code it recorded: `if (int rc = blk.size(a->size, sizeof *a)) return rc;`
struct Block {
    dtts_ctx* h;
    const char* me;   // "dtts_text2mel_fetch(DTTS_OUT_X)"
    int size(int got, size_t want) const {
        return got == (int)want ? 0 : fail(h, DTTS_E_INVAL, "%s: argument block of size = %d bytes, this library's is %d", me, got, (int)want);
    }
    template <size_t N>   // (an array of fixed length, so that the loop unrolls where n is a constant)
    int aligned(int n, const std::pair<const char*, const void*> (&ptrs)[N]) const {   // n: a power of two; null counts as aligned
        for (const auto& q : ptrs)
            if ((uintptr_t)q.second & (uintptr_t)(n - 1)) return fail(h, DTTS_E_INVAL, "%s: %s = %p is not aligned to %d bytes", me, q.first, q.second, n);
        return 0;
    }
    int handle() const { return h ? 0 : fail(nullptr, DTTS_E_INVAL, "%s: null handle", me); }
    int finalized(int part) const;   // context.hip: the part's row of UNITS says whether it is ready
    int workspace() const { return fail(h, DTTS_E_NOMEM, "%s: workspace", me); }
};

// the largest chunk of a batch of n whose workspace of bytes(chunk) stays within cap, found by halving (a chunk of 1 is taken as it is)
template <class F>
int chunk_within(int n, size_t cap, F bytes) {
    while (n > 1 && bytes(n) > cap) n = (n + 1) / 2;
    return n;
}

#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return fail(h, DTTS_E_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));   \
    } while (0)

#define LAUNCH(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return fail(h, DTTS_E_HIP, "%s: %s", #expr, hipGetErrorString(_e));             \
    } while (0)

// ---- pack.hip: device allocations owned by the context, weight access, folding and packing
void* dev_alloc(dtts_ctx* h, size_t bytes);
void dev_free(dtts_ctx* h, void* user);

template <class T>
T* upload(dtts_ctx* h, const std::vector<T>& v) {
    T* d = (T*)dev_alloc(h, v.size() * sizeof(T));
    if (!d) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}

bool pack_conv(dtts_ctx* h, PackedConv& L, int engine, int C_out, int C_in, int K, const std::function<float(int, int, int)>& getw,
               const std::vector<float>& bias, int dil, int stride, int pad, int gate_H = 0, double flops_per_row = -1, int frag = 32);

struct Need {
    dtts_ctx* h;
    std::string missing;
    const HostTensor* get(const std::string& name) {
        auto it = h->w.find(name);
        if (it == h->w.end()) {
            if (missing.empty()) missing = name;
            return nullptr;
        }
        return &it->second;
    }
};

const HostTensor* folded_weight(dtts_ctx* h, Need& need, const std::string& base);
std::vector<float> bias_of(Need& need, const std::string& base);
bool pack_plain(dtts_ctx* h, Need& need, PackedConv& L, int engine, const std::string& base, int dil, int stride, int pad,
                bool with_bias = true, int gate_H = 0, int frag = 32);
bool pack_transposed(dtts_ctx* h, Need& need, PackedConv& L, int engine, const std::string& base, int u, int p);
float* upload_named(dtts_ctx* h, Need& need, const std::string& name);

// ---- pack.hip: parameter blocks of a packed convolution (conv1d: base_params / set_res; vconv: vparams / vparams_x3)
ConvParams base_params(const float* x, int ldx, int B, int T_in, int T_out, float* y, int ldy);
void set_res(ConvParams& p, int s, const float* res, int ld);
VConvParams vparams(const PackedConv& L, const unsigned short* x, const int* lens, int B, int T);
VConvParams vparams_x3(const PackedConv& L, const float* xf, int ld, float in_slope, const int* lens, int B, int T);

// ---- one event pair around a span of launches (dtts_timer_*); nothing is recorded unless the timer is enabled
struct Timed {
    dtts_ctx* h;
    int which;
    hipStream_t s;
    hipEvent_t e1 = nullptr;
    Timed(dtts_ctx* h_, int which_, hipStream_t s_) : h(h_), which(which_), s(s_) {
        TimerSlot& t = h->timers[which];
        if (!t.enabled) return;
        if (which == DTTS_TIMER_VOC_CONV && h->voc_span) {   // inside a family span: count the launch, record nothing
            t.launches += 1;
            return;
        }
        if (t.used + 2 > t.pool.size()) {
            for (int i = 0; i < 256; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) return;
                t.pool.push_back(e);
            }
        }
        hipEvent_t e0 = t.pool[t.used];
        e1 = t.pool[t.used + 1];
        t.used += 2;
        t.launches += 1;
        (void)hipEventRecord(e0, s);
    }
    void stop() {   // close the span now (the destructor closes it at scope exit otherwise)
        if (e1) (void)hipEventRecord(e1, s);
        e1 = nullptr;
    }
    ~Timed() { stop(); }
};

// ---- the builders behind dtts_finalize_weights (text2mel_build.hip, vocoder.hip, fft_blocks.hip, melspec.hip)
int build_acoustic(dtts_ctx* h);
int build_vocoder(dtts_ctx* h);
int build_fft(dtts_ctx* h);
int build_melspec(dtts_ctx* h);   // melspec.hip
int check_wav_ld(dtts_ctx* h, const char* me, int wav_ld, int n_fft);   // melspec.hip: stft_wav_ld_ok or the one refusal (0 = in range)
int melspec_forward(dtts_ctx* h, const dtts_melspec_args* a, hipStream_t stream);
int build_stft(dtts_ctx* h);      // stftdist.hip
int stft_forward(dtts_ctx* h, const dtts_stft_args* a, hipStream_t stream);
int build_istft(dtts_ctx* h);     // istft.hip
int spectral_forward(dtts_ctx* h, const dtts_spectral_args* a, hipStream_t stream);
int check_envelope(dtts_ctx* h, const char* me, int hop);   // istft.hip: the inverse's criterion on (window, hop) or the one refusal (0 = met)
int griffin_lim(dtts_ctx* h, const dtts_griffinlim_args* a, hipStream_t stream);   // griffinlim.hip
int losses_forward(dtts_ctx* h, const dtts_loss_args* a, hipStream_t stream);     // losses.hip
int dtw_forward(dtts_ctx* h, const dtts_dtw_args* a, hipStream_t stream);          // dtw.hip (h may be null: the block is checked first)
int pitch_forward(dtts_ctx* h, const dtts_pitch_args* a, hipStream_t stream);      // pitch.hip (the same)
int build_resample(dtts_ctx* h);  // resample.hip
int resample_forward(dtts_ctx* h, const dtts_resample_args* a, hipStream_t stream);   // resample.hip (the same)
int loudness_forward(dtts_ctx* h, const dtts_loudness_args* a, hipStream_t stream);   // loudness.hip (the same)
int build_disc(dtts_ctx* h);      // disc.hip
int disc_forward(dtts_ctx* h, const dtts_disc_args* a, hipStream_t stream);           // disc.hip (the same)
int build_spkenc(dtts_ctx* h);    // spkenc.hip
int spkenc_forward(dtts_ctx* h, const dtts_spkenc_args* a, hipStream_t stream);       // spkenc.hip (the same)
int build_meldisc(dtts_ctx* h);   // meldisc.hip
int meldisc_forward(dtts_ctx* h, const dtts_meldisc_args* a, hipStream_t stream);     // meldisc.hip (the same)
int build_gloss(dtts_ctx* h);     // gloss.hip
int build_ps(dtts_ctx* h);        // portaspeech.hip
int ps_forward(dtts_ctx* h, const dtts_ps_args* a, hipStream_t stream);               // portaspeech.hip (the same)
// text2mel_build.hip: the halves of the acoustic part that the PortaSpeech baseline shares, from the tensors "<m>dur_predictor.*" / "<m>fvae.*"
bool build_dur_predictor(dtts_ctx* h, Need& need, const std::string& m);
bool build_fvae(dtts_ctx* h, Need& need, const std::string& m, int* rc);   // *rc != 0: refused with a message of its own
// text2mel.hip: the duration predictor's launches (in [B][T][cin] -> dur [B][T], d0 / d1 [B*T][dur_chans] scratch) and the frame layout
// every encode ends with (T_raw -> T_mel, the decode workspace, mel2word filled from `starts` or copied from mel2word, the encoded state)
int run_dur_predictor(dtts_ctx* h, const float* in, int cin, const int* ilens, float* d0, float* d1, float* dur, int B, int T, hipStream_t s);
int lay_out_frames(dtts_ctx* h, const int64_t* mel2word, int T_m2w, int T_raw, const int* starts, const int* ilens, int T_w, hipStream_t s,
                   int32_t* T_mel_host);
// fft_blocks.hip: a stack's weights from "<p>layers.<i>.op.*" (+ "<p>layer_norm.*", "<p>pos_embed_alpha"), and its launches
int build_fft_stack(dtts_ctx* h, Need& need, FftStack& S, const std::string& p, int layers, int C, int heads, bool* ok);
int run_fft_stack(dtts_ctx* h, const FftStack& S, const float* x_in, const int* lens_in, const float* pos_table, int n_pos, int B, int T, int C,
                  int heads, float* y, const FftBufs& w, hipStream_t s);
int gloss_forward(dtts_ctx* h, const dtts_gloss_args* a, hipStream_t stream);         // gloss.hip (the same)
int dict_edit_forward(dtts_ctx* h, const dtts_dict_edit_args* a, hipStream_t stream);    // dict_edit.hip (the same)
int dict_entry_forward(dtts_ctx* h, const dtts_dict_entry_args* a, hipStream_t stream);  // dict_edit.hip (the same; writes the block's out fields)

// ---- a row of the one table of parts and block items (UNITS, context.hip): dtts_finalize_weights walks its parts in row order,
// dtts_text2mel_fetch finds the item's forward in it, Block::finalized the part's ready predicate.  A row may be a part without an item
// (the acoustic model), an item without a part (the losses), or both
struct Unit {
    int part;                        // DTTS_PART_* bit, or 0: the item has no part of its own
    const char* part_name;           // "DTTS_PART_X"
    const char* prefix;              // the part owns the tensors named "<prefix>..." (the dot included)
    int (*build)(dtts_ctx*);
    bool once;                       // built once per context; false: rebuilt by every finalize that names it, from the tensors loaded last
    bool (*ready)(const dtts_ctx*);
    int out;                         // DTTS_OUT_* whose dst is this unit's argument block, or 0
    int (*forward)(dtts_ctx*, const void*, hipStream_t);
    bool null_handle;                // the forward checks its block before the handle, so it is reached with a null one too
};
const Unit* find_item(int what);   // the row whose argument block DTTS_OUT_<what> takes, or null

} // namespace dtts
