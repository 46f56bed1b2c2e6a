// libdicttts_hip.so — the acoustic model's passes: encode (dictionary encoder, duration predictor, length regulator), decode (prior flow
// in reverse, FVAE decoder), the teacher-forced posterior pass, the resident dictionary table.  Weights: text2mel_build.hip.
#include "ctx.h"

using namespace dtts;

namespace {

int run_encoder(dtts_ctx* h, const Encoder& E, float* x, float* hbuf, float* qkv, float* att, float* ff, float* out,
                const int* lens, int B, int T, hipStream_t s, const float* spk = nullptr) {
    const int C = h->cfg.hidden_size, F = 4 * C;
    for (size_t i = 0; i < E.l.size(); ++i) {
        const EncLayer& l = E.l[i];
        LAUNCH(layernorm_launch(x, hbuf, l.g1, l.b1, 1e-4f, lens, 1, 0, B, T, C, s));
        ConvParams p = base_params(hbuf, C, B, T, T, qkv, 3 * C);
        LAUNCH(conv1d_launch(l.qkv, p, s));
        LAUNCH(mha_launch(qkv, att, lens, B, T, C, h->cfg.num_heads, s));
        p = base_params(att, C, B, T, T, x, C);
        set_res(p, 0, x, C);
        LAUNCH(conv1d_launch(l.o, p, s));
        LAUNCH(layernorm_launch(x, hbuf, l.g2, l.b2, 1e-4f, lens, 0, 0, B, T, C, s));
        p = base_params(hbuf, C, B, T, T, ff, F);
        p.in_lens = lens;
        p.post_act = 1;
        LAUNCH(conv1d_launch(l.ffn1, p, s));
        p = base_params(ff, F, B, T, T, x, C);
        p.in_lens = lens;
        p.out_lens = lens;
        p.zero_masked = 1;
        set_res(p, 0, x, C);
        LAUNCH(conv1d_launch(l.ffn2, p, s));
    }
    LAUNCH(layernorm_launch(x, out, E.lg, E.lb, 1e-4f, lens, 0, 1, B, T, C, s, spk));   // spk: (LN + spk[b]) * nonpadding
    return DTTS_OK;
}

// WN.forward (modules/commons/wavenet.py:54-78): x is updated in place, `out` receives the skip sum
// g == null: `cond` already holds the conditioning (the caller computed it)
// mask == null: x_mask = 1 (inference).  Otherwise [B][T]: x = (x + res) * mask in every non-last layer and out = skip_sum * mask, both in the
// res / skip epilogue (x must arrive masked)
int run_wn(dtts_ctx* h, const WNet& W, float* x, const float* g, int g_ld, float* cond, float* acts, float* out, int B,
           int T, hipStream_t s, const int64_t* cond_m2w = nullptr, int cond_Tw = 0, const float* mask = nullptr) {
    const int H = W.hidden;
    ConvParams p;
    if (g) {
        p = base_params(g, g_ld, B, T, T, cond, 2 * H * W.layers);
        LAUNCH(conv1d_launch(W.cond, p, s));
    }
    for (int i = 0; i < W.layers; ++i) {
        if (W.in[i].engine == ENG_BF16X3) {   // split-operand WaveNet layer on the vconv kernel (vconv.hip: WaveNet epilogue)
            {   // acts = tanh(in(x) + cond_t) * sigmoid(in(x) + cond_s)
                VConvParams v = vparams_x3(W.in[i], x, H, 1.f, nullptr, B, T);
                v.bias = nullptr;
                v.gbias = W.in[i].bias;
                v.gate_H = H;
                v.cond = cond;
                v.ld_cond = 2 * H * W.layers;
                v.cond_coff = i * 2 * H;
                v.cond_m2w = (const long long*)cond_m2w;   // word-level conditioning gathered in the epilogue (decoder)
                v.cond_Tw = cond_Tw;
                v.yf = acts;
                v.ldyf = H;
                LAUNCH(vconv_launch(v, s));
            }
            {   // res / skip: x += rs[:H], out (+)= rs[H:]  (the last layer has the skip half only)
                VConvParams v = vparams_x3(W.rs[i], acts, H, 1.f, nullptr, B, T);
                v.bias = nullptr;
                v.gbias = W.rs[i].bias;
                v.row_mask = mask;   // the first segment: the res half, or the last layer's skip sum
                if (i < W.layers - 1) {
                    v.split = H;
                    v.yf = x;
                    v.ldyf = H;
                    v.res = x;
                    v.ldres = H;
                    v.yf2 = out;
                    v.ldyf2 = H;
                    if (i > 0) {
                        v.res_b = out;
                        v.ldres_b = H;
                    }
                } else {
                    v.split = 1 << 30;   // single segment through the same epilogue
                    v.yf = out;
                    v.ldyf = H;
                    if (i > 0) {
                        v.res = out;
                        v.ldres = H;
                    }
                }
                LAUNCH(vconv_launch(v, s));
            }
            continue;
        }
        p = base_params(x, H, B, T, T, acts, H);
        p.cond = cond;
        p.ld_cond = 2 * H * W.layers;
        p.cond_coff = i * 2 * H;
        LAUNCH(conv1d_launch(W.in[i], p, s));
        p = base_params(acts, H, B, T, T, x, H);
        p.row_mask = mask;   // seg[0]: the res half, or the last layer's skip sum
        if (i < W.layers - 1) {
            p.split = H;
            set_res(p, 0, x, H);
            p.seg[1].y = out;
            p.seg[1].ld = H;
            if (i > 0) set_res(p, 1, out, H);
        } else {
            p.seg[0].y = out;
            if (i > 0) set_res(p, 0, out, H);
        }
        LAUNCH(conv1d_launch(W.rs[i], p, s));
    }
    return DTTS_OK;
}

// g_sqz = g_pre_net(g) = Conv1d(k = 8, s = 4, p = 2): [B][T][C] -> [B][T / 4][C]
int run_g_sqz(dtts_ctx* h, const float* g, float* gs, int B, int T, hipStream_t s) {
    const int C = h->cfg.hidden_size, T4 = T / 4;
    if (h->g_pre_poly.w_hi) {
        VConvParams v = vparams_x3(h->g_pre_poly, g, 4 * C, 1.f, nullptr, B, T4);
        v.in_half = 1;
        v.yf = gs;
        v.ldyf = C;
        LAUNCH(vconv_launch(v, s));
    } else {
        ConvParams p = base_params(g, C, B, T, T4, gs, C);
        LAUNCH(conv1d_launch(h->g_pre, p, s));
    }
    return DTTS_OK;
}

// scratch of the prior flow, T / 4 rows: cond_all [fs_cond.C_out] for the one-kernel form; fcond, fh, facts, fout for launch by launch
struct FlowScratch { float *cond_all, *fcond, *fh, *facts, *fout; };

// The prior flow over `flows` (execution order), conditioned on gs: z_out = flow(z_in).  fs_w != null: every block in one kernel (flowstack.hip)
// on that pack, the conditioning of all blocks by one convolution (fs_cond).  Otherwise launch by launch (DTTS_TUNE bit 8, or a flow shape the
// fused kernel does not take), in place on z_out: z_in is copied there first when they differ.  mask: null (the reverse flow of inference) or
// the squeezed frame mask [B][T4] of the masked forward flow (glow_modules.py:108-123,157-161)
int run_prior_flow(dtts_ctx* h, const std::vector<Flow>& flows, const float* fs_w, const PackedConv& fs_cond, const float* gs, const float* z_in,
                   float* z_out, const float* mask, const FlowScratch& w, int B, int T4, hipStream_t s) {
    const dtts_config& c = h->cfg;
    const int C = c.hidden_size, Z = c.latent_size, Hf = c.prior_glow_hidden;
    if (fs_w) {
        const int n_c = fs_cond.C_out;
        if (fs_cond.engine == ENG_BF16X3) {
            VConvParams v = vparams_x3(fs_cond, gs, C, 1.f, nullptr, B, T4);
            v.yf = w.cond_all;
            v.ldyf = n_c;
            LAUNCH(vconv_launch(v, s));
        } else {
            ConvParams p = base_params(gs, C, B, T4, T4, w.cond_all, n_c);
            LAUNCH(conv1d_launch(fs_cond, p, s));
        }
        FlowStackParams fp;
        memset(&fp, 0, sizeof fp);
        fp.z_in = z_in;
        fp.z_out = z_out;
        fp.cond = w.cond_all;
        fp.ld_cond = n_c;
        fp.w = fs_w;
        fp.B = B;
        fp.T4 = T4;
        fp.Z = Z;
        fp.n_flows = (int)flows.size();
        fp.layers = c.prior_glow_n_layers;
        fp.x3 = c.decoder_fp32 ? 0 : 1;   // split-bf16 like the decoder WaveNet unless the exact-fp32 decoder was asked for
        for (size_t i = 0; i < flows.size(); ++i) {
            fp.in_coff[i] = flows[i].in_coff;
            fp.out_coff[i] = flows[i].out_coff;
        }
        fp.mask = mask;
        LAUNCH(flowstack_launch(fp, s));
        return DTTS_OK;
    }
    if (z_out != z_in) HIPCHK(hipMemcpyAsync(z_out, z_in, (size_t)B * T4 * Z * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (const Flow& fl : flows) {
        ConvParams p = base_params(z_out, Z, B, T4, T4, w.fh, Hf);
        p.x_coff = fl.in_coff;
        p.row_mask = mask;   // h = pre(x0) * x_mask
        LAUNCH(conv1d_launch(fl.pre, p, s));
        int rc = run_wn(h, fl.wn, w.fh, gs, C, w.fcond, w.facts, w.fout, B, T4, s, nullptr, 0, mask);
        if (rc) return rc;
        p = base_params(w.fout, Hf, B, T4, T4, z_out, Z);
        p.seg[0].coff = fl.out_coff;
        set_res(p, 0, z_out, Z);
        p.seg[0].coff_res = fl.out_coff;
        p.row_mask = mask;   // x1 = post(h) * mask + x1 * mask
        LAUNCH(conv1d_launch(fl.post, p, s));
    }
    return DTTS_OK;
}

// The FVAE decoder behind its pre_net: dx [B][T][Hd] (the WaveNet updates it in place) -> mel_out [B][mel_cap ? mel_cap : T][n_mel].  mask: null,
// or the frame mask [B][T] of the teacher-forced pass (dx arrives masked).  cond_w: [B * T_w + 1][CW]; dcond, where needed, comes from A.
// The decoder's conditioning is a 1x1 convolution of g, and g[b,t] is just word row mel2word[b,t] of the encoder
// output (or the zero row): the convolution is applied to the B*T_w word rows (33x fewer than the B*T frames) and its
// output gathered by mel2word; frames with mel2word == 0 get conv(0) = bias.  Bit-identical: every output row of this
// kernel depends only on its own input row, summed in the same order whatever the tile shape.
// dense_g != null (the PortaSpeech baseline): g is a dense per-frame tensor [B][T][C], no gather of word rows: the conditioning is the same
// convolution applied to the B*T frames (run_wn's dense-g branch) and every layer reads its own row of it.
int run_decoder_tail(dtts_ctx* h, Arena& A, const char* ws_name, float* cond_w, float* dx, float* dacts, float* dout, const float* mask,
                     float* mel_out, int mel_cap, hipStream_t s, const float* dense_g = nullptr) {
    const dtts_config& c = h->cfg;
    const int B = h->B, T = h->T_mel, C = c.hidden_size, Hd = c.fvae_enc_dec_hidden, CW = 2 * Hd * c.fvae_dec_n_layers;
    int rc;
    ConvParams p;
    if (dense_g) {
        float* dcond = A.alloc<float>((size_t)B * T * CW);
        if (!dcond) return fail(h, DTTS_E_NOMEM, "%s", ws_name);
        rc = run_wn(h, h->dec_wn, dx, dense_g, C, dcond, dacts, dout, B, T, s, nullptr, 0, mask);
    } else {
        // row 0: conv(0) = the bias, rows 1..: the B*T_w word rows
        if (hipMemcpyAsync(cond_w, h->dec_wn.cond.bias, (size_t)CW * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
            return fail(h, DTTS_E_HIP, "decoder conditioning bias row");
        p = base_params(h->weo, C, B, h->T_w, h->T_w, cond_w + CW, CW);
        LAUNCH(conv1d_launch(h->dec_wn.cond, p, s));
        if (!h->dec_wn.in.empty() && h->dec_wn.in[0].engine == ENG_BF16X3) {
            // split-operand layers: every layer's epilogue gathers its conditioning row by mel2word from the word-level tensor (L2-resident,
            // B*T_w rows) — the [B*T, 2*Hd*layers] expansion (221 MB written and read back at B=60) never exists
            rc = run_wn(h, h->dec_wn, dx, nullptr, C, cond_w, dacts, dout, B, T, s, h->m2w, h->T_w, mask);
        } else {
            float* dcond = A.alloc<float>((size_t)B * T * CW);
            if (!dcond) return fail(h, DTTS_E_NOMEM, "%s", ws_name);
            LAUNCH(expand_launch(cond_w + CW, h->m2w, dcond, nullptr, B, h->T_w, T, CW, s, h->dec_wn.cond.bias));
            rc = run_wn(h, h->dec_wn, dx, nullptr, C, dcond, dacts, dout, B, T, s, nullptr, 0, mask);
        }
    }
    if (rc) return rc;
    p = base_params(dout, Hd, B, T, T, mel_out, c.audio_num_mel_bins);
    if (mel_cap) {
        if (mel_cap < T) return fail(h, DTTS_E_INVAL, "mel_out holds %d frames per utterance, T_mel = %d", mel_cap, T);
        p.y_bstride_rows = mel_cap;   // only this layer's output lives in the caller's capacity layout
    }
    LAUNCH(conv1d_launch(h->dec_out, p, s));
    return DTTS_OK;
}

} // namespace

namespace dtts {

// DurationPredictor.forward (modules/portaspeech/model.py:58-66) on in [B][T][cin]; ilens: the rows that are no padding
int run_dur_predictor(dtts_ctx* h, const float* in, int cin, const int* ilens, float* d0, float* d1, float* dur, int B, int T, hipStream_t s) {
    const dtts_config& c = h->cfg;
    for (int i = 0; i < c.dur_predictor_layers; ++i) {
        ConvParams p = base_params(in, cin, B, T, T, d0, c.dur_chans);
        p.post_act = 1;
        LAUNCH(conv1d_launch(h->dur_conv[i], p, s));
        LAUNCH(layernorm_launch(d0, d1, h->dur_g[i], h->dur_b[i], 1e-5f, ilens, 0, 1, B, T, c.dur_chans, s));
        in = d1;  // next conv reads d1 and writes d0 again
        cin = c.dur_chans;
    }
    LAUNCH(dur_head_launch(in, h->dur_w, h->dur_bias, ilens, dur, B, T, c.dur_chans, s));
    return DTTS_OK;
}

// What every encode ends with: T_raw -> T_mel, the decode workspace with mel2word and x_mask first, mel2word from the durations' `starts`
// (mel2word == null) or copied, the encoded state
int lay_out_frames(dtts_ctx* h, const int64_t* mel2word, int T_m2w, int T_raw, const int* starts, const int* ilens, int T_w, hipStream_t s,
                   int32_t* T_mel_host) {
    const dtts_config& c = h->cfg;
    const int B = h->B, C = c.hidden_size;
    const int fm = c.frames_multiple;
    const int T_mel = (T_raw % fm) ? T_raw + fm - T_raw % fm : T_raw;
    const int T4 = T_mel / 4;
    const size_t mrows = (size_t)B * T_mel, qrows = (size_t)B * T4;
    const int Hd = c.fvae_enc_dec_hidden, Hf = c.prior_glow_hidden;
    HIPCHK(h->a_dec.reserve(mrows * (size_t)(C + 1 + 2 + 2 * Hd * c.fvae_dec_n_layers + 3 * Hd + 8) * sizeof(float) +
                            qrows * (size_t)(C + 2 * c.latent_size + 2 * Hf * c.prior_glow_n_layers * (1 + c.prior_glow_n_blocks) + 3 * Hf + 16) * sizeof(float) +
                            (size_t)B * T_w * 2 * Hd * c.fvae_dec_n_layers * sizeof(float) + (64 << 10), s));
    h->m2w = h->a_dec.alloc<int64_t>(mrows);
    h->x_mask = h->a_dec.alloc<float>(mrows);
    if (!h->m2w || !h->x_mask) return fail(h, DTTS_E_NOMEM, "decoder workspace");
    if (!mel2word) LAUNCH(mel2word_fill_launch(starts, h->mel_lens, ilens, h->m2w, B, T_w, T_raw, T_mel, s));
    else LAUNCH(mel2word_copy_launch(mel2word, h->m2w, h->mel_lens, B, T_m2w, T_mel, s));
    h->T_mel = T_mel;
    *T_mel_host = T_mel;
    h->encoded = true;
    return DTTS_OK;
}

} // namespace dtts

extern "C" {

static int encode_impl(dtts_handle h, const int64_t* word_tokens, const float* keys, const float* values,
                       const float* key_map, const int64_t* pinyin, const int64_t* pinyin_map, const int32_t* entry_ids,
                       const int64_t* pron_modified, const int64_t* mel2word, int T_m2w, int B, int T_w, int L_k, int P,
                       int32_t* T_mel_host, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    // an armed speaker batch belongs to THIS encode whatever its outcome: a later batch never reuses it
    const int spk_B = h->spk_armed_B;
    h->spk_armed_B = 0;
    h->enc_spk = false;
    if (!h->acoustic_ready) return fail(h, DTTS_E_STATE, "acoustic weights not finalized");
    const bool tensors_ok = keys && values && key_map && pinyin && pinyin_map;
    if (!word_tokens || (!entry_ids && !tensors_ok) || !T_mel_host || B <= 0 || T_w <= 0 || L_k <= 0 || P <= 0 || L_k > 1024 ||
        P > 64)
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_encode: bad argument (B=%d T_w=%d L_k=%d P=%d)", B, T_w, L_k, P);
    if (entry_ids && !h->t_entries) return fail(h, DTTS_E_STATE, "dtts_text2mel_encode_ids before dtts_dict_table_upload");
    if (spk_B && spk_B != B)
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_speakers armed %d utterances but this encode has B=%d (the speakers are dropped; arm again)",
                    spk_B, B);
    const float* spk = spk_B ? h->spk_rows : nullptr;
    hipStream_t s = (hipStream_t)stream;
    const dtts_config& c = h->cfg;
    const int C = c.hidden_size, D = c.gloss_dim, F = 4 * C;
    const size_t rows = (size_t)B * T_w;
    h->encoded = false;
    h->ps_encoded = false;
    HIPCHK(h->a_enc.reserve(rows * (size_t)(12 * C + 3 * C + F + 2 * D + 3 * c.dur_chans + P + 8) * sizeof(float) +
                            (size_t)B * L_k * T_w * sizeof(float) + (size_t)B * (T_w + 8) * 4 * sizeof(int) + (64 << 10), s));
    Arena& A = h->a_enc;
    float* x = A.alloc<float>(rows * C);
    float* hb = A.alloc<float>(rows * C);
    float* qkv = A.alloc<float>(rows * 3 * C);
    float* att = A.alloc<float>(rows * C);
    float* ff = A.alloc<float>(rows * F);
    float* enc1 = A.alloc<float>(rows * C);
    float* q = A.alloc<float>(rows * C);
    float* qk = A.alloc<float>(rows * D);
    float* wv = A.alloc<float>(rows * D);
    float* v = A.alloc<float>(rows * C);
    float* pron = A.alloc<float>(rows * C);
    h->context = A.alloc<float>(rows * C);
    h->weo = A.alloc<float>(rows * C);
    h->dur = A.alloc<float>(rows);
    h->pron_attn = A.alloc<float>(rows * P);
    h->dict_attn = A.alloc<float>((size_t)B * L_k * T_w);
    float* d0 = A.alloc<float>(rows * c.dur_chans);
    float* d1 = A.alloc<float>(rows * c.dur_chans);
    h->lens = A.alloc<int>(B);
    int* ilens = A.alloc<int>(B);
    int* starts = A.alloc<int>((size_t)B * (T_w + 1));
    h->mel_lens = A.alloc<int>(B);
    int* pm_max = A.alloc<int>(3);   // [0] largest sense index; id path: [1] / [2] rows / slots of the longest entry
    if (!x || !hb || !qkv || !att || !ff || !enc1 || !q || !qk || !wv || !v || !pron || !h->context || !h->weo || !h->dur ||
        !h->pron_attn || !h->dict_attn || !d0 || !d1 || !h->lens || !ilens || !starts || !h->mel_lens || !pm_max)
        return fail(h, DTTS_E_NOMEM, "encoder workspace");
    h->B = B;
    h->T_w = T_w;
    h->L_k = L_k;
    h->P = P;
    // stage spans under the reference's profile_infer names (modules/dict_tts/model.py:50,86): 'encoder' = this whole call's
    // device work (dictionary encoder, duration predictor, length regulator; the gather-expand runs in decode here),
    // 'dict_encoder' = embedding + both relative-position encoders + S2PA
    Timed t_encoder(h, DTTS_TIMER_STAGE_ENCODER, s);
    Timed t_dict(h, DTTS_TIMER_STAGE_DICT_ENCODER, s);
    // A1: embedding * sqrt(hidden), lengths
    LAUNCH(embed_launch(word_tokens, h->word_emb, sqrtf((float)C), x, h->lens, B, T_w, C, c.word_size, s));
    // A2: semantic encoder
    int rc = run_encoder(h, h->sem, x, hb, qkv, att, ff, enc1, h->lens, B, T_w, s);
    if (rc) return rc;
    // A3: S2PA
    {
        ConvParams p = base_params(enc1, C, B, T_w, T_w, q, C);
        p.out_mul = (float)std::pow((double)D, -0.5);  // q * key_depth_per_head ** -0.5 (dict_encoder.py:45-46)
        LAUNCH(conv1d_launch(h->s2_q, p, s));
        const bool projected = entry_ids != nullptr;   // resident table of projected rows: logits = K . q, context = Wo sum_l w_l V_l
        if (!projected) {
            p = base_params(q, C, B, T_w, T_w, qk, D);
            LAUNCH(conv1d_launch(h->s2_kT, p, s));
        }
        if (entry_ids) LAUNCH(max_entry_pm_launch(entry_ids, h->t_pmmax, h->t_off, h->t_poff, (long long)rows, pm_max, s));
        else LAUNCH(max_i64_launch(pinyin_map, (long long)rows * P, pm_max, s));
        S2paArgs a;
        memset(&a, 0, sizeof a);
        a.entry = entry_ids;
        a.t_off = h->t_off;
        a.t_keys = h->t_keys;
        a.t_values = h->t_values;
        a.t_key_map = h->t_key_map;
        a.t_poff = h->t_poff;
        a.t_pinyin = h->t_pinyin;
        a.t_pinyin_map = h->t_pinyin_map;
        a.qk = projected ? q : qk;
        a.keys = keys;
        a.values = values;
        a.key_map = key_map;
        a.pinyin = pinyin;
        a.pinyin_map = pinyin_map;
        a.pron_modified = pron_modified;
        a.pinyin_emb = h->pinyin_emb;
        a.pm_max = pm_max;
        a.lens = h->lens;
        a.wv = projected ? v : wv;
        a.dict_attn = h->dict_attn;
        a.pron_attn = h->pron_attn;
        a.pron = pron;
        a.B = B;
        a.T_w = T_w;
        a.L_k = L_k;
        a.P = P;
        a.D = projected ? C : D;
        a.H = C;
        a.n_pinyin = c.value_embedding_size;
        a.language_zh = c.language_zh;
        {
            Timed tm(h, DTTS_TIMER_S2PA, s);
            LAUNCH(s2pa_launch(a, s));
        }
        if (!projected) {
            p = base_params(wv, D, B, T_w, T_w, v, C);
            LAUNCH(conv1d_launch(h->s2_v, p, s));
        }
        p = base_params(v, C, B, T_w, T_w, h->context, C);
        p.out_lens = h->lens;
        p.zero_masked = 1;  // context * x_mask (dict_encoder.py:140)
        LAUNCH(conv1d_launch(h->s2_o, p, s));
        LAUNCH(add_launch(h->context, pron, x, (long long)rows * C, s));
    }
    // A4: linguistic encoder; * (word_tokens > 0) is the same prefix mask
    rc = run_encoder(h, h->lin, x, hb, qkv, att, ff, h->weo, h->lens, B, T_w, s, spk);   // + spk_embed, * nonpadding (model.py:94-96)
    if (rc) return rc;
    t_dict.stop();
    // A5: duration predictor
    LAUNCH(rowcount_nonzero_launch(h->weo, ilens, B, T_w, C, s));
    rc = run_dur_predictor(h, h->weo, C, ilens, d0, d1, h->dur, B, T_w, s);
    if (rc) return rc;
    // A6/A7: durations -> mel2word
    int T_raw = 0;
    if (!mel2word) {
        LAUNCH(durations_launch(h->dur, ilens, starts, h->mel_lens, B, T_w, s));
        std::vector<int> tot(B);
        int pm_host3[3] = {0, 0, 0};
        int& pm_host = pm_host3[0];
        unsigned long long spk_bad[2] = {0ull, 0ull};
        HIPCHK(hipMemcpyAsync(tot.data(), h->mel_lens, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pm_host3, pm_max, sizeof(int) * (entry_ids ? 3 : 1), hipMemcpyDeviceToHost, s));
        if (spk) HIPCHK(hipMemcpyAsync(spk_bad, h->spk_flag, sizeof spk_bad, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));  // the one host sync of the path: T_mel sizes every later buffer
        if (pm_host > DTTS_MAX_SENSES)   // the S2PA kernel keeps DTTS_MAX_SENSES sense slots; larger indices would silently get weight 0
            return fail(h, DTTS_E_INVAL, "pinyin_map holds sense index %d; at most %d senses per word are supported", pm_host, DTTS_MAX_SENSES);
        if (pm_host3[1] > L_k || pm_host3[2] > P)   // s2pa_row clamps an entry to L_k rows / P slots: the rest would be dropped silently
            return fail(h, DTTS_E_INVAL, "dtts_text2mel_encode_ids: the batch holds a table entry of %d gloss rows and one of %d pinyin slots; L_k=%d P=%d must be the batch maxima",
                        pm_host3[1], pm_host3[2], L_k, P);
        if (spk_bad[0])   // nn.Embedding raises on such an id; the gather wrote a zero row instead of reading out of range
            return fail(h, DTTS_E_INVAL, "speaker id %lld of utterance %llu is out of range: spk_embed_proj has %d rows (num_spk)",
                        (long long)spk_bad[1], spk_bad[0] - 1, h->spk_n);
        for (int b = 0; b < B; ++b) T_raw = std::max(T_raw, tot[b]);
    } else {
        if (T_m2w <= 0) return fail(h, DTTS_E_INVAL, "mel2word given with T_m2w=%d", T_m2w);
        T_raw = T_m2w;
    }
    rc = lay_out_frames(h, mel2word, T_m2w, T_raw, starts, ilens, T_w, s, T_mel_host);
    if (rc) return rc;
    h->enc_spk = spk != nullptr;
    h->enc_spk_gen = h->spk_gen;
    return DTTS_OK;
}

int dtts_text2mel_speakers(dtts_handle h, int kind, const void* spk, int B, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    h->spk_armed_B = 0;
    if (!h->acoustic_ready) return fail(h, DTTS_E_STATE, "dtts_text2mel_speakers: acoustic weights not finalized");
    if (!h->spk_kind)
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_speakers: no speaker weights loaded (spk_embed_proj.* exists only in checkpoints trained with "
                    "use_spk_embed / use_spk_id and num_spk > 1)");
    if (kind != h->spk_kind)
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_speakers: kind %d does not match the loaded spk_embed_proj (%s: kind %d)", kind,
                    h->spk_kind == DTTS_SPK_EMBED ? "nn.Linear(256, hidden), use_spk_embed" : "Embedding(num_spk, hidden), use_spk_id", h->spk_kind);
    if (!spk || B <= 0 || B > DTTS_MAX_SPEAKER_BATCH)
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_speakers: bad argument (B=%d, at most %d)", B, DTTS_MAX_SPEAKER_BATCH);
    hipStream_t s = (hipStream_t)stream;
    const int C = h->cfg.hidden_size;
    HIPCHK(h->a_spk.reserve((size_t)DTTS_MAX_SPEAKER_BATCH * C * sizeof(float) + (64 << 10), s));   // fixed capacity: allocated once
    h->spk_rows = h->a_spk.alloc<float>((size_t)B * C);
    h->spk_flag = h->a_spk.alloc<unsigned long long>(2);
    if (!h->spk_rows || !h->spk_flag) return fail(h, DTTS_E_NOMEM, "speaker workspace");
    h->spk_gen += 1;
    if (kind == DTTS_SPK_EMBED) LAUNCH(spk_linear_launch(h->spk_w, h->spk_bias, (const float*)spk, h->spk_rows, B, C, h->spk_flag, s));
    else LAUNCH(spk_gather_launch(h->spk_w, h->spk_n, (const int64_t*)spk, h->spk_rows, B, C, h->spk_flag, s));
    h->spk_armed_B = B;
    return DTTS_OK;
}

int dtts_text2mel_encode(dtts_handle h, const int64_t* word_tokens, const float* keys, const float* values,
                         const float* key_map, const int64_t* pinyin, const int64_t* pinyin_map,
                         const int64_t* pron_modified, const int64_t* mel2word, int T_m2w, int B, int T_w, int L_k, int P,
                         int32_t* T_mel_host, dtts_stream stream) {
    if (h && !(keys && values && key_map && pinyin && pinyin_map))
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_encode: null dictionary tensor");
    return encode_impl(h, word_tokens, keys, values, key_map, pinyin, pinyin_map, nullptr, pron_modified, mel2word, T_m2w, B, T_w,
                       L_k, P, T_mel_host, stream);
}

int dtts_text2mel_encode_ids(dtts_handle h, const int64_t* word_tokens, const int32_t* entry_ids, const int64_t* pron_modified,
                             const int64_t* mel2word, int T_m2w, int B, int T_w, int L_k, int P, int32_t* T_mel_host,
                             dtts_stream stream) {
    if (h && !entry_ids) return fail(h, DTTS_E_INVAL, "dtts_text2mel_encode_ids: null entry ids");
    return encode_impl(h, word_tokens, nullptr, nullptr, nullptr, nullptr, nullptr, entry_ids, pron_modified, mel2word, T_m2w, B,
                       T_w, L_k, P, T_mel_host, stream);
}

int dtts_dict_table_upload(dtts_handle h, int n_entries, const int32_t* tok_off, const float* keys, const float* values,
                           const float* key_map, const int32_t* pin_off, const int64_t* pinyin, const int64_t* pinyin_map) {
    if (!h || n_entries <= 0 || !tok_off || !keys || !key_map || !pin_off || !pinyin || !pinyin_map)
        return fail(h, DTTS_E_INVAL, "dtts_dict_table_upload: bad argument");
    const int D = h->cfg.gloss_dim;
    const size_t nL = (size_t)tok_off[n_entries], nP = (size_t)pin_off[n_entries];
    for (int e = 0; e < n_entries; ++e)
        if (tok_off[e + 1] < tok_off[e] || pin_off[e + 1] < pin_off[e])
            return fail(h, DTTS_E_INVAL, "dtts_dict_table_upload: offsets must be non-decreasing (entry %d)", e);
    std::vector<int> pmmax(n_entries, 0);
    for (int e = 0; e < n_entries; ++e) {
        for (int p = pin_off[e]; p < pin_off[e + 1]; ++p) pmmax[e] = std::max(pmmax[e], (int)pinyin_map[p]);
        float km = 0.f;
        for (int l = tok_off[e]; l < tok_off[e + 1]; ++l) km = std::max(km, key_map[l]);
        if (pmmax[e] > DTTS_MAX_SENSES || km > (float)DTTS_MAX_SENSES)
            return fail(h, DTTS_E_INVAL, "dtts_dict_table_upload: entry %d has sense index %d; at most %d senses per word are supported",
                        e, std::max(pmmax[e], (int)km), DTTS_MAX_SENSES);
    }
    // ---- build the NEW table completely before touching the one in use: a failed re-upload leaves the previous table working
    int dev_cur = -1;
    (void)hipGetDevice(&dev_cur);
    if (dev_cur != h->device)
        return fail(h, DTTS_E_STATE, "dtts_dict_table_upload: the current HIP device is %d, the context was created on device %d", dev_cur, h->device);
    std::vector<void*> fresh;   // the new table's allocations (released again if anything below fails)
    const char* what = nullptr;
    hipError_t herr = hipSuccess;
    auto up = [&](const void* src, size_t bytes) -> void* {
        void* d = dev_alloc(h, bytes);
        if (!d) {
            what = "device allocation";
            return nullptr;
        }
        fresh.push_back(d);
        if (bytes && (herr = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice)) != hipSuccess) {
            what = "host-to-device copy";
            return nullptr;
        }
        return d;
    };
    // SURVEY 8d "resident-table path": the table holds the PROJECTED rows K = k_transform(key), V = v_transform(value)
    // (dict_encoder.py:36-39: the reference projects every gloss row of every batch; here once, at upload) — 2 x hidden_size floats per
    // row instead of 768 (+ 768), and the logit becomes k . q in the reference's own association order.
    if (!h->acoustic_ready)
        return fail(h, DTTS_E_STATE, "dtts_dict_table_upload: the acoustic weights must be finalized first (the table stores k_transform / v_transform projections)");
    if (nL > (size_t)INT_MAX / 2) return fail(h, DTTS_E_INVAL, "dtts_dict_table_upload: %zu gloss rows", nL);
    int* n_off = (int*)up(tok_off, sizeof(int) * (n_entries + 1));
    int* n_poff = (int*)up(pin_off, sizeof(int) * (n_entries + 1));
    int* n_pmmax = (int*)up(pmmax.data(), sizeof(int) * n_entries);
    float *n_keys = nullptr, *n_values = nullptr;
    const int C = h->cfg.hidden_size;
    float* raw = nullptr;
    hipStream_t ps = nullptr;   // the projection runs on its own stream, on the device that is current now (= the context's: its weights live there)
    if (!what && (herr = hipMalloc((void**)&raw, std::max<size_t>(nL * D * sizeof(float), 16))) != hipSuccess) what = "staging buffer allocation";
    if (!what && (herr = hipStreamCreate(&ps)) != hipSuccess) what = "hipStreamCreate";
    auto proj = [&](const float* src, const PackedConv& L) -> float* {   // [nL][D] host rows -> [nL][C] device rows
        if (what) return nullptr;
        float* out = (float*)dev_alloc(h, nL * C * sizeof(float));
        if (!out) {
            what = "device allocation";
            return nullptr;
        }
        fresh.push_back(out);
        if (nL == 0) return out;
        if ((herr = hipMemcpyAsync(raw, src, nL * D * sizeof(float), hipMemcpyHostToDevice, ps)) != hipSuccess) {
            what = "host-to-device copy";
            return nullptr;
        }
        ConvParams p = base_params(raw, D, 1, (int)nL, (int)nL, out, C);
        if ((herr = conv1d_launch(L, p, ps)) != hipSuccess) {
            what = "projection kernel launch";
            return nullptr;
        }
        if ((herr = hipStreamSynchronize(ps)) != hipSuccess) {
            what = "projection kernel";
            return nullptr;
        }
        return out;
    };
    n_keys = proj(keys, h->s2_k);
    n_values = proj(values ? values : keys, h->s2_v);
    if (ps) (void)hipStreamDestroy(ps);
    if (raw) (void)hipFree(raw);
    float* n_key_map = (float*)up(key_map, nL * sizeof(float));
    int64_t* n_pinyin = (int64_t*)up(pinyin, nP * sizeof(int64_t));
    int64_t* n_pinyin_map = (int64_t*)up(pinyin_map, nP * sizeof(int64_t));
    if (what || !n_off || !n_poff || !n_pmmax || !n_keys || !n_values || !n_key_map || !n_pinyin || !n_pinyin_map) {
        for (void* q : fresh) dev_free(h, q);
        return fail(h, what && strstr(what, "allocation") ? DTTS_E_NOMEM : DTTS_E_HIP, "dtts_dict_table_upload: %s failed (%s)%s",
                    what ? what : "device allocation", hipGetErrorString(herr), h->t_entries ? "; the previous table stays in use" : "");
    }
    if (h->t_entries) {   // a second upload replaces the table: release the previous one (nothing may still be using it)
        if ((herr = hipDeviceSynchronize()) != hipSuccess) {   // (the new table is released again; the previous one stays in use)
            for (void* q : fresh) dev_free(h, q);
            return fail(h, DTTS_E_HIP, "dtts_dict_table_upload: hipDeviceSynchronize failed (%s); the previous table stays in use", hipGetErrorString(herr));
        }
        void* old[] = {h->t_off, h->t_poff, h->t_pmmax, h->t_keys, h->t_values != h->t_keys ? h->t_values : nullptr, h->t_key_map, h->t_pinyin, h->t_pinyin_map};
        for (void* q : old) dev_free(h, q);
    }
    h->t_off = n_off;
    h->t_poff = n_poff;
    h->t_pmmax = n_pmmax;
    h->t_keys = n_keys;
    h->t_values = n_values;
    h->t_key_map = n_key_map;
    h->t_pinyin = n_pinyin;
    h->t_pinyin_map = n_pinyin_map;
    h->t_entries = n_entries;
    h->m_off.assign(tok_off, tok_off + n_entries + 1);   // the host mirrors an edit starts from (dict_edit.hip)
    h->m_poff.assign(pin_off, pin_off + n_entries + 1);
    h->m_pmmax = std::move(pmmax);
    return DTTS_OK;
}

// z_p: [B][latent][z_ld] (z_ld >= T_mel/4; 0 = exactly T_mel/4) or null = drawn on the device; mel_out: [B][mel_cap][n_mel]
// (mel_cap >= T_mel; 0 = exactly T_mel), rows >= T_mel are left untouched
static int decode_impl(dtts_handle h, const float* z_p, int z_ld, float* mel_out, int mel_cap, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    if (!h->encoded) return fail(h, DTTS_E_STATE, "dtts_text2mel_decode called before a successful dtts_text2mel_encode");
    if (!mel_out) return fail(h, DTTS_E_INVAL, "dtts_text2mel_decode: null argument");
    hipStream_t s = (hipStream_t)stream;
    const dtts_config& c = h->cfg;
    const int B = h->B, T = h->T_mel, T4 = T / 4, C = c.hidden_size, Z = c.latent_size;
    const int Hd = c.fvae_enc_dec_hidden, Hf = c.prior_glow_hidden;
    const size_t mrows = (size_t)B * T, qrows = (size_t)B * T4;
    Timed t_fvae(h, DTTS_TIMER_STAGE_FVAE, s);   // 'fvae' (model.py:57) + the gather-expand of run_text_encoder
    Arena& A = h->a_dec;
    // (m2w and x_mask were allocated first by encode; everything below is re-allocated after them on every call)
    A.rewind();
    (void)A.alloc<int64_t>(mrows);
    (void)A.alloc<float>(mrows);
    float* g = h->ps_encoded ? h->ps_g : A.alloc<float>(mrows * C);   // (the baseline's encode left its dense condition and x_mask behind)
    float* gs = A.alloc<float>(qrows * C);
    float* z = A.alloc<float>(qrows * Z);
    float* fcond = A.alloc<float>(qrows * 2 * Hf * c.prior_glow_n_layers);
    float* fh = A.alloc<float>(qrows * Hf);
    float* facts = A.alloc<float>(qrows * Hf);
    float* fout = A.alloc<float>(qrows * Hf);
    float* dx = A.alloc<float>(mrows * Hd);
    float* dacts = A.alloc<float>(mrows * Hd);
    float* dout = A.alloc<float>(mrows * Hd);
    if (!g || !gs || !z || !fcond || !fh || !facts || !fout || !dx || !dacts || !dout)
        return fail(h, DTTS_E_NOMEM, "decoder workspace");
    // A7: gather-expand (x * tgt_nonpadding is implied: padded frames gather the zero row)
    if (!h->ps_encoded) LAUNCH(expand_launch(h->weo, h->m2w, g, h->x_mask, B, h->T_w, T, C, s));
    // A8: g_sqz = Conv1d(k=8, s=4, p=2)(g)
    int rc = run_g_sqz(h, g, gs, B, T, s);
    if (rc) return rc;
    if (z_p) {
        if (z_ld && z_ld < T4) return fail(h, DTTS_E_INVAL, "prior sample holds %d steps per row, T_mel/4 = %d", z_ld, T4);
        LAUNCH(transpose_cf_to_cl_launch(z_p, z, B, Z, T4, s, z_ld));
    } else {
        LAUNCH(normal_fill_launch(z, (long long)qrows * Z, h->noise_seed + ++h->noise_counter, s));   // z_p ~ N(0,1) (fvae_semantics.py:110-111)
    }
    // A9: prior flow, reverse, no mask; the one-kernel form writes to a second latent buffer
    FlowScratch fw = {nullptr, fcond, fh, facts, fout};
    float* zf = z;
    if (h->fs_w) {
        fw.cond_all = A.alloc<float>(qrows * h->fs_cond.C_out);
        zf = A.alloc<float>(qrows * Z);
        if (!fw.cond_all || !zf) return fail(h, DTTS_E_NOMEM, "decoder workspace");
    }
    rc = run_prior_flow(h, h->flows, h->fs_w, h->fs_cond, gs, z, zf, nullptr, fw, B, T4, s);
    if (rc) return rc;
    // A10: decoder
    ConvParams p = base_params(zf, Z, B, T4, T4, dx, 4 * Hd);  // ConvTranspose1d(k=4,s=4): [B,T4,16] -> [B,T4,4*Hd] == [B,T,Hd]
    LAUNCH(conv1d_launch(h->dec_pre, p, s));
    float* cond_w = h->ps_encoded ? nullptr : A.alloc<float>(((size_t)B * h->T_w + 1) * 2 * Hd * c.fvae_dec_n_layers);   // (word rows: unused with a dense g)
    if (!cond_w && !h->ps_encoded) return fail(h, DTTS_E_NOMEM, "decoder workspace");
    return run_decoder_tail(h, A, "decoder workspace", cond_w, dx, dacts, dout, nullptr, mel_out, mel_cap, s, h->ps_encoded ? g : nullptr);
}

int dtts_text2mel_decode(dtts_handle h, const float* z_p, float* mel_out, dtts_stream stream) {
    return decode_impl(h, z_p, 0, mel_out, 0, stream);   // z_p == NULL: the prior sample is drawn on the device
}

// The FVAE posterior pass, teacher-forced (FVAE_semantics.forward(infer=False), modules/dict_tts/fvae_semantics.py:84-108), on the batch the
// last encode laid out; reached through dtts_text2mel_fetch(DTTS_OUT_POSTERIOR).  Its own workspace (a_post): the infer path's buffers and results are untouched.
// (dtts_text2mel_fetch(DTTS_OUT_POSTERIOR): the argument block has been checked by the caller)
static int posterior_impl(dtts_handle h, const float* tgt_mels, int mel_ld, const float* eps, int eps_ld, float* mel_out, int mel_cap,
                          float* m_q, float* logs_q, float* z_p, float* kl, dtts_stream stream) {
    if (!h->post_ready && !h->post_unsupported.empty())
        return fail(h, DTTS_E_INVAL, "dtts_text2mel_fetch(DTTS_OUT_POSTERIOR): %s", h->post_unsupported.c_str());
    if (!h->post_ready)
        return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch(DTTS_OUT_POSTERIOR): the checkpoint lacks the posterior encoder (missing weight "
                    "tensor '%s')", h->post_missing.empty() ? "model.fvae.encoder.pre_net.0.weight" : h->post_missing.c_str());
    if (!tgt_mels || !mel_out) return fail(h, DTTS_E_INVAL, "dtts_text2mel_fetch(DTTS_OUT_POSTERIOR): null tgt_mels / mel_out");
    hipStream_t s = (hipStream_t)stream;
    const dtts_config& c = h->cfg;
    const int B = h->B, T = h->T_mel, T4 = T / 4, C = c.hidden_size, Z = c.latent_size, n_mel = c.audio_num_mel_bins;
    const int Hd = c.fvae_enc_dec_hidden, Hf = c.prior_glow_hidden, Le = c.fvae_enc_n_layers;
    if (mel_ld && mel_ld < T) return fail(h, DTTS_E_INVAL, "tgt_mels holds %d frames per utterance, T_mel = %d", mel_ld, T);
    if (mel_cap && mel_cap < T) return fail(h, DTTS_E_INVAL, "mel_out holds %d frames per utterance, T_mel = %d", mel_cap, T);
    if (eps && eps_ld && eps_ld < T4) return fail(h, DTTS_E_INVAL, "eps holds %d steps per row, T_mel/4 = %d", eps_ld, T4);
    const size_t mrows = (size_t)B * T, qrows = (size_t)B * T4;
    const int CW = 2 * Hd * c.fvae_dec_n_layers;
    const bool dec_x3 = !h->dec_wn.in.empty() && h->dec_wn.in[0].engine == ENG_BF16X3;
    HIPCHK(h->a_post.reserve(sizeof(float) * (mrows * (size_t)(C + 3 * Hd + (dec_x3 ? 0 : CW)) + ((size_t)B * h->T_w + 1) * CW +
                                              qrows * (size_t)(C + 2 + 3 * Hd + 2 * Hd * Le + 3 * Z + 2 * Hf * c.prior_glow_n_layers + 3 * Hf +
                                                               (h->fs_w_fwd ? h->fs_cond_fwd.C_out : 0))) +
                             sizeof(double) * 2 * KL_BLOCKS + (64 << 10), s));
    Arena& A = h->a_post;
    float* g = A.alloc<float>(mrows * C);
    float* gs = A.alloc<float>(qrows * C);
    float* msq = A.alloc<float>(qrows);
    float* hq = A.alloc<float>(qrows * Hd);
    float* ecnd = A.alloc<float>(qrows * 2 * Hd * Le);
    float* eacts = A.alloc<float>(qrows * Hd);
    float* eout = A.alloc<float>(qrows * Hd);
    float* epsb = A.alloc<float>(qrows * Z);
    float* zq = A.alloc<float>(qrows * Z);
    float* zp = A.alloc<float>(qrows * Z);
    float* logq = A.alloc<float>(qrows);
    float* fcond = A.alloc<float>(qrows * 2 * Hf * c.prior_glow_n_layers);
    float* fh = A.alloc<float>(qrows * Hf);
    float* facts = A.alloc<float>(qrows * Hf);
    float* fout = A.alloc<float>(qrows * Hf);
    float* dx = A.alloc<float>(mrows * Hd);
    float* dacts = A.alloc<float>(mrows * Hd);
    float* dout = A.alloc<float>(mrows * Hd);
    float* cond_w = A.alloc<float>(((size_t)B * h->T_w + 1) * CW);
    double* partial = A.alloc<double>(2 * KL_BLOCKS);
    if (!g || !gs || !msq || !hq || !ecnd || !eacts || !eout || !epsb || !zq || !zp || !logq || !fcond || !fh || !facts || !fout || !dx || !dacts ||
        !dout || !cond_w || !partial)
        return fail(h, DTTS_E_NOMEM, "posterior workspace");
    // g = expand(word_encoder_out) (* tgt_nonpadding), x_mask = (mel2word > 0); g_sqz = g_pre_net(g) exactly as the infer path computes them
    LAUNCH(expand_launch(h->weo, h->m2w, g, h->x_mask, B, h->T_w, T, C, s));
    int rc = run_g_sqz(h, g, gs, B, T, s);
    if (rc) return rc;
    LAUNCH(mask_sqz_launch(h->x_mask, msq, B, T, T4, s));   // x_mask[:, :, ::4] (fvae_semantics.py:31)
    // posterior encoder (fvae_semantics.py:29-35): pre_net(x) * x_mask_sqz, the masked WN conditioned on g_sqz, out_proj + sample + log q
    {
        ConvParams p = base_params(tgt_mels, n_mel, B, T, T4, hq, Hd);
        p.x_bstride = (long long)(mel_ld ? mel_ld : T) * n_mel;
        p.row_mask = msq;
        LAUNCH(conv1d_launch(h->post_pre, p, s));
    }
    if (h->post_wn.cond.engine == ENG_BF16X3) {   // the conditioning of all 8 layers by one split-operand convolution, then the masked layers
        VConvParams v = vparams_x3(h->post_wn.cond, gs, C, 1.f, nullptr, B, T4);
        v.yf = ecnd;
        v.ldyf = 2 * Hd * Le;
        LAUNCH(vconv_launch(v, s));
        rc = run_wn(h, h->post_wn, hq, nullptr, C, ecnd, eacts, eout, B, T4, s, nullptr, 0, msq);
    } else {
        rc = run_wn(h, h->post_wn, hq, gs, C, ecnd, eacts, eout, B, T4, s, nullptr, 0, msq);
    }
    if (rc) return rc;
    if (eps) {
        LAUNCH(transpose_cf_to_cl_launch(eps, epsb, B, Z, T4, s, eps_ld));
    } else {
        LAUNCH(normal_fill_launch(epsb, (long long)qrows * Z, h->noise_seed + ++h->noise_counter, s));   // torch.randn_like(m) (:34)
    }
    LAUNCH(post_proj_sample_launch(eout, h->post_wt, h->post_bias, epsb, zq, logq, m_q, logs_q, B, T4, Hd, Z, s));
    // prior flow, forward, masked (glow_modules.py:108-123,157-161) on a copy of z_q, then log p and the KL (fvae_semantics.py:95-99)
    if (z_p || kl) {
        FlowScratch fw = {nullptr, fcond, fh, facts, fout};
        if (h->fs_w_fwd && !(fw.cond_all = A.alloc<float>(qrows * h->fs_cond_fwd.C_out))) return fail(h, DTTS_E_NOMEM, "posterior workspace");
        rc = run_prior_flow(h, h->flows_fwd, h->fs_w_fwd, h->fs_cond_fwd, gs, zq, zp, msq, fw, B, T4, s);
        if (rc) return rc;
        LAUNCH(kl_launch(zp, logq, msq, z_p, partial, kl, B, T4, Z, s));
    }
    // decoder with the frame mask (fvae_semantics.py:52-57): pre_net(z_q) * x_mask, the masked WN, out_proj
    ConvParams p = base_params(zq, Z, B, T4, T4, dx, 4 * Hd);
    LAUNCH(conv1d_launch(h->dec_pre, p, s));
    LAUNCH(rows_scale_launch(dx, h->x_mask, (long long)mrows, Hd, s));
    return run_decoder_tail(h, A, "posterior workspace", cond_w, dx, dacts, dout, h->x_mask, mel_out, mel_cap, s);
}

int dtts_text2mel_plan(dtts_handle h, const int64_t* word_tokens, const float* keys, const float* values, const float* key_map,
                       const int64_t* pinyin, const int64_t* pinyin_map, const int64_t* pron_modified, const int64_t* mel2word,
                       int T_m2w, int B, int T_w, int L_k, int P, int32_t* T_mel_host, dtts_stream stream) {
    return dtts_text2mel_encode(h, word_tokens, keys, values, key_map, pinyin, pinyin_map, pron_modified, mel2word, T_m2w, B, T_w, L_k,
                                P, T_mel_host, stream);
}

static int forward_tail(dtts_handle h, const float* z_p, int z_cap, float* mel_out, int mel_cap, int T_mel, int64_t* T_mel_out,
                        float* pron_attn, float* dur, dtts_stream stream) {
    if (T_mel_out) *T_mel_out = T_mel;
    if (T_mel > mel_cap) return fail(h, DTTS_E_INVAL, "dtts_text2mel_forward: %d frames exceed the capacity %d of mel_out", T_mel, mel_cap);
    int rc = decode_impl(h, z_p, z_p ? z_cap : 0, mel_out, mel_cap, stream);
    if (rc == DTTS_OK && pron_attn) rc = dtts_text2mel_fetch(h, DTTS_OUT_PRON_ATTN, pron_attn, stream);
    if (rc == DTTS_OK && dur) rc = dtts_text2mel_fetch(h, DTTS_OUT_DUR, dur, stream);
    return rc;
}

int dtts_text2mel_forward(dtts_handle h, const int64_t* word_tokens, const float* keys, const float* values, const float* key_map,
                          const int64_t* pinyin, const int64_t* pinyin_map, const int64_t* pron_modified, const int64_t* mel2word,
                          int T_m2w, const float* z_p, int z_cap, int B, int T_w, int L_k, int P, float* mel_out, int mel_cap,
                          int64_t* T_mel_out, float* pron_attn, float* dur, dtts_stream stream) {
    if (h && (!mel_out || mel_cap <= 0)) return fail(h, DTTS_E_INVAL, "dtts_text2mel_forward: bad argument");
    int32_t T_mel = 0;
    const int rc = dtts_text2mel_encode(h, word_tokens, keys, values, key_map, pinyin, pinyin_map, pron_modified, mel2word, T_m2w, B,
                                        T_w, L_k, P, &T_mel, stream);
    return rc ? rc : forward_tail(h, z_p, z_cap, mel_out, mel_cap, T_mel, T_mel_out, pron_attn, dur, stream);
}

int dtts_text2mel_forward_ids(dtts_handle h, const int64_t* word_tokens, const int32_t* entry_ids, const int64_t* pron_modified,
                              const int64_t* mel2word, int T_m2w, const float* z_p, int z_cap, int B, int T_w, int L_k, int P,
                              float* mel_out, int mel_cap, int64_t* T_mel_out, float* pron_attn, float* dur, dtts_stream stream) {
    if (h && (!mel_out || mel_cap <= 0)) return fail(h, DTTS_E_INVAL, "dtts_text2mel_forward_ids: bad argument");
    int32_t T_mel = 0;
    const int rc = dtts_text2mel_encode_ids(h, word_tokens, entry_ids, pron_modified, mel2word, T_m2w, B, T_w, L_k, P, &T_mel, stream);
    return rc ? rc : forward_tail(h, z_p, z_cap, mel_out, mel_cap, T_mel, T_mel_out, pron_attn, dur, stream);
}

int dtts_text2mel_fetch(dtts_handle h, int what, void* dst, dtts_stream stream) {
    // the block items (none needs an encode); a unit that checks its block before the handle is reached with a null one too
    if (const Unit* u = find_item(what); u && dst && (h || u->null_handle)) return u->forward(h, dst, (hipStream_t)stream);
    if (!h || !dst) return DTTS_E_INVAL;
    if (!h->encoded) return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch before encode");
    if (h->ps_encoded && (what == DTTS_OUT_PRON_ATTN || what == DTTS_OUT_DICT_ATTN || what == DTTS_OUT_CONTEXT || what == DTTS_OUT_POSTERIOR))
        return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch: item %d belongs to the Dict-TTS model; the last encode was the PortaSpeech baseline's "
                    "(DTTS_PS_ENCODE), which has no dictionary attention and whose posterior pass is not implemented", what);
    if (!h->ps_encoded && (what == DTTS_PS_PH_ENCODER_OUT || what == DTTS_PS_ATTN || what == DTTS_PS_DECODER_INP))
        return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch: item %d needs an encode of the PortaSpeech baseline (DTTS_PS_ENCODE)", what);
    if (what == DTTS_OUT_POSTERIOR) {   // the posterior pass; dst is the host argument block
        const dtts_posterior_args* a = (const dtts_posterior_args*)dst;
        if (a->size != (int32_t)sizeof(dtts_posterior_args))
            return fail(h, DTTS_E_INVAL, "dtts_text2mel_fetch(DTTS_OUT_POSTERIOR): argument block of %d bytes, this library's is %d", a->size,
                        (int)sizeof(dtts_posterior_args));
        return posterior_impl(h, a->tgt_mels_dev, a->mel_ld, a->eps_dev, a->eps_ld, a->mel_out_dev, a->mel_cap, a->m_q_dev, a->logs_q_dev,
                              a->z_p_dev, a->kl_dev, stream);
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t rows = (size_t)h->B * h->T_w, mrows = (size_t)h->B * h->T_mel;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (what) {
        case DTTS_OUT_PRON_ATTN: src = h->pron_attn; bytes = rows * h->P * 4; break;
        case DTTS_OUT_DUR: src = h->dur; bytes = rows * 4; break;
        case DTTS_OUT_MEL2WORD: src = h->m2w; bytes = mrows * 8; break;
        case DTTS_OUT_DICT_ATTN:
            // kept as [B][T_w][L_k] (every word's weights one contiguous row, written coalesced by s2pa_kernel); the reference returns the
            // transposed view weights.permute(0, 1, 3, 2) = [B, 1, L_k, T_w] (dict_encoder.py:66): produced here, when somebody asks for it
            LAUNCH(transpose_cf_to_cl_launch(h->dict_attn, (float*)dst, h->B, h->T_w, h->L_k, s));
            return DTTS_OK;
        case DTTS_OUT_WORD_ENCODER_OUT:
            if (h->enc_spk) {   // padded rows hold the speaker row (model.py:94,102), added here, off the hot path
                if (h->enc_spk_gen != h->spk_gen)
                    return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch(DTTS_OUT_WORD_ENCODER_OUT): the speakers were re-armed since the encode; "
                                "fetch before arming the next batch");
                LAUNCH(weo_spk_fetch_launch(h->weo, h->spk_rows, h->lens, (float*)dst, h->B, h->T_w, h->cfg.hidden_size, s));
                return DTTS_OK;
            }
            src = h->weo;
            bytes = rows * h->cfg.hidden_size * 4;
            break;
        case DTTS_OUT_X_MASK: src = h->x_mask; bytes = mrows * 4; break;
        case DTTS_OUT_CONTEXT: src = h->context; bytes = rows * h->cfg.hidden_size * 4; break;
        case DTTS_OUT_MEL_LENS: src = h->mel_lens; bytes = (size_t)h->B * 4; break;
        case DTTS_PS_PH_ENCODER_OUT: src = h->ps_ph_out; bytes = (size_t)h->B * h->ps_T_ph * h->cfg.hidden_size * 4; break;
        case DTTS_PS_DECODER_INP: src = h->ps_g; bytes = mrows * h->cfg.hidden_size * 4; break;
        case DTTS_PS_ATTN:
            if (!h->ps_attn) return fail(h, DTTS_E_STATE, "dtts_text2mel_fetch(DTTS_PS_ATTN): the encode ran with want_attn = 0");
            src = h->ps_attn;
            bytes = mrows * h->ps_T_ph * 4;
            break;
        default: return fail(h, DTTS_E_INVAL, "dtts_text2mel_fetch: unknown item %d", what);
    }
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
    return DTTS_OK;
}

int dtts_length_regulate(dtts_handle h, const float* dur, const int32_t* ilens, int B, int T_w, int64_t* mel2word, int cap,
                         int32_t* T_max_host, dtts_stream stream) {
    if (!h || !dur || !ilens || !mel2word || !T_max_host || B <= 0 || T_w <= 0 || cap <= 0)
        return fail(h, DTTS_E_INVAL, "dtts_length_regulate: bad argument");
    hipStream_t s = (hipStream_t)stream;
    int *starts = nullptr, *total = nullptr;
    HIPCHK(hipMalloc((void**)&starts, sizeof(int) * ((size_t)B * (T_w + 1) + B)));
    total = starts + (size_t)B * (T_w + 1);
    std::vector<int> tot(B);
    hipError_t e = durations_launch(dur, ilens, starts, total, B, T_w, s);
    if (e == hipSuccess) e = hipMemcpyAsync(tot.data(), total, sizeof(int) * B, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    int T_raw = 0;
    for (int b = 0; b < B; ++b) T_raw = std::max(T_raw, tot[b]);
    *T_max_host = T_raw;
    int rc = DTTS_OK;
    if (e != hipSuccess) rc = fail(h, DTTS_E_HIP, "dtts_length_regulate: %s", hipGetErrorString(e));
    else if (T_raw > cap) rc = fail(h, DTTS_E_INVAL, "dtts_length_regulate: %d frames exceed the capacity %d", T_raw, cap);
    else {
        e = mel2word_fill_launch(starts, total, ilens, mel2word, B, T_w, cap, cap, s);  // columns >= total[b] are zero
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = fail(h, DTTS_E_HIP, "dtts_length_regulate: %s", hipGetErrorString(e));
    }
    (void)hipFree(starts);
    return rc;
}

int dtts_set_noise_seed(dtts_handle h, uint64_t seed) {
    if (!h) return DTTS_E_INVAL;
    h->noise_seed = seed;
    h->noise_counter = 0x5EEDull;
    return DTTS_OK;
}

} // extern "C"
