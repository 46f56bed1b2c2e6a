// libdicttts_hip.so — the acoustic model's weights: S2PA encoders, duration predictor, FVAE (prior flow, decoder, posterior encoder),
// speaker projection.  The passes that run them are in text2mel.hip.
#include "ctx.h"

using namespace dtts;

namespace {

bool build_encoder(dtts_ctx* h, Need& need, Encoder& E, const std::string& p) {
    const int n = h->cfg.enc_layers, C = h->cfg.hidden_size, K = h->cfg.enc_ffn_kernel_size;
    E.l.resize(n);
    for (int i = 0; i < n; ++i) {
        EncLayer& l = E.l[i];
        const std::string a = p + ".attn_layers." + std::to_string(i);
        const HostTensor *wq = need.get(a + ".conv_q.weight"), *wk = need.get(a + ".conv_k.weight"),
                         *wv = need.get(a + ".conv_v.weight");
        const HostTensor *bq = need.get(a + ".conv_q.bias"), *bk = need.get(a + ".conv_k.bias"),
                         *bv = need.get(a + ".conv_v.bias");
        if (!wq || !wk || !wv || !bq || !bk || !bv) return false;
        std::vector<float> bias(3 * C);
        for (int c = 0; c < C; ++c) {
            bias[c] = bq->f[c];
            bias[C + c] = bk->f[c];
            bias[2 * C + c] = bv->f[c];
        }
        const float *pq = wq->f.data(), *pk = wk->f.data(), *pv = wv->f.data();
        if (!pack_conv(h, l.qkv, ENG_F32, 3 * C, C, 1,
                       [=](int co, int ci, int) {
                           const float* src = co < C ? pq : (co < 2 * C ? pk : pv);
                           return src[(size_t)(co % C) * C + ci];
                       },
                       bias, 1, 1, 0))
            return false;
        if (!pack_plain(h, need, l.o, ENG_F32, a + ".conv_o", 1, 1, 0)) return false;
        const std::string f = p + ".ffn_layers." + std::to_string(i);
        if (!pack_plain(h, need, l.ffn1, ENG_F32, f + ".conv_1", 1, 1, K / 2)) return false;
        if (!pack_plain(h, need, l.ffn2, ENG_F32, f + ".conv_2", 1, 1, 0)) return false;
        l.g1 = upload_named(h, need, p + ".norm_layers_1." + std::to_string(i) + ".gamma");
        l.b1 = upload_named(h, need, p + ".norm_layers_1." + std::to_string(i) + ".beta");
        l.g2 = upload_named(h, need, p + ".norm_layers_2." + std::to_string(i) + ".gamma");
        l.b2 = upload_named(h, need, p + ".norm_layers_2." + std::to_string(i) + ".beta");
        if (!l.g1 || !l.b1 || !l.g2 || !l.b2) return false;
    }
    E.lg = upload_named(h, need, p + ".last_ln.gamma");
    E.lb = upload_named(h, need, p + ".last_ln.beta");
    return E.lg && E.lb;
}

// eng: ENG_F32 (exact fp32 MFMA, generic kernel) or ENG_BF16X3 (split operands: the vconv kernel's WaveNet form)
// cond_eng: the conditioning layer's engine (ENG_BF16X3: computed by the caller on the vconv kernel, as the posterior encoder does)
bool build_wn(dtts_ctx* h, Need& need, WNet& W, const std::string& p, int hidden, int k, int layers, int eng = ENG_F32, int cond_eng = ENG_F32) {
    W.hidden = hidden;
    W.layers = layers;
    W.in.resize(layers);
    W.rs.resize(layers);
    for (int i = 0; i < layers; ++i) {
        if (!pack_plain(h, need, W.in[i], eng, p + ".in_layers." + std::to_string(i), 1, 1, (k - 1) / 2, true, hidden))
            return false;
        if (!pack_plain(h, need, W.rs[i], eng, p + ".res_skip_layers." + std::to_string(i), 1, 1, 0)) return false;
    }
    return pack_plain(h, need, W.cond, cond_eng, p + ".cond_layer", 1, 1, 0);
}

// spk_embed_proj (modules/portaspeech/model.py:159-163), optional: the form follows from the shapes — weight [hidden][256] + bias [hidden]
// = nn.Linear(256, hidden) (use_spk_embed), weight [num_spk][hidden] without bias = Embedding(num_spk, hidden) (use_spk_id)
int build_speaker(dtts_ctx* h) {
    h->spk_kind = 0;
    h->spk_n = 0;
    h->spk_armed_B = 0;
    const auto iw = h->w.find("model.spk_embed_proj.weight"), ib = h->w.find("model.spk_embed_proj.bias");
    const bool has_w = iw != h->w.end(), has_b = ib != h->w.end();
    if (!has_w && !has_b) return DTTS_OK;
    const int H = h->cfg.hidden_size;
    if (!has_w) return fail(h, DTTS_E_INVAL, "spk_embed_proj.bias without spk_embed_proj.weight");
    const HostTensor& w = iw->second;
    if (has_b) {
        if (w.shape.size() != 2 || w.shape[0] != H || w.shape[1] != SPK_IN || ib->second.shape.size() != 1 || ib->second.shape[0] != H)
            return fail(h, DTTS_E_INVAL, "spk_embed_proj with a bias must be nn.Linear(%d, %d): weight [%d, %d] + bias [%d] expected, got weight "
                        "of %d dims [%lld, %lld]", SPK_IN, H, H, SPK_IN, H, (int)w.shape.size(), w.shape.empty() ? -1LL : (long long)w.shape[0],
                        w.shape.size() > 1 ? (long long)w.shape[1] : -1LL);
        std::vector<float> wt((size_t)SPK_IN * H);
        for (int o = 0; o < H; ++o)
            for (int k = 0; k < SPK_IN; ++k) wt[(size_t)k * H + o] = w.f[(size_t)o * SPK_IN + k];
        h->spk_w = upload(h, wt);
        h->spk_bias = upload(h, ib->second.f);
        if (!h->spk_w || !h->spk_bias) return fail(h, DTTS_E_NOMEM, "uploading spk_embed_proj");
        h->spk_kind = DTTS_SPK_EMBED;
        return DTTS_OK;
    }
    if (w.shape.size() != 2 || w.shape[1] != H || w.shape[0] < 1 || w.shape[0] > INT_MAX / H)
        return fail(h, DTTS_E_INVAL, "spk_embed_proj.weight without a bias must be Embedding(num_spk, %d) = [num_spk, %d], got %d dims [%lld, %lld]",
                    H, H, (int)w.shape.size(), w.shape.empty() ? -1LL : (long long)w.shape[0], w.shape.size() > 1 ? (long long)w.shape[1] : -1LL);
    h->spk_w = upload(h, w.f);
    h->spk_bias = nullptr;
    if (!h->spk_w) return fail(h, DTTS_E_NOMEM, "uploading spk_embed_proj");
    h->spk_n = (int)w.shape[0];
    h->spk_kind = DTTS_SPK_ID;
    return DTTS_OK;
}

// One coupling block (prior_flow.flows.<2f> = p) for the fused prior-flow kernel (flowstack.hip): its logical weights with the flip folded into
// the channel order of pre / post (rev) as in the launch-by-launch packs, post and its bias times `sign` (-1: the reverse flow's x1 - m as
// an add; +1: the forward flow), appended to fs_host; its cond_layer appended to fs_cond_w / fs_cond_b.  false: a tensor is missing or has
// an unexpected shape (nothing is appended)
bool flowstack_block(dtts_ctx* h, Need& need, const std::string& p, bool rev, float sign, std::vector<float>& fs_host,
                     std::vector<float>& fs_cond_w, std::vector<float>& fs_cond_b) {
    const dtts_config& c = h->cfg;
    const int Hf = c.prior_glow_hidden, half = c.latent_size / 2, nl = c.prior_glow_n_layers;
    const HostTensor *wpre = need.get(p + ".pre.weight"), *wpost = need.get(p + ".post.weight");
    const std::vector<float> bpre = bias_of(need, p + ".pre"), bpost = bias_of(need, p + ".post");
    if (!wpre || !wpost || bpre.empty() || bpost.empty()) return false;
    FlowStackHostWeights fw;
    fw.pre.resize((size_t)Hf * half);
    for (int co = 0; co < Hf; ++co)
        for (int ci = 0; ci < half; ++ci) fw.pre[(size_t)co * half + ci] = wpre->f[(size_t)co * half + (rev ? half - 1 - ci : ci)];
    fw.bpre = bpre;
    fw.post.resize((size_t)half * Hf);
    fw.bpost.resize(half);
    for (int q = 0; q < half; ++q) {
        fw.bpost[q] = sign * bpost[rev ? half - 1 - q : q];
        for (int ci = 0; ci < Hf; ++ci) fw.post[(size_t)q * Hf + ci] = sign * wpost->f[(size_t)(rev ? half - 1 - q : q) * Hf + ci];
    }
    for (int l = 0; l < nl; ++l) {
        const std::string bi = p + ".enc.in_layers." + std::to_string(l), br = p + ".enc.res_skip_layers." + std::to_string(l);
        const HostTensor *wi = folded_weight(h, need, bi), *wr = folded_weight(h, need, br);
        std::vector<float> b1 = bias_of(need, bi), b2 = bias_of(need, br);
        const size_t n_rs = (size_t)(l == nl - 1 ? Hf : 2 * Hf);
        if (!wi || !wr || wi->f.size() != (size_t)2 * Hf * Hf * c.glow_kernel_size || wr->f.size() != n_rs * Hf || b1.size() != (size_t)2 * Hf ||
            b2.size() != n_rs)
            return false;
        fw.in.push_back(wi->f);
        fw.bin.push_back(b1);
        fw.rs.push_back(wr->f);
        fw.brs.push_back(b2);
    }
    const HostTensor* wc = folded_weight(h, need, p + ".enc.cond_layer");
    const std::vector<float> bc = bias_of(need, p + ".enc.cond_layer");
    const size_t n_c = (size_t)2 * Hf * nl;
    if (!wc || wc->f.size() != n_c * c.hidden_size || bc.size() != n_c) return false;
    flowstack_pack(fw, nl, !c.decoder_fp32, fs_host);
    fs_cond_w.insert(fs_cond_w.end(), wc->f.begin(), wc->f.end());
    fs_cond_b.insert(fs_cond_b.end(), bc.begin(), bc.end());
    return true;
}

// The FVAE posterior encoder + the prior flow's forward-direction packs.  A checkpoint without fvae.encoder.* loads as before; the
// posterior call then reports the missing tensor.  The forward flow shares pre / WN packs with the reverse one (same flip parity per block:
// block f sees f flips going forward and n - f going back, n even) and gets its own post pack with the reference's signs.
int build_posterior(dtts_ctx* h) {
    h->post_ready = false;
    h->post_missing.clear();
    h->post_unsupported.clear();
    h->flows_fwd.clear();
    const dtts_config& c = h->cfg;
    const std::string p = "model.fvae.encoder";
    if (c.latent_size != 16 || c.fvae_enc_dec_hidden > 512 || c.frames_multiple % 4) {
        h->post_unsupported = "the posterior pass supports latent_size 16, fvae_enc_dec_hidden <= 512 and frames_multiple % 4 == 0 (latent_size " +
                              std::to_string(c.latent_size) + ", fvae_enc_dec_hidden " + std::to_string(c.fvae_enc_dec_hidden) +
                              ", frames_multiple " + std::to_string(c.frames_multiple) + ")";
        return DTTS_OK;
    }
    if (!h->w.count(p + ".pre_net.0.weight") && !h->w.count(p + ".pre_net.0.weight_v")) {
        h->post_missing = p + ".pre_net.0.weight";
        return DTTS_OK;
    }
    Need need{h, ""};
    const int Hd = c.fvae_enc_dec_hidden, Z = c.latent_size, half = Z / 2, Hf = c.prior_glow_hidden;
    bool ok = pack_plain(h, need, h->post_pre, ENG_F32, p + ".pre_net.0", 1, 4, 2);
    // the encoder WaveNet (8 layers at T_mel / 4) on the decoder's engine: split-bf16 operands unless the width does not tile or fp32 was asked for
    const int eng = (Hd % 64 == 0 && !c.decoder_fp32) ? ENG_BF16X3 : ENG_F32;
    // (its 192 -> 3,072 conditioning on the vconv kernel too when the width allows: 1.2 MFLOP per T/4 row, like fs_cond)
    const int cond_eng = (eng == ENG_BF16X3 && (2 * Hd * c.fvae_enc_n_layers) % 256 == 0 && c.hidden_size == 192) ? ENG_BF16X3 : ENG_F32;
    ok = ok && build_wn(h, need, h->post_wn, p + ".wn", Hd, c.fvae_kernel_size, c.fvae_enc_n_layers, eng, cond_eng);
    const HostTensor* wo = ok ? folded_weight(h, need, p + ".out_proj") : nullptr;
    std::vector<float> bo = ok ? bias_of(need, p + ".out_proj") : std::vector<float>();
    if (ok && wo && !bo.empty()) {
        if (wo->numel() != (int64_t)2 * Z * Hd || (int)bo.size() != 2 * Z)
            return fail(h, DTTS_E_INVAL, "fvae.encoder.out_proj must be Conv1d(%d, %d, 1)", Hd, 2 * Z);
        std::vector<float> wt((size_t)Hd * 2 * Z);
        for (int o = 0; o < 2 * Z; ++o)
            for (int k = 0; k < Hd; ++k) wt[(size_t)k * 2 * Z + o] = wo->f[(size_t)o * Hd + k];
        h->post_wt = upload(h, wt);
        h->post_bias = upload(h, bo);
        if (!h->post_wt || !h->post_bias) return fail(h, DTTS_E_NOMEM, "uploading fvae.encoder.out_proj");
    } else
        ok = false;
    const int n = (int)h->flows.size();
    std::vector<float> fs_host, fs_cond_w, fs_cond_b;
    const bool fuse = h->fs_w != nullptr;   // the reverse flow is fused: the forward one is too (same shapes, same DTTS_TUNE bit 8)
    for (int f = 0; ok && f < n; ++f) {
        Flow fl = h->flows[n - 1 - f];   // h->flows is in reverse execution order: the same block, the same pre / WN packs and channel offsets
        const bool rev = f & 1;
        const std::string q = "model.fvae.prior_flow.flows." + std::to_string(2 * f);
        const HostTensor* wpost = need.get(q + ".post.weight");
        std::vector<float> bpost = bias_of(need, q + ".post");
        if (!wpost || bpost.empty()) { ok = false; break; }
        const float* pp = wpost->f.data();
        std::vector<float> b(half);
        for (int o = 0; o < half; ++o) b[o] = bpost[rev ? half - 1 - o : o];
        fl.post = PackedConv();
        // x1 = post(h) + x1, masked (glow_modules.py:112,120): the epilogue's residual add, then the row mask
        ok = pack_conv(h, fl.post, ENG_F32, half, Hf, 1, [=](int co, int ci, int) { return pp[(size_t)(rev ? half - 1 - co : co) * Hf + ci]; }, b, 1, 1, 0);
        h->flows_fwd.push_back(fl);
        // the same block for the fused kernel, post with the reference's sign (the shapes were checked when the reverse blocks were packed)
        if (ok && fuse) ok = flowstack_block(h, need, q, rev, 1.f, fs_host, fs_cond_w, fs_cond_b);
    }
    h->fs_w_fwd = nullptr;
    if (ok && fuse && n > 0) {
        h->fs_w_fwd = upload(h, fs_host);
        const int n_c = (int)fs_cond_b.size(), Cg = c.hidden_size;
        const float* pc = fs_cond_w.data();
        ok = h->fs_w_fwd && pack_conv(h, h->fs_cond_fwd, h->fs_cond.engine, n_c, Cg, 1, [=](int co, int ci, int) { return pc[(size_t)co * Cg + ci]; },
                                      fs_cond_b, 1, 1, 0);
    }
    if (!ok) {
        if (!need.missing.empty()) {
            h->post_missing = need.missing;
            h->flows_fwd.clear();
            return DTTS_OK;
        }
        if (h->err.empty()) return fail(h, DTTS_E_NOMEM, "packing / uploading the FVAE posterior encoder failed");
        return DTTS_E_INVAL;
    }
    h->post_ready = true;
    return DTTS_OK;
}

} // namespace

namespace dtts {

// The duration predictor (modules/portaspeech/model.py:38-66) from "<m>dur_predictor.*": shared by the Dict-TTS part and the baseline
bool build_dur_predictor(dtts_ctx* h, Need& need, const std::string& m) {
    const dtts_config& c = h->cfg;
    bool ok = true;
    h->dur_conv.resize(c.dur_predictor_layers);
    h->dur_g.resize(c.dur_predictor_layers);
    h->dur_b.resize(c.dur_predictor_layers);
    for (int i = 0; ok && i < c.dur_predictor_layers; ++i) {
        const std::string p = m + "dur_predictor.conv." + std::to_string(i);
        ok = ok && pack_plain(h, need, h->dur_conv[i], ENG_F32, p + ".1", 1, 1, (c.dur_predictor_kernel - 1) / 2);
        h->dur_g[i] = upload_named(h, need, p + ".3.weight");
        h->dur_b[i] = upload_named(h, need, p + ".3.bias");
        ok = ok && h->dur_g[i] && h->dur_b[i];
    }
    h->dur_w = upload_named(h, need, m + "dur_predictor.linear.0.weight");
    h->dur_bias = upload_named(h, need, m + "dur_predictor.linear.0.bias");
    ok = ok && h->dur_w && h->dur_bias;
    return ok;
}

// The FVAE's inference half (g_pre_net, the prior flow in reverse, the decoder) from "<m>fvae.*": shared in the same way
bool build_fvae(dtts_ctx* h, Need& need, const std::string& m, int* rc) {
    const dtts_config& c = h->cfg;
    bool ok = true;
    *rc = DTTS_OK;
    ok = ok && pack_plain(h, need, h->g_pre, c.decoder_fp32 ? ENG_F32 : ENG_BF16X3, m + "fvae.g_pre_net.0", 1, 4, 2);
    // g_pre_net = Conv1d(k = 8, stride 4, pad 2) as a STRIDE-1, 3-tap convolution over 4-frame groups: [B][T][C] is also [B][T/4][4C]
    // (T is a multiple of frames_multiple = 4), out[q] = sum_j W_j x[4q + j - 2] reads group q - 1 (frames 2, 3), q (all four) and q + 1
    // (frames 0, 1) — on the split-operand vconv kernel, which skips the two all-zero half taps per input chunk (vconv.hip: in_half).
    h->g_pre_poly = PackedConv();
    if (ok && !c.decoder_fp32 && c.frames_multiple == 4 && c.hidden_size % 64 == 0) {
        const HostTensor* wg = folded_weight(h, need, m + "fvae.g_pre_net.0");
        std::vector<float> bg = bias_of(need, m + "fvae.g_pre_net.0");
        if (wg && wg->shape.size() == 3 && wg->shape[2] == 8 && !bg.empty()) {
            const int Co = (int)wg->shape[0], Ci = (int)wg->shape[1];
            const float* pw = wg->f.data();
            ok = pack_conv(h, h->g_pre_poly, ENG_BF16X3, Co, 4 * Ci, 3,
                           [=](int co, int cip, int tap) {
                               const int ph = cip / Ci, ci = cip % Ci, j = 4 * (tap - 1) + ph + 2;
                               return (j >= 0 && j < 8) ? pw[((size_t)co * Ci + ci) * 8 + j] : 0.f;
                           },
                           bg, 1, 1, 1, 0, 2.0 * Co * Ci * 8);
        }
    }
    const int half = c.latent_size / 2;
    h->flows.clear();
    int parity = 0;
    // one fused kernel for the whole prior flow where the configuration allows (DTTS_TUNE bit 8: launch by launch again)
    bool fuse_flows = flowstack_supported(c.prior_glow_hidden, c.glow_kernel_size, c.prior_glow_n_layers, c.prior_glow_n_blocks, c.latent_size) &&
                      !DTTS_TUNE(h, 256);
    std::vector<float> fs_host, fs_cond_w, fs_cond_b;
    for (int f = c.prior_glow_n_blocks - 1; ok && f >= 0; --f) {
        // reversed(flows): Flip, then the coupling layer (glow_modules.py:157-163).  The flip is not executed:
        // it is tracked as a parity and folded into the channel order of pre / post.
        parity ^= 1;
        Flow fl;
        const std::string p = m + "fvae.prior_flow.flows." + std::to_string(2 * f);
        const HostTensor *wpre = need.get(p + ".pre.weight"), *wpost = need.get(p + ".post.weight");
        std::vector<float> bpre = bias_of(need, p + ".pre"), bpost = bias_of(need, p + ".post");
        if (!wpre || !wpost || bpre.empty() || bpost.empty()) { ok = false; break; }
        const int Hf = c.prior_glow_hidden;
        const float *ppre = wpre->f.data(), *ppost = wpost->f.data();
        const bool rev = parity == 1;
        // logical x0[c] = phys[rev ? 15 - c : c], c < half ; logical x1[c] = phys[rev ? 7 - c : 8 + c]
        fl.in_coff = rev ? half : 0;
        fl.out_coff = rev ? 0 : half;
        ok = ok && pack_conv(h, fl.pre, ENG_F32, Hf, half, 1,
                             [=](int co, int ci, int) { return ppre[(size_t)co * half + (rev ? half - 1 - ci : ci)]; }, bpre, 1, 1, 0);
        std::vector<float> nb(half);
        for (int q = 0; q < half; ++q) nb[q] = -bpost[rev ? half - 1 - q : q];
        // x1 = x1 - m  ->  epilogue residual add with negated weights
        ok = ok && pack_conv(h, fl.post, ENG_F32, half, Hf, 1,
                             [=](int co, int ci, int) { return -ppost[(size_t)(rev ? half - 1 - co : co) * Hf + ci]; }, nb, 1, 1, 0);
        ok = ok && build_wn(h, need, fl.wn, p + ".enc", Hf, c.glow_kernel_size, c.prior_glow_n_layers);
        h->flows.push_back(fl);
        // the same block for the fused kernel (flowstack.hip); an unexpected shape: the launch-by-launch path reports it
        if (ok && fuse_flows) fuse_flows = flowstack_block(h, need, p, rev, -1.f, fs_host, fs_cond_w, fs_cond_b);
    }
    if (ok && parity != 0)
        return (*rc = fail(h, DTTS_E_INVAL, "prior_glow_n_blocks %d: an odd number of flow blocks is not supported", c.prior_glow_n_blocks)), false;
    h->fs_w = nullptr;
    if (ok && fuse_flows && !h->flows.empty()) {
        h->fs_w = upload(h, fs_host);
        const int n_c = (int)fs_cond_b.size(), Cg = c.hidden_size;
        const float* pc = fs_cond_w.data();
        // (split-bf16 operands on the vconv kernel like the WaveNet layers it conditions, unless the exact-fp32 decoder was asked for)
        ok = ok && h->fs_w && pack_conv(h, h->fs_cond, (c.decoder_fp32 || Cg % 64 || n_c % 256) ? ENG_F32 : ENG_BF16X3, n_c, Cg, 1,
                                         [=](int co, int ci, int) { return pc[(size_t)co * Cg + ci]; }, fs_cond_b, 1, 1, 0);
    }
    ok = ok && pack_transposed(h, need, h->dec_pre, ENG_F32, m + "fvae.decoder.pre_net.0", 4, 0);
    // the decoder WaveNet carries 4.09 of the acoustic model's 4.69 MFLOP per frame: split-bf16 operands (three bf16 MFMAs
    // per product = 5.3x the fp32-MFMA rate, mel error ~3e-5 against the 1e-3 gate) unless the hidden width does not tile
    const int dec_eng = (c.fvae_enc_dec_hidden % 64 == 0 && !c.decoder_fp32) ? ENG_BF16X3 : ENG_F32;
    ok = ok && build_wn(h, need, h->dec_wn, m + "fvae.decoder.wn", c.fvae_enc_dec_hidden, c.fvae_kernel_size, c.fvae_dec_n_layers, dec_eng);
    ok = ok && pack_plain(h, need, h->dec_out, ENG_F32, m + "fvae.decoder.out_proj", 1, 1, 0);
    return ok;
}

int build_acoustic(dtts_ctx* h) {
    if (h->ps_ready)   // the two acoustic models share the duration predictor's and the FVAE's packs: a context holds one of them
        return fail(h, DTTS_E_STATE, "dtts_finalize_weights(DTTS_PART_ACOUSTIC): this context holds the PortaSpeech baseline (DTTS_PART_PORTASPEECH); "
                    "a context holds one acoustic model");
    Need need{h, ""};
    const dtts_config& c = h->cfg;
    const std::string m = "model.";
    const std::string enc = m + "dict_encoder.S2PA_module";
    bool ok = true;
    h->word_emb = upload_named(h, need, enc + ".word_emb.weight");
    const std::string att = enc + ".s2pa_attention";
    h->pinyin_emb = upload_named(h, need, att + ".pinyin_embedding.weight");
    ok = ok && h->word_emb && h->pinyin_emb;
    ok = ok && build_encoder(h, need, h->sem, enc + ".semantic_encoder");
    ok = ok && build_encoder(h, need, h->lin, enc + ".linguistic_encoder");
    // S2PA projections (no bias).  k_transform is applied TRANSPOSED to the query (see ops.h)
    const HostTensor *wq = need.get(att + ".q_transform.weight"), *wk = need.get(att + ".k_transform.weight"),
                     *wv = need.get(att + ".v_transform.weight"), *wo = need.get(att + ".output_transform.weight");
    if (ok && wq && wk && wv && wo) {
        const int H = c.hidden_size, D = c.gloss_dim;
        const float *pq = wq->f.data(), *pk = wk->f.data(), *pv = wv->f.data(), *po = wo->f.data();
        ok = ok && pack_conv(h, h->s2_q, ENG_F32, H, H, 1, [=](int co, int ci, int) { return pq[(size_t)co * H + ci]; }, {}, 1, 1, 0);
        ok = ok && pack_conv(h, h->s2_kT, ENG_F32, D, H, 1, [=](int co, int ci, int) { return pk[(size_t)ci * D + co]; }, {}, 1, 1, 0);
        ok = ok && pack_conv(h, h->s2_k, ENG_F32, H, D, 1, [=](int co, int ci, int) { return pk[(size_t)co * D + ci]; }, {}, 1, 1, 0);
        ok = ok && pack_conv(h, h->s2_v, ENG_F32, H, D, 1, [=](int co, int ci, int) { return pv[(size_t)co * D + ci]; }, {}, 1, 1, 0);
        ok = ok && pack_conv(h, h->s2_o, ENG_F32, H, H, 1, [=](int co, int ci, int) { return po[(size_t)co * H + ci]; }, {}, 1, 1, 0);
    } else
        ok = false;
    ok = ok && build_dur_predictor(h, need, m);
    if (ok) {
        int rc = DTTS_OK;
        ok = build_fvae(h, need, m, &rc);
        if (rc) return rc;
    }
    if (ok) {
        const int rc = build_speaker(h);
        if (rc) return rc;
    }
    if (ok) {
        const int rc = build_posterior(h);
        if (rc) return rc;
    }
    if (!ok) {
        if (!need.missing.empty()) return fail(h, DTTS_E_NOENT, "missing weight tensor '%s'", need.missing.c_str());
        if (h->err.empty()) return fail(h, DTTS_E_NOMEM, "packing / uploading acoustic weights failed");
        return DTTS_E_INVAL;
    }
    h->acoustic_ready = true;
    return DTTS_OK;
}

} // namespace dtts
