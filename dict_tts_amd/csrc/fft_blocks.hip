// libdicttts_hip.so — the FFT block stack: weights and forward.
#include "ctx.h"

using namespace dtts;

// ---------------------------------------------------------------------------------------------------------
// FFT block stack (FFTBlocks / EncSALayer): the same fp32-MFMA convolution, attention and LayerNorm
// kernels as the S2PA encoders, with torch-LayerNorm eps, bias-free attention projections and the k**-0.5 GELU FFN
namespace dtts {

// S.K, S.pos and S.last_norm are set by the caller.  *ok = false: a tensor is missing (need.missing names it) or an upload failed;
// a return != 0: a shape was refused with a message
int build_fft_stack(dtts_ctx* h, Need& need, FftStack& S, const std::string& pre, int layers, int C, int heads, bool* okp) {
    const int K = S.K;
    bool& ok = *okp;
    ok = true;
    if (layers <= 0 || K <= 0 || !(K & 1) || C % heads || C / heads > 96)
        return fail(h, DTTS_E_INVAL, "FFT blocks: unsupported configuration (layers=%d kernel=%d hidden=%d heads=%d)", layers, K, C, heads);
    S.l.resize(layers);
    for (int i = 0; i < layers && ok; ++i) {
        EncLayer& l = S.l[i];
        const std::string p = pre + "layers." + std::to_string(i) + ".op.";
        const HostTensor* win = need.get(p + "self_attn.in_proj_weight");   // [3C][C], no bias (EncSALayer: bias=False)
        const HostTensor* wout = need.get(p + "self_attn.out_proj.weight");
        if (!win || !wout) {
            ok = false;
            break;
        }
        if (win->numel() != (int64_t)3 * C * C || wout->numel() != (int64_t)C * C)
            return fail(h, DTTS_E_INVAL, "%sself_attn: projection shapes do not match hidden_size %d", p.c_str(), C);
        const float *pi = win->f.data(), *po = wout->f.data();
        ok = ok && pack_conv(h, l.qkv, ENG_F32, 3 * C, C, 1, [=](int co, int ci, int) { return pi[(size_t)co * C + ci]; },
                             std::vector<float>(), 1, 1, 0);
        ok = ok && pack_conv(h, l.o, ENG_F32, C, C, 1, [=](int co, int ci, int) { return po[(size_t)co * C + ci]; },
                             std::vector<float>(), 1, 1, 0);
        ok = ok && pack_plain(h, need, l.ffn1, ENG_F32, p + "ffn.ffn_1", 1, 1, K / 2);
        ok = ok && pack_plain(h, need, l.ffn2, ENG_F32, p + "ffn.ffn_2", 1, 1, 0);
        if (ok && (l.ffn1.K != K || l.ffn1.C_out != 4 * C))
            return fail(h, DTTS_E_INVAL, "%sffn.ffn_1: kernel %d / width %d differ from the configuration (%d / %d)", p.c_str(), l.ffn1.K,
                        l.ffn1.C_out, K, 4 * C);
        l.g1 = upload_named(h, need, p + "layer_norm1.weight");
        l.b1 = upload_named(h, need, p + "layer_norm1.bias");
        l.g2 = upload_named(h, need, p + "layer_norm2.weight");
        l.b2 = upload_named(h, need, p + "layer_norm2.bias");
        ok = ok && l.g1 && l.b1 && l.g2 && l.b2;
    }
    if (ok && S.last_norm) {
        S.g = upload_named(h, need, pre + "layer_norm.weight");
        S.b = upload_named(h, need, pre + "layer_norm.bias");
        ok = S.g && S.b;
    }
    if (ok && S.pos && h->w.count(pre + "pos_embed_alpha"))   // absent with use_pos_embed_alpha=False: alpha = 1
        ok = (S.alpha = upload_named(h, need, pre + "pos_embed_alpha")) != nullptr;
    return DTTS_OK;
}

int build_fft(dtts_ctx* h) {
    Need need{h, ""};
    const dtts_config& c = h->cfg;
    h->fft.K = c.fft_kernel_size;
    h->fft.pos = c.fft_use_pos_embed != 0;
    h->fft.last_norm = c.fft_use_last_norm != 0;
    bool ok = true;
    if (int rc = build_fft_stack(h, need, h->fft, "fft.", c.fft_layers, c.hidden_size, c.num_heads, &ok)) return rc;
    if (!ok) {
        if (!need.missing.empty()) return fail(h, DTTS_E_NOENT, "missing weight tensor '%s'", need.missing.c_str());
        return h->err.empty() ? fail(h, DTTS_E_HIP, "FFT blocks: weight upload failed") : DTTS_E_HIP;
    }
    h->fft_ready = true;
    return DTTS_OK;
}

int run_fft_stack(dtts_ctx* h, const FftStack& S, const float* x_in, const int* lens_in, const float* pos_table, int n_pos, int B, int T, int C,
                  int heads, float* y, const FftBufs& w, hipStream_t s) {
    const int F = 4 * C;
    const size_t rows = (size_t)B * T;
    float *x = w.x, *hb = w.hb, *qkv = w.qkv, *att = w.att, *ff = w.ff;
    int *lens = w.lens, *pos = w.pos;
    // padding_mask = x.abs().sum(-1).eq(0) unless the caller has the lengths (tts_modules.py:501)
    if (lens_in) HIPCHK(hipMemcpyAsync(lens, lens_in, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
    else LAUNCH(rowcount_nonzero_launch(x_in, lens, B, T, C, s));
    // x = (x + alpha * positions) * nonpadding (:503-509)
    LAUNCH(fft_input_launch(x_in, S.pos ? pos_table : nullptr, n_pos, S.alpha, lens, pos, x, B, T, C, s));
    const float kscale = (float)std::pow((double)S.K, -0.5);
    for (size_t i = 0; i < S.l.size(); ++i) {   // EncSALayer.forward (common_layers.py:649-673)
        const EncLayer& l = S.l[i];
        LAUNCH(layernorm_launch(x, hb, l.g1, l.b1, 1e-5f, lens, 0, 0, B, T, C, s));
        ConvParams p = base_params(hb, C, B, T, T, qkv, 3 * C);
        p.out_lens = lens;   // tiles wholly past the utterance's end are skipped (left unwritten: the attention kernel never reads them)
        LAUNCH(conv1d_launch(l.qkv, p, s));
        // keys past the utterance's end are masked (-1e4 fill: their softmax weight underflows to exactly 0, as with
        // the reference's -inf); query rows past the end are zeroed by the residual epilogue below
        LAUNCH(mha_launch(qkv, att, lens, B, T, C, heads, s));
        p = base_params(att, C, B, T, T, x, C);
        set_res(p, 0, x, C);
        p.out_lens = lens;
        p.zero_masked = 1;
        LAUNCH(conv1d_launch(l.o, p, s));
        LAUNCH(layernorm_launch(x, hb, l.g2, l.b2, 1e-5f, lens, 0, 0, B, T, C, s));
        // TransformerFFNLayer (:558-581): the conv reads the LayerNorm output of padded frames too (= its bias), as the
        // reference's SAME-padded Conv1d does; (conv + bias) * k**-0.5 -> GELU
        p = base_params(hb, C, B, T, T, ff, F);
        p.out_lens = lens;   // dead tiles skipped: ffn_2 is 1x1 and its rows past the end are written as zeros whatever it reads
        p.out_mul = kscale;
        p.post_act = 3;
        LAUNCH(conv1d_launch(l.ffn1, p, s));
        p = base_params(ff, F, B, T, T, x, C);
        set_res(p, 0, x, C);
        p.out_lens = lens;
        p.zero_masked = 1;
        LAUNCH(conv1d_launch(l.ffn2, p, s));
    }
    if (S.last_norm) LAUNCH(layernorm_launch(x, y, S.g, S.b, 1e-5f, lens, 0, 1, B, T, C, s));
    else HIPCHK(hipMemcpyAsync(y, x, rows * C * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DTTS_OK;
}
} // namespace dtts

extern "C" {

int dtts_fft_blocks_forward(dtts_handle h, const float* x_in, const int32_t* lens_in, const float* pos_table, int n_pos, int B, int T,
                            float* y, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    if (!h->fft_ready) return fail(h, DTTS_E_STATE, "FFT block weights not finalized");
    const dtts_config& c = h->cfg;
    if (!x_in || !y || B <= 0 || T <= 0) return fail(h, DTTS_E_INVAL, "dtts_fft_blocks_forward: bad argument");
    if (c.fft_use_pos_embed && (!pos_table || n_pos <= T))
        return fail(h, DTTS_E_INVAL, "dtts_fft_blocks_forward: the stack uses positional embeddings, pos_table needs > T = %d rows (got %d)", T,
                    pos_table ? n_pos : 0);
    hipStream_t s = (hipStream_t)stream;
    const int C = c.hidden_size, F = 4 * C;
    const size_t rows = (size_t)B * T;
    HIPCHK(h->a_fft.reserve(rows * (size_t)(C + C + 3 * C + C + F + 1) * sizeof(float) + (size_t)B * sizeof(int) + (64 << 10), s));
    Arena& A = h->a_fft;
    FftBufs w;
    w.x = A.alloc<float>(rows * C);
    w.hb = A.alloc<float>(rows * C);
    w.qkv = A.alloc<float>(rows * 3 * C);
    w.att = A.alloc<float>(rows * C);
    w.ff = A.alloc<float>(rows * F);
    w.lens = A.alloc<int>(B);
    w.pos = A.alloc<int>(rows);
    if (!w.x || !w.hb || !w.qkv || !w.att || !w.ff || !w.lens || !w.pos) return fail(h, DTTS_E_NOMEM, "FFT workspace");
    return run_fft_stack(h, h->fft, x_in, lens_in, pos_table, n_pos, B, T, C, c.num_heads, y, w, s);
}

} // extern "C"
