// libdicttts_hip.so — HifiGAN: weights, the static fp16 analysis, the two forwards (16-bit operands on the fused kernels; bf16x3 on the
// generic convolution kernel) and the vocoder entry points.
#include "ctx.h"

using namespace dtts;

namespace {

// Static fp16 analysis of the ResBlock operands (VERDICT r4 #3a).  The fused kernels round leaky_relu(x) and leaky_relu(xt) to fp16 in all 72
// ResBlock convolutions, where the reference computes in fp32 (modules/hifigan/hifigan.py:51-58).  Propagated from |mel| <= M through the
// folded weights, per channel:
//   worst case (a PROOF when it stays below 65504):  u_out[co] = |b[co]| + sum_ci u_in[ci] * sum_k |w[co][ci][k]|   (transposed convolutions:
//     the largest output phase), leaky_relu does not grow a bound, the residual adds, the stage output is the mean of its ResBlocks;
//   RMS estimate (NOT a proof: independent, zero-mean terms):  m_out[co] = b^2 + sum_ci m_in[ci] * sum_k w^2, leaky_relu halves it.
// Every (operand, channel) bound is a_q + b_q * M (M^2 for the second moments), both >= 0.  The two parts are propagated SEPARATELY — pass 0: the
// biases with M = 0 (a_q), pass 1: the weights alone, no bias, with M = 1 (b_q) — because the transposed convolutions' maximum over the output
// phases is a maximum of affine functions too: a_q = max_ph a_ph and b_q = max_ph b_ph bound every phase at every M, whereas value(1) - value(0)
// of the phase maxima underestimated the slope whenever another phase leads at M = 1 than at M = 6 (found by tests/test_upsampler_forms_gpu.py:
// 4e-5 .. 2e-4 below the directly evaluated peak at M = 6 for k < 2u, where the phases have unequal numbers of taps).
// The PEAK over channels is a maximum of affine functions — convex, so a secant through the peaks at M = 0 and 1 would UNDERestimate it beyond M = 1 (a bias-dominated channel sets both peaks while another channel's gain term overtakes it at
// M = 6: ADVICE r5).  Reported instead: max_q a_q + M * max_q b_q >= max_q (a_q + b_q M) for every M >= 0 — looser, but a bound.
// For real checkpoints the worst case is astronomically loose (it compounds sum|w| ~ 10-40 per convolution over 6 convolutions per
// ResBlock): it proves small-gain generators only.  Everything else runs fp16 under the always-on detector (conv_post epilogue).
bool vocoder_fp16_analysis(dtts_ctx* h, Need& need) {
    const dtts_config& c = h->cfg;
    const std::string v = "vocoder.";
    const int nk = c.n_resblock_kernels;
    std::vector<double> pt_wc[2], pt_m2[2];   // [pass][operand point x channel, in traversal order]: pass 0 = the bias part (M = 0), pass 1 = the slope (no bias, M = 1)
    for (int pass = 0; pass < 2; ++pass) {
        const double M = pass, bs = pass == 0 ? 1.0 : 0.0;   // bs: the biases count in pass 0 only
        auto conv = [&](const std::string& base, const std::vector<double>& uin, const std::vector<double>& min, std::vector<double>& uout,
                        std::vector<double>& mout) -> bool {   // Conv1d weight [co][ci][k]
            const HostTensor* w = folded_weight(h, need, base);
            const std::vector<float> b = bias_of(need, base);
            if (!w || b.empty() || w->shape.size() != 3) return false;
            const int co_n = (int)w->shape[0], ci_n = (int)w->shape[1], k_n = (int)w->shape[2];
            if ((int)uin.size() < ci_n) return false;
            uout.assign(co_n, 0.0);
            mout.assign(co_n, 0.0);
            for (int co = 0; co < co_n; ++co) {
                double su = bs * std::fabs((double)b[co]), sm = bs * (double)b[co] * b[co];
                for (int ci = 0; ci < ci_n; ++ci) {
                    double a1 = 0, a2 = 0;
                    const float* pw = &w->f[((size_t)co * ci_n + ci) * k_n];
                    for (int k = 0; k < k_n; ++k) {
                        a1 += std::fabs((double)pw[k]);
                        a2 += (double)pw[k] * pw[k];
                    }
                    su += a1 * uin[ci];
                    sm += a2 * min[ci];
                }
                uout[co] = su;
                mout[co] = sm;
            }
            return true;
        };
        std::vector<double> u(c.audio_num_mel_bins, M), m(c.audio_num_mel_bins, M * M), u2, m2;
        if (!conv(v + "conv_pre", u, m, u2, m2)) return false;
        u.swap(u2);
        m.swap(m2);
        for (int i = 0; i < c.n_upsamples; ++i) {
            const int r = c.upsample_rates[i], k_n = c.upsample_kernel_sizes[i], pad = (k_n - r) / 2;
            const HostTensor* w = folded_weight(h, need, v + "ups." + std::to_string(i));   // ConvTranspose1d [ci][co][k]
            const std::vector<float> b = bias_of(need, v + "ups." + std::to_string(i));
            if (!w || b.empty() || w->shape.size() != 3 || (int)w->shape[2] != k_n) return false;
            const int ci_n = (int)w->shape[0], co_n = (int)w->shape[1];
            std::vector<double> ux(co_n, 0.0), mx(co_n, 0.0);
            for (int co = 0; co < co_n; ++co)
                for (int ph = 0; ph < r; ++ph) {   // output phase ph collects the taps k == ph + pad (mod r)
                    double su = bs * std::fabs((double)b[co]), sm = bs * (double)b[co] * b[co];
                    for (int ci = 0; ci < ci_n; ++ci) {
                        const float* pw = &w->f[((size_t)ci * co_n + co) * k_n];
                        double a1 = 0, a2 = 0;
                        for (int k = (ph + pad) % r; k < k_n; k += r) {
                            a1 += std::fabs((double)pw[k]);
                            a2 += (double)pw[k] * pw[k];
                        }
                        su += a1 * u[ci];                    // leaky_relu(0.1) in front does not grow the bound
                        sm += a2 * 0.505 * m[ci];
                    }
                    ux[co] = std::max(ux[co], su);
                    mx[co] = std::max(mx[co], sm);
                }
            std::vector<double> us(co_n, 0.0), ms(co_n, 0.0);
            for (int j = 0; j < nk; ++j) {
                std::vector<double> x = ux, xm = mx, xt, xtm, y, ym, xa(co_n), xam(co_n);
                const std::string rb = v + "resblocks." + std::to_string(i * nk + j);
                // ResBlock1: three times convs1 / convs2 and the residual add; ResBlock2 (hifigan.py:67-84): two convolutions, the residual added
                // after each, the fp16 operands are leaky_relu(x) in front of both
                for (int mth = 0; mth < (h->resblock2 ? 2 : 3); ++mth) {
                    for (int q = 0; q < co_n; ++q) {
                        pt_wc[pass].push_back(x[q]);                             // fp16 operand: leaky_relu(x) (and, iterations 1 / 2, the stored fp16 stream)
                        pt_m2[pass].push_back(xm[q]);
                        xa[q] = x[q];
                        xam[q] = 0.505 * xm[q];
                    }
                    if (h->resblock2) {
                        if (!conv(rb + ".convs." + std::to_string(mth), xa, xam, y, ym)) return false;
                    } else {
                        if (!conv(rb + ".convs1." + std::to_string(mth), xa, xam, xt, xtm)) return false;
                        for (int q = 0; q < co_n; ++q) {
                            pt_wc[pass].push_back(xt[q]);                            // fp16 operand: leaky_relu(xt)
                            pt_m2[pass].push_back(xtm[q]);
                            xtm[q] *= 0.505;
                        }
                        if (!conv(rb + ".convs2." + std::to_string(mth), xt, xtm, y, ym)) return false;
                    }
                    for (int q = 0; q < co_n; ++q) {
                        x[q] += y[q];
                        xm[q] += ym[q];
                    }
                }
                for (int q = 0; q < co_n; ++q) {
                    us[q] += x[q] / nk;
                    ms[q] += xm[q] / nk;      // (second moment of a mean of nk terms: at most their mean)
                }
            }
            u.swap(us);
            m.swap(ms);
        }
    }
    if (pt_wc[0].size() != pt_wc[1].size()) return false;
    double a_wc = 0, b_wc = 0, a_m2 = 0, b_m2 = 0;   // max_q a_q, max_q b_q (possibly different channels: that is the point)
    for (size_t q = 0; q < pt_wc[0].size(); ++q) {
        a_wc = std::max(a_wc, pt_wc[0][q]);
        b_wc = std::max(b_wc, pt_wc[1][q]);
        a_m2 = std::max(a_m2, pt_m2[0][q]);
        b_m2 = std::max(b_m2, pt_m2[1][q]);
    }
    h->wc_const = a_wc;
    h->wc_lin = b_wc;
    h->est_const = std::sqrt(a_m2);
    h->est_lin = std::sqrt(b_m2);
    return true;
}

// One convolution of a whole-ResBlock kernel (rblock.hip, rb2x.hip): the weights of `base` with the tap axis zero padded so that the number of
// k-steps is whole groups of the contraction loop (rblock_padded_taps); K stays the real kernel size.  frag: the fragment order of the kernel
// that walks the pack (rblock.hip: rblock_mfma_shape(ch); rb2x.hip: 32; rbn.hip: RBN_FRAG, whole k-steps of 32 / ch taps and no slack — its kernel
// copies exactly the pack).  false: a tensor is missing or the upload failed.
// Slack: the weight ring runs RD - 1 k-steps ahead — three 16-channel steps (MfmaShape<32>) or one 32-channel step (MfmaShape<16>, RD = 2)
// behind the last tap, in either order less than the one zero tap appended here (>= 2 steps of 32 channels at ch >= 64) on top of pack_conv's own
// slack: the prefetch never clamps.
bool pack_rb_fused(dtts_ctx* h, Need& need, PackedConv& L, int eng, const std::string& base, int ch, int k, int dil, int frag) {
    const HostTensor* w = folded_weight(h, need, base);
    std::vector<float> bias = bias_of(need, base);
    if (!w || bias.empty()) return false;
    const float* pw = w->f.data();
    const int slack = ch >= 64 ? 1 : 2;   // >= 4 zero k-steps behind the last tap: the weight prefetch never clamps
    const bool ok = pack_conv(h, L, eng, ch, ch, frag == RBN_FRAG ? rbn_padded_taps(ch, k) : rblock_padded_taps(ch, k) + slack,
                              [=](int co, int ci, int tap) { return tap < k ? pw[((size_t)co * ch + ci) * k + tap] : 0.f; }, bias, dil, 1, 0, 0, -1, frag);
    L.K = k;
    return ok;
}

// Does the fused forward run this ResBlock1 (ch channels, kernel size k, dilations d[0..2], operand engine eng_rb) iteration by iteration on
// vpair.hip?  THE predicate: build_vocoder packs the block's convolutions in vpair's fragment order exactly where it holds, rb_path sends the
// block to vpair exactly where it holds, and the per-convolution path refuses a pack in another order than its own.
// what vpair_kernel<ch> assumes of a pack it walks: ch x ch x k, nothing padded, in its fragment order
bool vpair_pack_fits(const PackedConv& L, int ch, int k) {
    return L.C_in == ch && L.C_out == ch && L.C_in_pad == ch && L.C_out_pad == ch && L.K == k && L.frag == vpair_mfma_shape(ch);
}
bool vpair_runs(const dtts_config& c, bool resblock2, int eng_rb, int ch, int k, int d0, int d1, int d2) {
    const bool fuse = c.vocoder_precision == DTTS_VOC_F16 || !c.vocoder_unfused;   // (as in hifigan_forward_fused)
    return fuse && !resblock2 && eng_rb != ENG_BF16X3 && !rblock_supported(ch, k) && vpair_supported(ch, k, d0) && vpair_supported(ch, k, d1) &&
           vpair_supported(ch, k, d2);
}

} // namespace

namespace dtts {

int build_vocoder(dtts_ctx* h) {
    Need need{h, ""};
    const dtts_config& c = h->cfg;
    // DTTS_VOC_F16 (default): the six serial convolutions on bf16 hi/lo split operands, the ResBlocks on fp16 operands
    if (c.vocoder_precision != DTTS_VOC_BF16 && c.vocoder_precision != DTTS_VOC_BF16X3 && c.vocoder_precision != DTTS_VOC_F16)
        return fail(h, DTTS_E_INVAL, "vocoder_precision %d is not one of DTTS_VOC_BF16 / _BF16X3 / _F16", c.vocoder_precision);
    // the split-operand staging of conv_pre reads the caller's mel rows with 16-byte loads (vconv.hip): the row width must keep them aligned
    if (c.vocoder_precision == DTTS_VOC_F16 && c.audio_num_mel_bins % 4)
        return fail(h, DTTS_E_INVAL, "DTTS_VOC_F16 needs audio_num_mel_bins %% 4 == 0 (got %d); use DTTS_VOC_BF16X3", c.audio_num_mel_bins);
    if (!h->ovf_dev) {
        if (!(h->ovf_dev = (unsigned long long*)dev_alloc(h, sizeof(unsigned long long))) || hipMemset(h->ovf_dev, 0, sizeof(unsigned long long)) != hipSuccess)
            return fail(h, DTTS_E_NOMEM, "range-guard counter");
    }
    if (!h->bad_dev) {
        if (!(h->bad_dev = (unsigned*)dev_alloc(h, sizeof(unsigned))) || hipMemset(h->bad_dev, 0, sizeof(unsigned)) != hipSuccess)
            return fail(h, DTTS_E_NOMEM, "overflow-detector counter");
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocDefault) != hipSuccess) return fail(h, DTTS_E_NOMEM, "overflow-detector host word");
        h->bad_host = (volatile unsigned*)hp;
        *h->bad_host = 0;
    }
    const int eng = c.vocoder_precision == DTTS_VOC_BF16 ? ENG_BF16 : ENG_BF16X3;                                   // serial convolutions
    const int eng_rb = c.vocoder_precision == DTTS_VOC_F16 ? ENG_F16 : eng;                                         // ResBlock convolutions
    const std::string v = "vocoder.";
    bool ok = pack_plain(h, need, h->conv_pre, eng, v + "conv_pre", 1, 1, 3);
    h->ups.resize(c.n_upsamples);
    h->hop = 1;
    for (int i = 0; ok && i < c.n_upsamples; ++i) {
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        // OPTION (DTTS_TUNE bit 13, off by default): ups.1 — the most expensive serial convolution, 8.4 of their 18.9 MFLOP per frame — in the
        // fp16 two-product form (vconv.hip H2; weights packed as a single fp16 tensor).  Measured: vocoder -0.7 %, pipelined step -0.4 %,
        // waveform RMS error 4.6e-5 -> 7.2e-5 (gate 1e-4): the gain does not pay for a third of the gate's margin, so three products stay.
        const bool h2 = c.vocoder_precision == DTTS_VOC_F16 && i == 1 && DTTS_TUNE(h, 8192) && (u * (c.upsample_initial_channel >> (i + 1))) % 256 == 0 &&
                        (c.upsample_initial_channel >> i) % 128 == 0;
        ok = ok && pack_transposed(h, need, h->ups[i], h2 ? ENG_F16 : eng, v + "ups." + std::to_string(i), u, (k - u) / 2);
        h->hop *= u;
    }
    const int nk = c.n_resblock_kernels;
    h->rb1.assign((size_t)c.n_upsamples * nk, {});
    h->rb2.assign((size_t)c.n_upsamples * nk, {});
    const bool rb2x = h->resblock2;
    for (int i = 0; ok && i < c.n_upsamples * nk; ++i) {   // ResBlock1: convs1 (dilated) / convs2; ResBlock2: convs.{0,1}, both dilated
        const int j = i % nk, k = c.resblock_kernel_sizes[j], n = rb2x ? 2 : 3;
        const int ch = c.upsample_initial_channel >> (i / nk + 1);
        const std::string r = v + "resblocks." + std::to_string(i);
        // Each pack in the fragment order of the kernel that consumes it in THIS context (a context never uses both orders of a layer):
        // vpair's where the ResBlock runs on vpair.hip, the common order for vconv (vocoder_unfused, the per-convolution fallback) and
        // conv1d (DTTS_VOC_BF16X3).
        const int* dl = c.resblock_dilation_sizes[j];
        const bool vp = vpair_runs(c, rb2x, eng_rb, ch, k, dl[0], dl[1], dl[2]);
        const int frag = vp ? vpair_mfma_shape(ch) : 32;
        h->rb1[i].resize(n);
        if (!rb2x) h->rb2[i].resize(3);
        for (int mth = 0; ok && mth < n; ++mth) {
            const int d = c.resblock_dilation_sizes[j][mth];
            ok = ok && pack_plain(h, need, h->rb1[i][mth], eng_rb, r + (rb2x ? ".convs." : ".convs1.") + std::to_string(mth), d, 1, (k * d - d) / 2, true, 0, frag);
            if (!rb2x) ok = ok && pack_plain(h, need, h->rb2[i][mth], eng_rb, r + ".convs2." + std::to_string(mth), 1, 1, (k - 1) / 2, true, 0, frag);
            // vpair walks a pack with the strides of ch x ch x k: the checkpoint's tensors must have the shape the configuration states
            if (ok && vp && !vpair_pack_fits(h->rb1[i][mth], ch, k))
                return fail(h, DTTS_E_INVAL, "%s%d: weight shape [%d, %d, %d] is not the configured [%d, %d, %d]", (r + ".convs1.").c_str(), mth, h->rb1[i][mth].C_out,
                            h->rb1[i][mth].C_in, h->rb1[i][mth].K, ch, ch, k);
            if (ok && vp && !vpair_pack_fits(h->rb2[i][mth], ch, k))
                return fail(h, DTTS_E_INVAL, "%s%d: weight shape [%d, %d, %d] is not the configured [%d, %d, %d]", (r + ".convs2.").c_str(), mth, h->rb2[i][mth].C_out,
                            h->rb2[i][mth].C_in, h->rb2[i][mth].K, ch, ch, k);
        }
    }
    // fused ResBlock kernel (bf16 mode, narrow stages): the same weights with the tap axis zero padded so that the
    // number of k-steps is a multiple of the register ring depth
    h->rbf1.assign((size_t)c.n_upsamples * nk, {});
    h->rbf2.assign((size_t)c.n_upsamples * nk, {});
    for (int i = 0; ok && rb2x && eng_rb != ENG_BF16X3 && i < c.n_upsamples * nk; ++i) {   // ResBlock2: the fused kernel's packs (rb2x.hip)
        const int j = i % nk, k = c.resblock_kernel_sizes[j];
        const int ch = c.upsample_initial_channel >> (i / nk + 1);
        const int d0 = c.resblock_dilation_sizes[j][0], d1 = c.resblock_dilation_sizes[j][1];
        if (!rb2x_supported(ch, k, d0, d1) || h->rb1[i][0].C_in_pad != ch || nk < 2) {   // (nk = 1: no stage sum to fold the block into)
            if (eng_rb == ENG_F16)
                return fail(h, DTTS_E_INVAL, "DTTS_VOC_F16 needs ResBlock2 widths 32/64/128/256, odd kernels 3..11 and a dilation pair whose halo fits the tile "
                            "(resblock %d: %d channels, k=%d, dilations (%d, %d)); use DTTS_VOC_BF16X3", i, ch, k, d0, d1);
            continue;   // bf16: this ResBlock runs convolution by convolution (vconv)
        }
        h->rbf1[i].resize(2);
        for (int mth = 0; ok && mth < 2; ++mth)
            ok = pack_rb_fused(h, need, h->rbf1[i][mth], eng_rb, v + "resblocks." + std::to_string(i) + ".convs." + std::to_string(mth), ch, k,
                               c.resblock_dilation_sizes[j][mth], 32);
    }
    for (int i = 0; ok && !rb2x && eng_rb != ENG_BF16X3 && i < c.n_upsamples * nk; ++i) {
        const int j = i % nk, k = c.resblock_kernel_sizes[j];
        const int ch = c.upsample_initial_channel >> (i / nk + 1);
        const int* dl = c.resblock_dilation_sizes[j];
        // the narrow stages (C = 16 / 8: the V2 generators) have their own whole-ResBlock kernel (rbn.hip); nk = 1: no stage sum to fold the block into
        const bool narrow = nk >= 2 && rbn_supported(ch, k, dl[0], dl[1], dl[2]) && h->rb1[i][0].C_in == ch && h->rb1[i][0].C_out == ch;
        if (!rblock_supported(ch, k) && !narrow) {
            if (eng_rb == ENG_F16 && !vpair_runs(c, rb2x, eng_rb, ch, k, dl[0], dl[1], dl[2]))
                return fail(h, DTTS_E_INVAL, "DTTS_VOC_F16 needs ResBlock widths 8/16/32/64/128/256 and odd kernels 3..11 (resblock %d: %d channels, k=%d); use DTTS_VOC_BF16X3", i, ch, k);
            continue;
        }
        h->rbf1[i].resize(3);
        h->rbf2[i].resize(3);
        const std::string r = v + "resblocks." + std::to_string(i);
        const int ffrag = narrow ? RBN_FRAG : rblock_mfma_shape(ch);
        for (int mth = 0; ok && mth < 3; ++mth) {
            ok = pack_rb_fused(h, need, h->rbf1[i][mth], eng_rb, r + ".convs1." + std::to_string(mth), ch, k, c.resblock_dilation_sizes[j][mth], ffrag);
            ok = ok && pack_rb_fused(h, need, h->rbf2[i][mth], eng_rb, r + ".convs2." + std::to_string(mth), ch, k, 1, ffrag);
        }
    }
    ok = ok && pack_plain(h, need, h->conv_post, eng, v + "conv_post", 1, 1, 3);
    {   // conv_post (C -> 1, k = 7) + tanh fused into the last stage's last ResBlock kernel when that stage runs on rblock at C = 32 or on rbn (C = 16 / 8)
        const int last_ch = c.upsample_initial_channel >> c.n_upsamples;
        const HostTensor* w = ok ? folded_weight(h, need, v + "conv_post") : nullptr;
        const std::vector<float> b = ok ? bias_of(need, v + "conv_post") : std::vector<float>();
        bool fusable = ok && eng_rb != ENG_BF16X3 && (last_ch == 32 || (!rb2x && (last_ch == 16 || last_ch == 8))) && w && w->shape.size() == 3 && w->shape[0] == 1 &&
                       w->shape[1] == last_ch && w->shape[2] == 7 && b.size() == 1 && nk >= 2;
        for (int j = 0; fusable && j < nk; ++j) fusable = !h->rbf1[(size_t)(c.n_upsamples - 1) * nk + j].empty();
        if (fusable) {
            std::vector<float> wt((size_t)7 * last_ch);
            for (int ci = 0; ci < last_ch; ++ci)
                for (int k = 0; k < 7; ++k) wt[(size_t)k * last_ch + ci] = w->f[(size_t)ci * 7 + k];
            h->post_w = upload(h, wt);
            h->post_b = upload(h, b);
            ok = h->post_w && h->post_b;
        }
    }
    if (!ok) {
        if (!need.missing.empty()) return fail(h, DTTS_E_NOENT, "missing weight tensor '%s'", need.missing.c_str());
        if (h->err.empty()) return fail(h, DTTS_E_NOMEM, "packing / uploading vocoder weights failed");
        return DTTS_E_INVAL;
    }
    if (c.vocoder_precision == DTTS_VOC_F16 && !vocoder_fp16_analysis(h, need)) return fail(h, DTTS_E_NOENT, "fp16 analysis: missing weight tensor '%s'", need.missing.c_str());
    h->vocoder_ready = true;
    return DTTS_OK;
}

} // namespace dtts

// ---------------------------------------------------------------------------------------------------------
// HifiGAN forwards.  Stage i (0 = conv_pre's output, i = 1 .. n_upsamples = behind ups[i - 1]) has rows[i] = T * prod(upsample_rates[:i])
// rows per utterance of ch[i] = upsample_initial_channel / 2^i channels; max_elems = the largest activation of any stage for the batch
namespace {

struct StageGeom {
    long long rows[9];
    int ch[9];
    size_t max_elems;
};
StageGeom stage_geom(const dtts_config& c, int B, int T) {
    StageGeom g;
    g.rows[0] = T;
    g.ch[0] = c.upsample_initial_channel;
    g.max_elems = (size_t)B * T * g.ch[0];
    for (int i = 0; i < c.n_upsamples; ++i) {
        g.rows[i + 1] = g.rows[i] * c.upsample_rates[i];
        g.ch[i + 1] = g.ch[i] / 2;
        g.max_elems = std::max<size_t>(g.max_elems, (size_t)B * (size_t)g.rows[i + 1] * (size_t)g.ch[i + 1]);
    }
    return g;
}

struct StageMult { int m[9]; };  // cumulative upsampling factor per stage, passed by value (no H2D copy on the stream)

// wav[b][i] = 0 for i >= lens[b] * hop: the samples past an utterance's end (the generator's last kernel writes the valid ones only).  Round 5
// zero-filled the WHOLE [B][T * hop] buffer with hipMemsetAsync in front of every forward — 45 MB at B = 60, half of it about to be overwritten,
// through rocclr's generic fill kernel (51 us on average beside the other stream's kernels, up to 395 us: profiles/r05_h_kernel_trace.md).
__global__ void zero_wav_tails_kernel(float* wav, const int32_t* lens, int T, int hop) {
    const int b = blockIdx.y;
    const long long n = (long long)T * hop;
    int l = lens[b];
    l = l < 0 ? 0 : (l > T ? T : l);
    const long long first = (long long)l * hop;                       // (hop is a multiple of 4: 16-byte stores stay aligned)
    const long long i = first + ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) *(float4*)(wav + (long long)b * n + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    else for (long long k = i; k < n; ++k) wav[(long long)b * n + k] = 0.f;
}

} // namespace

// out[stage][b] = clamp(lens[b], 0, T) (T without lens) * mult.m[stage]: the valid rows of every utterance at every stage
extern "C" __global__ void scale_lens_kernel(const int32_t* lens, int32_t* out, int B, int T, int n_stage, StageMult mult) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n_stage) return;
    const int sidx = i / B, b = i % B;
    int l = lens ? lens[b] : T;
    l = l < 0 ? 0 : (l > T ? T : l);
    out[i] = l * mult.m[sidx];
}

namespace {

void scale_lens(const dtts_config& c, const int32_t* lens, int* lensS, int B, int T, hipStream_t s) {   // lensS: [n_upsamples + 1][B]
    const int nup = c.n_upsamples;
    StageMult mult;
    mult.m[0] = 1;
    for (int i = 0; i < nup; ++i) mult.m[i + 1] = mult.m[i] * c.upsample_rates[i];
    hipLaunchKernelGGL(scale_lens_kernel, dim3((B * (nup + 1) + 255) / 256), dim3(256), 0, s, lens, lensS, B, T, nup + 1, mult);
}

// ---------------------------------------------------------------------------------------------------------
// HifiGAN, the 16-bit modes: vconv kernels for the serial convolutions, one kernel per ResBlock (rblock / rb2x) or per ResBlock iteration
// (vpair) where one exists.  Every activation can exist twice: the fp32 residual stream and the bf16 leaky_relu copy the next convolution
// consumes (written by the producer's epilogue; bf16 mode, per-convolution path only).

// how ResBlock rb (= stage * n_resblock_kernels + j) of a C = ch stage runs.  fuse = false: per-convolution kernels everywhere
enum RbPath { RB_WHOLE, RB_VPAIR, RB_CONVS };   // rblock.hip / rbn.hip / rb2x.hip; vpair.hip (ResBlock1 only); vconv, convolution by convolution
RbPath rb_path(const dtts_ctx* h, bool fuse, int ch, size_t rb) {
    if (fuse && !h->rbf1[rb].empty()) return RB_WHOLE;
    if (h->resblock2) return RB_CONVS;
    const auto& c1 = h->rb1[rb];
    return fuse && vpair_runs(h->cfg, false, c1[0].engine, ch, c1[0].K, c1[0].dil, c1[1].dil, c1[2].dil) ? RB_VPAIR : RB_CONVS;
}

// Which stages run ALL their ResBlocks in one launch (rblock.hip; OPT-IN, tune bit 9 — measured: HBM traffic -0.36 MB / mel frame, vocoder
// alone +1.1 %, pipelined step +1.9 %: LABNOTES round 4): C <= 64, every ResBlock has a whole-ResBlock kernel, and the batch has at least
// two tiles per CU (small grids keep one launch per ResBlock: half-size tiles fill the chip there)
struct FusePlan {
    int fuse_n[8];    // ResBlocks in the stage's FIRST launch (1 = one launch per ResBlock)
    size_t s_elems;   // capacity of the stage-sum buffer
};
FusePlan fuse_plan(const dtts_ctx* h, const StageGeom& g, int B, bool fuse) {
    const dtts_config& c = h->cfg;
    const int nup = c.n_upsamples, nk = c.n_resblock_kernels;
    FusePlan pl = {{1, 1, 1, 1, 1, 1, 1, 1}, g.max_elems};
    for (int i = 0; i < nup; ++i) {
        const long long rows = g.rows[i + 1];
        const int ch = g.ch[i + 1];
        // (experiment, tune bit 12) C = 32 only: the first TWO ResBlocks in one launch — the k = 3 launch alone is HBM-bound (x in, stage sum out:
        // 4.6 TB/s), together with k = 7 its bytes ride on that launch's compute; the last ResBlock (fused conv_post) stays on its own
        if (h->resblock2) continue;   // (stage-fused launches, tune bits 9 / 12, exist for ResBlock1 only)
        if (fuse && DTTS_TUNE(h, 4096) && !DTTS_TUNE(h, 512) && nk == 3 && ch == 32 && !h->rbf1[(size_t)i * nk].empty() && !h->rbf1[(size_t)i * nk + 1].empty()) {
            int halo2 = 0;   // the launch's halo (rblock.h rblock_halo over its two ResBlocks)
            for (int j = 0; j < 2; ++j) halo2 = std::max(halo2, rblock_halo_of(h->rbf1[(size_t)i * nk + j][0].K, c.resblock_dilation_sizes[j]));
            const int TT2 = rblock_stage_tile_rows(ch, halo2);
            if (TT2 >= 64 && rblock_stage_launch_fits(ch, halo2, B, false) && (long long)B * ((rows + TT2 - 1) / TT2) >= 2LL * h->n_cu) pl.fuse_n[i] = 2;
            continue;
        }
        bool all = fuse && DTTS_TUNE(h, 512) && nk >= 2 && nk <= 3 && (ch == 32 || ch == 64);
        int halo = 0;
        for (int j = 0; j < nk && all; ++j) {
            all = !h->rbf1[(size_t)i * nk + j].empty();
            if (all) halo = std::max(halo, rblock_halo_of(h->rbf1[(size_t)i * nk + j][0].K, c.resblock_dilation_sizes[j]));
        }
        if (!all) continue;
        const bool with_post = i == nup - 1 && h->post_w;
        const int TT = rblock_stage_tile_rows(ch, halo);
        if (TT < 64 || !rblock_stage_launch_fits(ch, halo, B, with_post) || (long long)B * ((rows + TT - 1) / TT) < 2LL * h->n_cu) continue;
        if (with_post) {   // with the fused conv_post the tiles overlap: one private strip of the stage sum per tile
            const long long prow = rblock_private_rows(ch, halo, B, (int)rows);
            if (prow <= 0 || (size_t)prow * ch * sizeof(float) >= (size_t)INT_MAX) continue;
            pl.s_elems = std::max(pl.s_elems, (size_t)prow * ch);
        }
        pl.fuse_n[i] = nk;
    }
    return pl;
}

typedef unsigned short bf;
constexpr int TV = DTTS_TIMER_VOC_CONV;
constexpr int N_CTR = 64;

// One forward's workspace and the stage it is in, with the ways to run a ResBlock of that stage: x = Xf (the upsampler's output) in, the
// stage sum Sf (and, bf16 mode, its leaky_relu copy Sa behind the stage's last ResBlock) out
struct VocRun {
    dtts_ctx* h;
    hipStream_t s;
    int B, nk;
    bool exact;       // DTTS_VOC_F16: fp32 tensors between kernels (no 16-bit copies), serial convolutions on split operands, ResBlock
    int el;           // kernels on fp16 operands
    float* wav;
    float *Xf, *Rf, *Sf, *Rg;   // Rg: second ping-pong buffer of the fused-iteration path (vpair.hip)
    bf *Xa, *Ra, *Ta, *Sa;
    unsigned* ctrs;   // one tile counter per launch of a persistent kernel (vpair / rblock / rb2x: dynamic tile claiming), zeroed once per forward
    int n_ctr;
    size_t s_cap_bytes;
    bool post_done;   // conv_post + tanh ran in the epilogue of the last ResBlock kernel
    // ---- the stage
    int i, ch, Tcur;
    const int* lout;  // valid rows per utterance
    bool last_stage;

    // what RBlockParams and RB2xParams have in common.  j .. j_last: the ResBlocks of the launch (one unless the stage is fused)
    template <class P>
    void whole_rb_params(P& rp, int j, int j_last) {
        memset(&rp, 0, sizeof rp);
        rp.x = Xf;
        rp.S = Sf;
        rp.lens = lout;
        rp.B = B;
        rp.T = Tcur;
        rp.mode = j == 0 ? 0 : (j == nk - 1 ? 2 : 1);
        rp.div = (float)nk;
        rp.slope = last_stage ? 0.01f : 0.1f;
        rp.Sa = exact ? nullptr : Sa;
        rp.drop_S = exact ? 0 : 1;   // bf16 mode: after a stage only its bf16 leaky_relu copy is consumed (by ups[i+1] / conv_post)
        if (last_stage && j_last == nk - 1 && h->post_w) {   // conv_post + tanh in this kernel's epilogue: the stage output stays on chip
            rp.wav = wav;
            rp.post_w = h->post_w;
            rp.post_b = h->post_b;
            rp.Sa = nullptr;
            post_done = true;
        }
        rp.el = el;
        rp.tile_ctr = n_ctr < N_CTR ? ctrs + n_ctr++ : nullptr;
        rp.ovf = (exact && h->guard_on) ? h->ovf_dev : nullptr;
        rp.bad = h->bad_dev;
    }

    // whole ResBlock1 in one kernel (rblock.hip).  fuse_n > 1 (FusePlan): the stage's first fuse_n ResBlocks in ONE launch (work items (tile,
    // ResBlock)): x crosses HBM once per tile and the stage sum is accumulated through L2 / Infinity Cache
    int rblock(int j, int fuse_n) {
        if (nk == 1) return fail(h, DTTS_E_INVAL, "fused ResBlock path needs >= 2 resblock kernels");
        if (j > 0 && j < fuse_n) return DTTS_OK;   // (launched with j = 0)
        const int j_last = j == 0 ? fuse_n - 1 : j;
        RBlockParams rp;
        whole_rb_params(rp, j, j_last);
        rp.nrb = j_last - j + 1;
        rp.last_mode = j_last == nk - 1 ? 2 : 1;
        int frag = 0;
        for (int jj = j; jj <= j_last; ++jj) {
            RBlockParams::Set& st = rp.rb[jj - j];
            const auto& g1 = h->rbf1[(size_t)i * nk + jj];
            const auto& g2 = h->rbf2[(size_t)i * nk + jj];
            st.K = g1[0].K;
            st.Kp = rblock_padded_taps(ch, g1[0].K);
            // the order the launch's packs are in; a mixed set is in no kernel's order (0), and rblock_launch refuses whatever is not its kernel's
            if (jj == j) frag = g1[0].frag;
            for (int mth = 0; mth < 3; ++mth)
                if (g1[mth].frag != frag || g2[mth].frag != frag) frag = 0;
            for (int mth = 0; mth < 3; ++mth) {
                st.w1[mth] = (const uint4*)g1[mth].w_hi;
                st.w2[mth] = (const uint4*)g2[mth].w_hi;
                st.b1[mth] = g1[mth].bias;
                st.b2[mth] = g2[mth].bias;
                st.dil[mth] = g1[mth].dil;
            }
            rp.K = std::max(rp.K, st.K);
        }
        // a fused stage with the fused conv_post: one private strip of S per tile (the tiles overlap)
        if (rp.wav && fuse_n == nk) rp.s_private = (int)std::min<size_t>(s_cap_bytes, (size_t)INT_MAX);
        rp.small_tile = DTTS_TUNE(h, 16384) ? 1 : 0;
        if (h->debug_misorder) frag = frag == 16 ? 32 : 16;   // (self-test of the launcher's refusal: dtts_config.debug_redzone = 2)
        Timed tm(h, TV, s);
        LAUNCH(rblock_launch(rp, ch, frag, s));
        return DTTS_OK;
    }

    // whole ResBlock1 of a narrow stage (C = 16 / 8) in one kernel (rbn.hip); tune bits 9 / 12 / 14 / 15 have no meaning here
    int rbn(int j) {
        const auto& g1 = h->rbf1[(size_t)i * nk + j];
        const auto& g2 = h->rbf2[(size_t)i * nk + j];
        RBnParams rp;
        whole_rb_params(rp, j, j);
        rp.K = g1[0].K;
        rp.Kp = rbn_padded_taps(ch, g1[0].K);
        int frag = g1[0].frag;   // the order the launch's packs are in; a mixed set is in no kernel's order (0)
        for (int mth = 0; mth < 3; ++mth) {
            if (g1[mth].frag != frag || g2[mth].frag != frag) frag = 0;
            rp.w1[mth] = (const uint4*)g1[mth].w_hi;
            rp.w2[mth] = (const uint4*)g2[mth].w_hi;
            rp.b1[mth] = g1[mth].bias;
            rp.b2[mth] = g2[mth].bias;
            rp.dil[mth] = g1[mth].dil;
        }
        if (h->debug_misorder) frag = 16;   // (self-test of the launcher's refusal: dtts_config.debug_redzone = 2)
        Timed tm(h, TV, s);
        LAUNCH(rbn_launch(rp, ch, frag, s));
        return DTTS_OK;
    }

    // whole ResBlock2 in one kernel (rb2x.hip); tune bits 9 / 12 / 15 have no meaning here
    int rb2x(int j) {
        const auto& fv = h->rbf1[(size_t)i * nk + j];
        RB2xParams rp;
        whole_rb_params(rp, j, j);
        rp.K = fv[0].K;
        rp.Kp = rblock_padded_taps(ch, fv[0].K);
        for (int m = 0; m < 2; ++m) {
            rp.w[m] = (const uint4*)fv[m].w_hi;
            rp.b[m] = fv[m].bias;
            rp.dil[m] = fv[m].dil;
        }
        Timed tm(h, TV, s);
        LAUNCH(rb2x_launch(rp, ch, s));
        return DTTS_OK;
    }

    // ResBlock1, one kernel per iteration (vpair.hip): fp32 stream in, fp32 stream out
    int vpair(int j) {
        const auto& c1 = h->rb1[(size_t)i * nk + j];
        const auto& c2 = h->rb2[(size_t)i * nk + j];
        for (int mth = 0; mth < 3; ++mth)   // (build_vocoder packed and checked them where vpair_runs holds)
            if (!vpair_pack_fits(c1[mth], ch, c1[0].K) || !vpair_pack_fits(c2[mth], ch, c1[0].K))
                return fail(h, DTTS_E_STATE, "resblock %d is not packed for vpair<%d>", i * nk + j, ch);
        const float* xin = Xf;
        for (int mth = 0; mth < 3; ++mth) {
            VPairParams vp;
            memset(&vp, 0, sizeof vp);
            vp.x = xin;
            vp.w1 = (const uint4*)c1[mth].w_hi;
            vp.w2 = (const uint4*)c2[mth].w_hi;
            vp.b1 = c1[mth].bias;
            vp.b2 = c2[mth].bias;
            vp.lens = lout;
            vp.B = B;
            vp.T = Tcur;
            vp.K = c1[mth].K;
            vp.dil = c1[mth].dil;
            vp.div = (float)nk;
            vp.slope = last_stage ? 0.01f : 0.1f;
            vp.el = el;
            vp.tile_ctr = n_ctr < N_CTR ? ctrs + n_ctr++ : nullptr;
            vp.ovf = (exact && h->guard_on) ? h->ovf_dev : nullptr;
            // round 6: the stream BETWEEN the three iterations is fp16 (DTTS_VOC_F16 only; tune bit 15: fp32 as in round 5).  fp16(x) is what the
            // next iteration's convolution operand was anyway; the residual add sees the rounded value (tools/precision_sim.py --stream:
            // waveform error 5.3e-5 -> 6.7e-5, gate 1e-4).  The ResBlock's RESULT (iteration 2) stays fp32.
            const bool s16 = exact && !DTTS_TUNE(h, 32768);
            vp.x16 = (s16 && mth > 0) ? 1 : 0;
            if (mth < 2) {
                vp.y = mth == 0 ? Rf : Rg;
                vp.mode = 1;
                vp.y16 = s16 ? 1 : 0;
            } else {
                vp.y = Sf;
                vp.mode = j == 0 ? 1 : (j == nk - 1 ? 3 : 2);
                vp.ya = exact ? nullptr : Sa;
                vp.drop_y = exact ? 0 : 1;   // bf16 mode: after a stage only its bf16 leaky_relu copy is consumed (by ups[i+1])
            }
            xin = vp.y;
            Timed tm(h, TV, s);
            LAUNCH(vpair_launch(vp, ch, s));
        }
        return DTTS_OK;
    }

    // a ResBlock convolution by convolution (vconv; bf16 mode only).  ResBlock1: xt = c1(leaky_relu(x)), x = c2(leaky_relu(xt)) + x, three times;
    // ResBlock2: x = c(leaky_relu(x)) + x, twice
    int convs(int j) {
        if (exact) return fail(h, DTTS_E_STATE, "DTTS_VOC_F16: resblock %d has no fused kernel", i * nk + j);   // build_vocoder rejects such configs
        const auto& c1 = h->rb1[(size_t)i * nk + j];
        if (c1[0].frag != 32) return fail(h, DTTS_E_STATE, "resblock %d is packed for vpair, not for the per-convolution kernels", i * nk + j);   // (vpair_runs decides both)
        const int n = h->resblock2 ? 2 : 3;
        for (int mth = 0; mth < n; ++mth) {
            const bf* xa = mth == 0 ? Xa : Ra;
            if (!h->resblock2) {   // only leaky_relu(xt) in bf16 is ever consumed
                VConvParams p = vparams(c1[mth], xa, lout, B, Tcur);
                p.ldx = ch;    // (the activations are [T][ch]; below 32 channels the pack's C_in_pad is wider than the rows)
                p.ya = Ta;
                p.ldya = ch;
                p.slope = 0.1f;
                Timed tm(h, TV, s);
                LAUNCH(vconv_launch(p, s));
                xa = Ta;
            }
            VConvParams p = vparams(h->resblock2 ? c1[mth] : h->rb2[(size_t)i * nk + j][mth], xa, lout, B, Tcur);
            p.ldx = ch;
            p.res = mth == 0 ? Xf : Rf;
            p.ldres = ch;
            if (mth < n - 1) {
                p.yf = Rf;
                p.ldyf = ch;
                p.ya = Ra;
                p.ldya = ch;
                p.slope = 0.1f;
            } else {   // xs (+)= x ; the last resblock also applies / num_kernels and emits the next stage's input
                p.yf = Sf;
                p.ldyf = ch;
                if (j > 0) {
                    p.res2 = Sf;
                    p.ldres2 = ch;
                }
                if (j == nk - 1) {
                    p.div = (float)nk;
                    p.ya = Sa;
                    p.ldya = ch;
                    p.slope = last_stage ? 0.01f : 0.1f;  // F.leaky_relu default before conv_post (hifigan.py:138)
                }
            }
            Timed tm(h, TV, s);
            LAUNCH(vconv_launch(p, s));
        }
        return DTTS_OK;
    }
};

int hifigan_forward_fused(dtts_ctx* h, const float* mel, const int32_t* lens, int B, int T, float* wav, hipStream_t s) {
    const dtts_config& c = h->cfg;
    const bool exact = c.vocoder_precision == DTTS_VOC_F16;
    const int nup = c.n_upsamples, nk = c.n_resblock_kernels;
    const int melC = h->conv_pre.C_in_pad;
    const bool fuse = exact || !c.vocoder_unfused;   // vocoder_unfused: per-convolution kernels (a testing aid of the bf16 mode)
    const StageGeom g = stage_geom(c, B, T);
    const FusePlan plan = fuse_plan(h, g, B, fuse);
    const size_t max_elems = g.max_elems, s_elems = plan.s_elems;
    // ---- workspace
    HIPCHK(h->a_voc.reserve((s_elems - max_elems) * sizeof(float) + max_elems * (4 * sizeof(float) + 4 * sizeof(bf)) + (size_t)B * T * melC * sizeof(bf) +
                            (size_t)(nup + 2) * B * sizeof(int) + (64 << 10), s));
    Arena& A = h->a_voc;
    VocRun r = {h, s, B, nk, exact, exact ? EL_F16 : EL_BF16, wav};
    r.s_cap_bytes = s_elems * sizeof(float);
    float* Xf = r.Xf = A.alloc<float>(max_elems);
    r.Rf = A.alloc<float>(max_elems);
    float* Sf = r.Sf = A.alloc<float>(s_elems);
    r.Rg = A.alloc<float>(max_elems);
    bf* Xa = r.Xa = A.alloc<bf>(max_elems);
    r.Ra = A.alloc<bf>(max_elems);
    r.Ta = A.alloc<bf>(max_elems);
    bf* Sa = r.Sa = A.alloc<bf>(max_elems);
    bf* melb = A.alloc<bf>((size_t)B * T * melC);
    int* lensS = A.alloc<int>((size_t)(nup + 1) * B);
    r.ctrs = A.alloc<unsigned>(N_CTR);
    if (!Xf || !r.Rf || !Sf || !r.Rg || !Xa || !r.Ra || !r.Ta || !Sa || !melb || !lensS || !r.ctrs) return fail(h, DTTS_E_NOMEM, "vocoder workspace");
    HIPCHK(hipMemsetAsync(r.ctrs, 0, N_CTR * sizeof(unsigned), s));
    // ---- lengths per stage; samples past an utterance's end are zero (no lens: every sample is a valid one and is written below)
    scale_lens(c, lens, lensS, B, T, s);
    if (lens && (h->hop & 3) == 0 && ((uintptr_t)wav & 15) == 0) {
        const long long n = (long long)T * h->hop;
        hipLaunchKernelGGL(zero_wav_tails_kernel, dim3((unsigned)((n / 4 + 255) / 256), B), dim3(256), 0, s, wav, lens, T, h->hop);
        HIPCHK(hipGetLastError());
    } else if (lens) HIPCHK(hipMemsetAsync(wav, 0, (size_t)B * T * h->hop * sizeof(float), s));
    // The family's launches are consecutive on the stream (nothing else runs between conv_pre and the last ResBlock / conv_post): ONE
    // hipEvent pair per forward spans them all — the per-launch pairs of round 2 put 50 event packets between the kernels of every forward.
    // The span includes the kernel boundaries; launches are still counted one by one.
    struct SpanGuard {
        dtts_ctx* h;
        Timed* t;
        ~SpanGuard() {
            h->voc_span = false;
            delete t;   // closes the span (records the end event)
        }
    } span{h, nullptr};
    if (h->timers[TV].enabled) {
        span.t = new Timed(h, TV, s);
        if (span.t->e1) h->timers[TV].launches -= 1;   // (the span itself is not a launch; e1 is null when no event could be created)
        h->voc_span = true;
    }
    // ---- conv_pre
    if (exact) {   // mel fp32 in, fp32 out
        VConvParams p = vparams_x3(h->conv_pre, mel, c.audio_num_mel_bins, 1.f, lensS, B, T);
        p.yf = Sf;
        p.ldyf = g.ch[0];
        Timed tm(h, TV, s);
        LAUNCH(vconv_launch(p, s));
    } else {   // only its leaky_relu(0.1) bf16 copy is consumed (by ups[0])
        LAUNCH(f32_to_bf16_pad_launch(mel, melb, (long long)B * T, c.audio_num_mel_bins, melC, s));
        VConvParams p = vparams(h->conv_pre, melb, lensS, B, T);
        p.ya = Sa;
        p.ldya = g.ch[0];
        p.slope = 0.1f;
        Timed tm(h, TV, s);
        LAUNCH(vconv_launch(p, s));
    }
    // ---- the stages: upsampler, then the ResBlocks
    for (int i = 0; i < nup; ++i) {
        const int u = c.upsample_rates[i], ch = g.ch[i + 1], Tin = (int)g.rows[i];
        const int* lin = lensS + (size_t)i * B;
        // the bf16 leaky_relu copy of the stage input is consumed only by the per-convolution fallback: the fused kernels
        // (vpair, rblock, rb2x) read the fp32 stream and round it themselves
        bool need_xa = false;
        for (int j = 0; j < nk; ++j) need_xa = need_xa || rb_path(h, fuse, ch, (size_t)i * nk + j) == RB_CONVS;
        {   // ups[i] (polyphase): Sa [B,Tin,2ch] -> Xf / Xa [B,Tin,u*ch] == [B,Tin*u,ch]
            VConvParams p = exact ? vparams_x3(h->ups[i], Sf, 2 * ch, 0.1f, lin, B, Tin) : vparams(h->ups[i], Sa, lin, B, Tin);
            if (!exact) p.ldx = 2 * ch;   // Sa is [T][2 ch] (= C_in_pad except below 32 channels)
            p.small_tiles = exact;   // narrow split-operand upsamplers: 64-row tiles, 4 workgroups / CU (-0.15 ms same-box)
            p.yf = Xf;
            p.ldyf = u * ch;
            p.ya = need_xa ? Xa : nullptr;
            p.ldya = u * ch;
            p.slope = 0.1f;
            Timed tm(h, TV, s);
            LAUNCH(vconv_launch(p, s));
        }
        r.i = i;
        r.ch = ch;
        r.Tcur = (int)g.rows[i + 1];
        r.lout = lensS + (size_t)(i + 1) * B;
        r.last_stage = i == nup - 1;
        for (int j = 0; j < nk; ++j) {
            const RbPath path = rb_path(h, fuse, ch, (size_t)i * nk + j);
            const bool narrow = path == RB_WHOLE && !h->resblock2 && h->rbf1[(size_t)i * nk + j][0].frag == RBN_FRAG;
            const int rc = path == RB_WHOLE ? (h->resblock2 ? r.rb2x(j) : (narrow ? r.rbn(j) : r.rblock(j, plan.fuse_n[i])))
                                            : (path == RB_VPAIR ? r.vpair(j) : r.convs(j));
            if (rc) return rc;
        }
    }
    if (!r.post_done) {   // wav = tanh(conv_post(leaky_relu(x, 0.01)))
        const int Tcur = (int)g.rows[nup], ch = g.ch[nup];
        VConvParams p = exact ? vparams_x3(h->conv_post, Sf, ch, 0.01f, lensS + (size_t)nup * B, B, Tcur)
                              : vparams(h->conv_post, Sa, lensS + (size_t)nup * B, B, Tcur);
        if (!exact) p.ldx = ch;
        p.yf = wav;
        p.ldyf = 1;
        p.post_tanh = 1;
        p.bad = h->bad_dev;
        Timed tm(h, TV, s);
        LAUNCH(vconv_launch(p, s));
    }
    return DTTS_OK;
}

// ---------------------------------------------------------------------------------------------------------
// HifiGAN, DTTS_VOC_BF16X3: every convolution on the generic kernel (conv1d.hip) with hi / lo split operands, fp32 tensors between them
int hifigan_forward_x3(dtts_ctx* h, const float* mel, const int32_t* lens, int B, int T, float* wav, hipStream_t s) {
    const dtts_config& c = h->cfg;
    const int nup = c.n_upsamples, nk = c.n_resblock_kernels;
    const size_t max_elems = stage_geom(c, B, T).max_elems;
    HIPCHK(h->a_voc.reserve(4 * (max_elems * sizeof(float) + 256) + (size_t)(nup + 2) * B * sizeof(int) + 8192, s));
    float* bufX = h->a_voc.alloc<float>(max_elems);
    float* bufR = h->a_voc.alloc<float>(max_elems);
    float* bufT = h->a_voc.alloc<float>(max_elems);
    float* bufS = h->a_voc.alloc<float>(max_elems);
    int* lensS = h->a_voc.alloc<int>((size_t)(nup + 1) * B);
    if (!bufX || !bufR || !bufT || !bufS || !lensS) return fail(h, DTTS_E_NOMEM, "vocoder workspace");
    scale_lens(c, lens, lensS, B, T, s);
    // conv_pre: mel [B,T,80] -> S [B,T,512]
    int Tcur = T, ch = c.upsample_initial_channel;
    {
        ConvParams p = base_params(mel, c.audio_num_mel_bins, B, T, T, bufS, ch);
        p.in_lens = lensS;
        p.out_lens = lensS;
        Timed tm(h, TV, s);
        LAUNCH(conv1d_launch(h->conv_pre, p, s));
    }
    for (int i = 0; i < nup; ++i) {
        const int u = c.upsample_rates[i];
        const int* lin = lensS + (size_t)i * B;
        const int* lout = lensS + (size_t)(i + 1) * B;
        ch /= 2;
        {   // x = ups[i](leaky_relu(x, 0.1)) as a polyphase convolution: [B,Tcur,2ch] -> [B,Tcur,u*ch] == [B,Tcur*u,ch]
            ConvParams p = base_params(bufS, 2 * ch, B, Tcur, Tcur, bufX, u * ch);
            p.in_lens = lin;
            p.out_lens = lin;
            p.pre_act = 1;
            p.pre_slope = 0.1f;
            Timed tm(h, TV, s);
            LAUNCH(conv1d_launch(h->ups[i], p, s));
        }
        Tcur *= u;
        // y = c(leaky_relu(xin)) (+ res); the last convolution of a ResBlock also folds xs (+)= x, and the stage's last one the / num_kernels
        auto conv = [&](const PackedConv& L, const float* xin, const float* res, float* y, bool last, int j) -> int {
            ConvParams p = base_params(xin, ch, B, Tcur, Tcur, y, ch);
            p.in_lens = lout;
            p.out_lens = lout;
            p.pre_act = 1;
            p.pre_slope = 0.1f;
            if (res) set_res(p, 0, res, ch);
            if (last && j > 0) {
                p.seg[0].res2 = bufS;
                p.seg[0].ld_res2 = ch;
            }
            if (last && j == nk - 1) p.out_div = (float)nk;
            Timed tm(h, TV, s);
            LAUNCH(conv1d_launch(L, p, s));
            return DTTS_OK;
        };
        for (int j = 0; j < nk; ++j) {
            const auto& c1 = h->rb1[(size_t)i * nk + j];
            const int n = h->resblock2 ? 2 : 3;
            for (int mth = 0; mth < n; ++mth) {
                const float* xin = mth == 0 ? bufX : bufR;
                const bool last = mth == n - 1;
                // ResBlock1: xt = c1(leaky_relu(x)), x = c2(leaky_relu(xt)) + x ; ResBlock2: x = c(leaky_relu(x)) + x
                if (!h->resblock2)
                    if (int rc = conv(c1[mth], xin, nullptr, bufT, false, j)) return rc;
                const PackedConv& L = h->resblock2 ? c1[mth] : h->rb2[(size_t)i * nk + j][mth];
                if (int rc = conv(L, h->resblock2 ? xin : bufT, xin, last ? bufS : bufR, last, j)) return rc;
            }
        }
    }
    {   // x = tanh(conv_post(leaky_relu(x)))   (default slope 0.01, hifigan.py:138)
        const int* lout = lensS + (size_t)nup * B;
        ConvParams p = base_params(bufS, ch, B, Tcur, Tcur, wav, 1);
        p.in_lens = lout;
        p.out_lens = lout;
        p.zero_masked = 1;
        p.pre_act = 1;
        p.pre_slope = 0.01f;
        p.post_act = 2;
        Timed tm(h, TV, s);
        LAUNCH(conv1d_launch(h->conv_post, p, s));
    }
    return DTTS_OK;
}

} // namespace

extern "C" {

int dtts_hifigan_hop(dtts_handle h) { return h ? h->hop : 0; }

int dtts_wav_to_int16(dtts_handle h, const float* wav, const int32_t* lens, int B, int T, int norm, int16_t* out, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    if (!h->vocoder_ready) return fail(h, DTTS_E_STATE, "vocoder weights not finalized");
    if (!wav || !out || B <= 0 || T <= 0) return fail(h, DTTS_E_INVAL, "dtts_wav_to_int16: bad argument");
    hipStream_t s = (hipStream_t)stream;
    if (!h->amax_bits || h->amax_cap < B) {   // tiny persistent scratch, grown outside the steady state
        if (h->amax_bits) {
            HIPCHK(hipDeviceSynchronize());
            (void)hipFree(h->amax_bits);
            h->amax_bits = nullptr;
        }
        HIPCHK(hipMalloc((void**)&h->amax_bits, sizeof(unsigned) * std::max(B, 256)));
        h->amax_cap = std::max(B, 256);
    }
    LAUNCH(wav_to_int16_launch(wav, lens, h->hop, B, (long long)T * h->hop, norm, h->amax_bits, out, s));
    return DTTS_OK;
}

int dtts_hifigan_forward(dtts_handle h, const float* mel, const int32_t* lens, int B, int T, float* wav, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    if (!h->vocoder_ready) return fail(h, DTTS_E_STATE, "vocoder weights not finalized");
    if (!mel || !wav || B <= 0 || T <= 0) return fail(h, DTTS_E_INVAL, "dtts_hifigan_forward: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const dtts_config& c = h->cfg;
    Timed t_voc(h, DTTS_TIMER_STAGE_HIFIGAN, s);   // 'hifigan' (vocoders/hifigan.py:59): the generator forward
    if (c.vocoder_precision != DTTS_VOC_BF16X3) {
        // the fused kernels' persistent workgroups keep a per-utterance tile table (12 B per utterance) in LDS beside their tiles
        if (B > DTTS_MAX_VOCODER_BATCH) return fail(h, DTTS_E_INVAL, "dtts_hifigan_forward: B = %d exceeds %d utterances per call", B, DTTS_MAX_VOCODER_BATCH);
        if (c.vocoder_precision == DTTS_VOC_F16 && ((uintptr_t)mel & 15))
            return fail(h, DTTS_E_INVAL, "dtts_hifigan_forward: DTTS_VOC_F16 reads mel with 16-byte loads: the pointer must be 16-byte aligned");
        const int rc = hifigan_forward_fused(h, mel, lens, B, T, wav, s);
        // the detector's count follows the forward's last kernel into pinned host memory: whoever synchronises with this stream to read the
        // waveform can read it (dtts_vocoder_nonfinite) without another synchronisation
        if (rc == DTTS_OK && h->bad_dev && h->bad_host) HIPCHK(hipMemcpyAsync((void*)h->bad_host, h->bad_dev, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        return rc;
    }
    return hifigan_forward_x3(h, mel, lens, B, T, wav, s);
}

int dtts_vocoder_range_guard(dtts_handle h, int enable) {
    if (!h) return DTTS_E_INVAL;
    if (enable && h->cfg.vocoder_precision != DTTS_VOC_F16) return fail(h, DTTS_E_INVAL, "the range guard exists for DTTS_VOC_F16 only (the other modes have fp32's exponent range)");
    h->guard_on = enable != 0;
    return DTTS_OK;
}

int dtts_vocoder_clamped(dtts_handle h, int64_t* count, int reset, dtts_stream stream) {
    if (!h || !count) return DTTS_E_INVAL;
    if (!h->ovf_dev) return fail(h, DTTS_E_STATE, "vocoder weights not finalized");
    unsigned long long v = 0;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(&v, h->ovf_dev, sizeof v, hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(h->ovf_dev, 0, sizeof v, s));
    HIPCHK(hipStreamSynchronize(s));
    *count = (int64_t)v;
    return DTTS_OK;
}

int dtts_vocoder_nonfinite(dtts_handle h, int64_t* count) {
    if (!h || !count) return DTTS_E_INVAL;
    if (!h->vocoder_ready) return fail(h, DTTS_E_STATE, "vocoder weights not finalized");
    *count = h->bad_host ? (int64_t)*h->bad_host : 0;
    return DTTS_OK;
}

int dtts_vocoder_fp16_bound(dtts_handle h, float mel_abs_max, double* worst_case, double* rms_estimate) {
    if (!h || !(mel_abs_max >= 0.f)) return DTTS_E_INVAL;
    if (!h->vocoder_ready) return fail(h, DTTS_E_STATE, "vocoder weights not finalized");
    const bool f16 = h->cfg.vocoder_precision == DTTS_VOC_F16;
    if (worst_case) *worst_case = f16 ? h->wc_const + h->wc_lin * (double)mel_abs_max : 0.0;
    if (rms_estimate) *rms_estimate = f16 ? std::sqrt(h->est_const * h->est_const + h->est_lin * h->est_lin * (double)mel_abs_max * mel_abs_max) : 0.0;
    return DTTS_OK;
}

} // extern "C"
