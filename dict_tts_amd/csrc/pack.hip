// libdicttts_hip.so — host side of the weights: device allocations owned by the context, number conversion, weight-norm folding, packing
// into MFMA fragment order (the format conv1d.hip / vconv.hip read), and the parameter blocks built from a pack.
#include "ctx.h"

namespace dtts {

// device allocation owned by the context (freed by dtts_destroy / dev_free); debug_redzone: between two 0xFF red zones
void* dev_alloc(dtts_ctx* h, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    char* d = nullptr;
    if (!h->debug_rz) {
        if (hipMalloc((void**)&d, bytes) != hipSuccess) return nullptr;
        h->allocs.push_back(d);
        return d;
    }
    const size_t padded = (bytes + 255) & ~(size_t)255;
    if (hipMalloc((void**)&d, padded + 2 * RZ) != hipSuccess) return nullptr;
    h->allocs.push_back(d);
    if (hipMemset(d, 0xFF, padded + 2 * RZ) != hipSuccess) return nullptr;
    h->rz_static.push_back({d + RZ, bytes});
    return d + RZ;
}
void dev_free(dtts_ctx* h, void* user) {
    if (!user) return;
    char* basep = (char*)user - (h->debug_rz ? RZ : 0);
    auto it = std::find(h->allocs.begin(), h->allocs.end(), (void*)basep);
    if (it == h->allocs.end()) return;
    (void)hipFree(basep);
    h->allocs.erase(it);
    for (size_t i = 0; i < h->rz_static.size(); ++i)
        if (h->rz_static[i].p == (char*)user) {
            h->rz_static.erase(h->rz_static.begin() + i);
            break;
        }
}

namespace {

uint16_t f2bf_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float bf2f_host(uint16_t hbits) {
    uint32_t u = (uint32_t)hbits << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// fp32 -> IEEE half bits, round-to-nearest-even, saturating at the largest finite half (weights never get there)
uint16_t f2h_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    const uint32_t a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | (a > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7bffu);            // >= 65520 rounds past the largest finite half: saturate
    if (a < 0x33000001u) return (uint16_t)sign;                          // <= 2^-25: rounds to zero
    const int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;                            // 24-bit significand
    int shift = e >= -14 ? 13 : 13 + (-14 - e);                          // bits dropped (subnormal halves drop more)
    const uint32_t half_ulp = 1u << (shift - 1), rem = m & ((1u << shift) - 1);
    uint32_t q = m >> shift;
    if (rem > half_ulp || (rem == half_ulp && (q & 1u))) ++q;
    uint32_t out = e >= -14 ? (((uint32_t)(e + 15) << 10) + (q - 0x400u)) : q;   // a carry out of the significand bumps the exponent
    return (uint16_t)(sign | out);
}

} // namespace

// Pack one convolution into MFMA fragment order and upload it.  getw(co, ci, tap) addresses the LOGICAL
// weight; bias is in logical channel order.  gate_H > 0: logical C_out = 2*gate_H, packed co-tiles
// alternate (tanh[32j..32j+32), sigmoid[H+32j..H+32j+32)).
// frag: the fragment order.  32 (every kernel but vpair.hip and rblock.hip at C = 64): the A operand of v_mfma_f32_32x32x16 — per (tap, kg-channel group, co-tile)
// 64 lanes x kg / 2 elements, lane = 32 * half + co % 32, ci = kg * g + (kg / 2) * half + e.  16 (16-bit engines only; rb_common.h:
// MfmaShape<16>): the A operand of v_mfma_f32_16x16x32 — per (tap, 32-channel group, co-tile, co half) 64 lanes x 8 elements,
// lane = 16 * kq + co % 16, ci = 32 * g + 8 * kq + e.  Both orders have the same size, slack included.
// RBN_FRAG (rbn.h; 16-bit engines, C_in = C_out = 16 or 8, K whole k-steps of 32 / C taps): the A operand of v_mfma_f32_16x16x32 with the taps folded
// into the contraction index — per k-step 64 lanes x 8 elements, lane = 16 * kq + co, k = 8 * kq + e = (tap % (32 / C)) * C + ci; no slack (rbn.hip
// copies exactly the pack to LDS).
bool pack_conv(dtts_ctx* h, PackedConv& L, int engine, int C_out, int C_in, int K,
               const std::function<float(int, int, int)>& getw, const std::vector<float>& bias, int dil, int stride,
               int pad, int gate_H, double flops_per_row, int frag) {
    const bool folded = frag == RBN_FRAG;
    if (folded && (C_in != C_out || (C_in != 16 && C_in != 8) || K % rbn_taps_per_step(C_in) || gate_H)) return false;
    if (frag != 32 && ((frag != 16 && !folded) || engine == ENG_F32 || engine == ENG_BF16X3)) return false;
    L.engine = engine;
    L.frag = frag;
    L.C_in = C_in;
    L.C_out = C_out;
    L.K = K;
    L.dil = dil;
    L.stride = stride;
    L.pad = pad;
    L.gate_H = gate_H;
    L.CK = (C_in <= 32) ? 32 : 64;
    L.C_in_pad = (C_in + L.CK - 1) / L.CK * L.CK;
    L.C_out_pad = (C_out + 31) / 32 * 32;
    if (frag == 16 && L.C_in_pad % 32) return false;   // whole 32-channel k-steps
    L.flops_per_row = flops_per_row >= 0 ? flops_per_row : 2.0 * C_out * C_in * K;
    const int KG = engine == ENG_F32 ? 8 : 16, NCT = L.C_out_pad / 32;
    // + zero k-steps of slack behind the last tap: the kernels prefetch weight fragments past the end instead of clamping.  vconv walks
    // one C_in CHUNK at a time and, at the end of a chunk's last tap, its running pointer wraps to "next tap, same chunk" = up to a whole
    // tap's k-groups (NG) beyond the end for the last chunk (found in round 3: the 192 -> 2048 conditioning convolution read one
    // 64 KB step past the old 8-step slack — a GPU page fault whenever the allocation ended on a mapped-region boundary)
    const size_t n = folded ? (size_t)(K / rbn_taps_per_step(C_in)) * 512
                            : (size_t)K * L.C_in_pad * L.C_out_pad + (size_t)(L.C_in_pad / 16 + 8) * 16 * L.C_out_pad;
    // put(fragment index, logical weight) for every weight, with k-groups of kg input channels
    auto each_weight = [&](int kg, auto&& put) {
        const int E = kg / 2, NG = L.C_in_pad / kg;
        for (int pco = 0; pco < L.C_out_pad; ++pco) {
            int co = pco;
            if (gate_H) {
                const int tile = pco / 32, j = tile / 2, within = pco % 32;
                co = (tile & 1) ? gate_H + j * 32 + within : j * 32 + within;
                if (j * 32 + within >= gate_H) co = -1;
            }
            if (co < 0 || co >= C_out) continue;
            const int ct = pco / 32, col = pco % 32;
            for (int tap = 0; tap < K; ++tap)
                for (int ci = 0; ci < C_in; ++ci) {
                    if (folded) {
                        const int tps = rbn_taps_per_step(C_in), k = (tap % tps) * C_in + ci;
                        put((((size_t)(tap / tps) * 64 + k / 8 * 16 + co) * 8) + k % 8, getw(co, ci, tap));
                        continue;
                    }
                    if (frag == 16) {   // (kg = 16, C_in_pad % 32 == 0)
                        const int g = ci / 32, kq = ci % 32 / 8, e = ci % 8;
                        put((((((size_t)tap * (L.C_in_pad / 32) + g) * NCT + ct) * 2 + col / 16) * 64 + kq * 16 + col % 16) * 8 + e, getw(co, ci, tap));
                        continue;
                    }
                    const int g = ci / kg, within = ci % kg, half = within / E, e = within % E;
                    put(((((size_t)tap * NG + g) * NCT + ct) * 64 + half * 32 + col) * E + e, getw(co, ci, tap));
                }
        }
    };
    std::vector<float> wf;
    std::vector<uint16_t> whi, wlo;
    if (engine == ENG_F32) wf.assign(n, 0.f);
    else {
        whi.assign(n, 0);
        if (engine == ENG_BF16X3) wlo.assign(n, 0);
    }
    each_weight(KG, [&](size_t idx, float v) {
        if (engine == ENG_F32) wf[idx] = v;
        else if (engine == ENG_F16) whi[idx] = f2h_host(v);
        else {
            const uint16_t hi = f2bf_host(v);
            whi[idx] = hi;
            if (engine == ENG_BF16X3) wlo[idx] = f2bf_host(v - bf2f_host(hi));
        }
    });
    if (engine == ENG_F32) {
        L.w_hi = upload(h, wf);
        // + the same weights as three bf16 pieces in k-groups of 16 (conv1d.h: ENG_BF16X6) for the short-sequence kernel
        if (L.C_in_pad % 16 == 0) {
            std::vector<uint16_t> pc[3];
            for (auto& v : pc) v.assign(n, 0);
            each_weight(16, [&](size_t idx, float r) {
                for (int pl = 0; pl < 3; ++pl) {
                    const uint16_t b16 = f2bf_host(r);
                    pc[pl][idx] = b16;
                    r -= bf2f_host(b16);   // exact: the remainder of a round-to-nearest bf16 fits fp32
                }
            });
            for (int pl = 0; pl < 3; ++pl) L.x6[pl] = upload(h, pc[pl]);
            if (!L.x6[0] || !L.x6[1] || !L.x6[2]) return false;
        }
    } else {
        L.w_hi = upload(h, whi);
        if (engine == ENG_BF16X3) L.w_lo = upload(h, wlo);
    }
    if (!bias.empty()) {
        std::vector<float> bp(bias);
        bp.resize(std::max<size_t>(bias.size(), (size_t)L.C_out_pad), 0.f);  // zero padded: 16 B loads in vconv's epilogue
        L.bias = upload(h, bp);
    }
    return L.w_hi != nullptr && (bias.empty() || L.bias != nullptr);
}

// fold weight norm if <base>.weight is absent: w = v * (g / ||v||), norm over all dims but 0
// (torch.nn.utils.weight_norm dim=0; remove_weight_norm at tasks/tts/ps_flow.py:262-268, hifigan.py:144-151)
const HostTensor* folded_weight(dtts_ctx* h, Need& need, const std::string& base) {
    auto it = h->w.find(base + ".weight");
    if (it != h->w.end()) return &it->second;
    const HostTensor* g = need.get(base + ".weight_g");
    const HostTensor* v = need.get(base + ".weight_v");
    if (!g || !v) return nullptr;
    HostTensor out;
    out.shape = v->shape;
    out.f.resize(v->f.size());
    const int64_t d0 = v->shape[0], inner = v->numel() / d0;
    for (int64_t i = 0; i < d0; ++i) {
        double ss = 0;
        for (int64_t j = 0; j < inner; ++j) ss += (double)v->f[i * inner + j] * v->f[i * inner + j];
        const float nrm = (float)std::sqrt(ss);
        const float sc = g->f[i] / nrm;
        for (int64_t j = 0; j < inner; ++j) out.f[i * inner + j] = v->f[i * inner + j] * sc;
    }
    auto& slot = h->w[base + ".weight"];
    slot = std::move(out);
    return &slot;
}

std::vector<float> bias_of(Need& need, const std::string& base) {
    const HostTensor* b = need.get(base + ".bias");
    return b ? b->f : std::vector<float>();
}

// ordinary Conv1d weight [C_out][C_in][K]
bool pack_plain(dtts_ctx* h, Need& need, PackedConv& L, int engine, const std::string& base, int dil, int stride, int pad,
                bool with_bias, int gate_H, int frag) {
    const HostTensor* w = folded_weight(h, need, base);
    if (!w) return false;
    const int C_out = (int)w->shape[0], C_in = (int)w->shape[1], K = w->shape.size() > 2 ? (int)w->shape[2] : 1;
    std::vector<float> bias = with_bias ? bias_of(need, base) : std::vector<float>();
    if (with_bias && bias.empty()) return false;
    const float* p = w->f.data();
    return pack_conv(h, L, engine, C_out, C_in, K,
                     [=](int co, int ci, int tap) { return p[((size_t)co * C_in + ci) * K + tap]; }, bias, dil, stride,
                     pad, gate_H, -1, frag);
}

// ConvTranspose1d weight [C_in][C_out][k], stride u, padding p -> polyphase Conv1d with u*C_out channels
// (phase-major), taps over input offsets {-1,0,+1} (or a single tap when k == u, p == 0):
// out[u*q + r] = sum_delta sum_ci x[q + delta][ci] * w[ci][co][r + p - u*delta]
bool pack_transposed(dtts_ctx* h, Need& need, PackedConv& L, int engine, const std::string& base, int u, int p) {
    const HostTensor* w = folded_weight(h, need, base);
    if (!w) return false;
    const int C_in = (int)w->shape[0], C_out = (int)w->shape[1], k = (int)w->shape[2];
    std::vector<float> b0 = bias_of(need, base);
    if (b0.empty()) return false;
    // Accepted: stride <= k <= 2 * stride with k - stride even and pad = (k - stride) / 2 — exactly T * stride output rows (what stage_geom,
    // scale_lens and the hop assume) and at most the three taps {-1, 0, +1}.  Refused in EVERY precision (the shape is wrong, not the arithmetic):
    // an odd k - stride (ConvTranspose1d then yields T * stride + 1 rows: the polyphase form would drop each stage's last row) and k < stride
    // ((k - stride) / 2 truncates toward zero in C; the reference's padding would be negative, which PyTorch refuses).
    if (u < 1 || k < u || k > 2 * u || (k - u) % 2 || 2 * p != k - u) {
        fail(h, DTTS_E_INVAL, "%s: unsupported transposed conv k=%d stride=%d pad=%d (accepted: stride <= k <= 2 * stride, k - stride even, pad = (k - stride) / 2)",
             base.c_str(), k, u, p);
        return false;
    }
    const bool single = (k == u && p == 0);
    const int K = single ? 1 : 3, pad = single ? 0 : 1;
    std::vector<float> bias((size_t)u * C_out);
    for (int r = 0; r < u; ++r)
        for (int co = 0; co < C_out; ++co) bias[(size_t)r * C_out + co] = b0[co];
    const float* pw = w->f.data();
    // k = 2u, pad = u/2 (HifiGAN's upsamplers): phase r < u/2 reads input offsets {-1, 0}, r >= u/2 reads {0, +1} — a third
    // of the 3-tap polyphase weights are structural zeros and the kernel skips them per wave (vconv.hip: poly_half)
    const int cop = u * C_out, wave_ch = (cop % 256 == 0) ? 64 : 32;   // channels per wave of the vconv configuration this layer gets
    const bool half = !single && k == 2 * u && 2 * p == u && (cop / 2) % wave_ch == 0;
    const bool ok = pack_conv(
        h, L, engine, u * C_out, C_in, K,
        [=](int pco, int ci, int tap) {
            const int r = pco / C_out, co = pco % C_out, delta = tap - pad;
            const int j = r + p - u * delta;
            return (j >= 0 && j < k) ? pw[((size_t)ci * C_out + co) * k + j] : 0.f;
        },
        bias, 1, 1, pad, 0, 2.0 * C_in * C_out * k /* per INPUT row: u outputs x k/u taps */);
    L.poly_half = half ? 1 : 0;
    return ok;
}

float* upload_named(dtts_ctx* h, Need& need, const std::string& name) {
    const HostTensor* t = need.get(name);
    return t ? upload(h, t->f) : nullptr;
}

// ---------------------------------------------------------------------------------------------------------
// vconv parameter blocks (vocoder convolutions and the decoder's split-operand WaveNet layers)
VConvParams vparams(const PackedConv& L, const unsigned short* x, const int* lens, int B, int T) {
    VConvParams p;
    memset(&p, 0, sizeof p);
    p.x = x;
    p.ldx = L.C_in_pad;
    p.w = (const uint4*)L.w_hi;
    p.bias = L.bias;
    p.lens = lens;
    p.B = B;
    p.T = T;
    p.C_in_pad = L.C_in_pad;
    p.C_out = L.C_out;
    p.C_out_pad = L.C_out_pad;
    p.K = L.K;
    p.dil = L.dil;
    p.pad = L.pad;
    p.slope = 1.f;
    p.div = 1.f;
    p.in_slope = 1.f;
    p.C_in = L.C_in;
    p.poly_half = L.poly_half;
    return p;
}
// waveform-exact form: fp32 input [B][T][ld] (leaky_relu(in_slope) applied while staging), hi/lo split operands
VConvParams vparams_x3(const PackedConv& L, const float* xf, int ld, float in_slope, const int* lens, int B, int T) {
    VConvParams p = vparams(L, nullptr, lens, B, T);
    p.xf = xf;
    p.ldx = ld;
    p.in_slope = in_slope;
    p.wlo = (const uint4*)L.w_lo;
    p.h2 = L.engine == ENG_F16 ? 1 : 0;
    return p;
}

// ---------------------------------------------------------------------------------------------------------
// conv1d parameter blocks
ConvParams base_params(const float* x, int ldx, int B, int T_in, int T_out, float* y, int ldy) {
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.x = x;
    p.ldx = ldx;
    p.x_bstride = (long long)T_in * ldx;
    p.B = B;
    p.T_in = T_in;
    p.T_out = T_out;
    p.out_div = 1.f;
    p.out_mul = 1.f;
    p.y_bstride_rows = T_out;
    p.split = INT_MAX;
    p.seg[0].y = y;
    p.seg[0].ld = ldy;
    return p;
}
void set_res(ConvParams& p, int s, const float* res, int ld) {
    p.seg[s].res = res;
    p.seg[s].ld_res = ld;
}

} // namespace dtts
