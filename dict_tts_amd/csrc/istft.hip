// Spectral-subtraction denoising on the device, and its two halves alone: the reference's denoise(wav, v) (vocoders/vocoder_utils.py:7-15:
// librosa.stft -> max(|S| - v, 0), phase kept -> librosa.istft; center=True, pad_mode='constant'), _stft and _istft (utils/audio.py:35-42).
//
// FORWARD + EDIT (spectral_fwd_kernel) is the shared contraction of stft_core.h, staged with zeros outside
// [0, len), which IS the constant padding.  re and im stay in the accumulators, the edit S' = S max(|S| - v, 0) / |S| happens there (v = 0:
// nothing, no division), and S' leaves as interleaved (re, im) pairs [B][spec_cap][n_fft / 2 + 1][2], torch.view_as_real's layout.
//
// INVERSE (section 3.8), two launches:
//   * istft_frames_kernel: D[sample 32][frame 32] += Wi[sample][q 2] * S'[q 2][frame], one wave per 32 frames, over the n_fft REAL spectral
//     values of a frame in their memory order, q = 2 k -> re[k], q = 2 k + 1 -> im[k], with re[n_fft / 2] taking the place of im[0] (the
//     imaginary parts of bins 0 and n_fft / 2 are never read, as in every c2r transform).  Wi is the inverse basis with the synthesis
//     window, 1 / n_fft and the factor 2 folded in (fp64 at finalisation, rounded once, fragment order, streamed from L2); the B operand
//     comes straight from the spectrum: lane half h holds 16 consecutive values of a super-group, read as eight 8-byte loads.  Two sample
//     blocks share one B value, as re / im do in the forward kernel; same short chains, same fp64 join.  The windowed frames go to a
//     workspace fr[b][t][n].
//   * istft_gather_kernel: one thread per output sample sums the covering frames in ASCENDING frame order in fp64, divides by the window
//     envelope of exactly those frames (fp64, so the first and last n_fft / hop frames get their own) and rounds once.
// No atomics, no LDS in the inverse, one summation order: a frame's samples do not depend on the tile it falls into, so an utterance is
// bit-identical alone, in any batch, at either tile size of the forward kernel (the inverse has one).
#include "ctx.h"
#include "istft.h"

namespace dtts {

template <int WT>
__global__ __launch_bounds__(64 * WT) void spectral_fwd_kernel(const SpecFwdParams p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fi = lane & 31, hf = lane >> 5;
    const int cg = blockIdx.x % p.csplit, bt = blockIdx.x / p.csplit, b = bt / p.g.ntile, tile = bt % p.g.ntile;
    const int len = stft_len(p.lens, b, p.wav_ld);
    const int T = 1 + len / p.g.hop;
    if (tile == 0 && cg == 0 && tid == 0) p.frames[b] = T;
    const int f0 = tile * p.g.tt;
    if (f0 >= T) return;
    const int nf = T - f0 < p.g.tt ? T - f0 : p.g.tt;   // frames of this tile
    const float* const sig[1] = {p.wav + (size_t)b * p.wav_ld};
    stft_stage<64 * WT>(slab, 0, sig, len, f0, nf, p.g, tid, [](int g) { return g; });
    __syncthreads();
    if (wv * 32 >= nf) return;   // (no barrier below)
    const int f = wv * 32 + fi;
    const bool live = f < nf;
    const int abase = (live ? f : wv * 32) * p.g.hop + hf;   // a dead lane recomputes the wave's first frame and stores nothing
    const int N = p.g.n_fft, c_lo = cg * (N / 64 / p.csplit), c_hi = c_lo + N / 64 / p.csplit;   // this workgroup's bin blocks
    float* row = p.spec + ((size_t)b * p.spec_cap + f0 + (live ? f : wv * 32)) * (size_t)(N + 2);
    const float v = p.floor;

    stft_contract(p.g.basis, N / 32, p.g.sg_lo, p.g.sg_hi, c_lo, c_hi, slab, abase, p.g.ps, lane, [&](int c, stft_f32x16 re, stft_f32x16 im) {
        // ---- bin 0 is real and its im slot carried re[n_fft / 2], a (real) bin of its own
        const bool edge = c == 0 && hf == 0;
        float nyq = 0.f;
        if (edge) {
            nyq = im[0];
            im[0] = 0.f;
        }
        // ---- the edit, in place: m > v scales by (m - v) / m, anything else (m = 0 included) becomes zero; v = 0 leaves S as it is
        if (v > 0.f) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float m = __builtin_sqrtf(__builtin_fmaf(re[r], re[r], __fmul_rn(im[r], im[r])));
                const float s = m > v ? (m - v) / m : 0.f;
                re[r] = __fmul_rn(re[r], s);
                im[r] = __fmul_rn(im[r], s);
            }
            const float m = __builtin_fabsf(nyq);
            nyq = m > v ? __fmul_rn(nyq, (m - v) / m) : 0.f;
        }
        if (live) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                float2* d = (float2*)(row + 2 * (32 * c + 8 * rq + 4 * hf));
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = make_float2(re[4 * rq + e], im[4 * rq + e]);
            }
            if (edge) *(float2*)(row + N) = make_float2(nyq, 0.f);
        }
    });
}

// NOT stft_contract, though the pipeline has the same shape: the B operand is no slab read but registers fetched alongside the basis (xa / xb
// travel with fa / fb), and every chain ends at a sched_barrier of its own.  A shared loop would have to branch on its caller.
__global__ __launch_bounds__(64) void istft_frames_kernel(const SpecInvParams p) {
    const int lane = threadIdx.x, fi = lane & 31, hf = lane >> 5;
    const int cg = blockIdx.x % p.csplit, bt = blockIdx.x / p.csplit, b = bt / p.ntile, tile = bt % p.ntile;
    int T = p.frames[b];
    T = T < 0 ? 0 : (T > p.tcap ? p.tcap : T);
    const int f0 = tile * ISTFT_TILE;
    if (f0 >= T) return;
    const bool live = f0 + fi < T;
    const int f = f0 + (live ? fi : 0);   // a dead lane recomputes the tile's first frame and stores nothing
    const int N = p.n_fft, SG = N / 32, c_lo = cg * (N / 64 / p.csplit), c_hi = c_lo + N / 64 / p.csplit;   // this workgroup's pairs of sample blocks
    const float* row = p.spec + ((size_t)b * p.spec_cap + f) * (size_t)(N + 2);
    const float nyq = row[N];
    const float2* xr = (const float2*)(row + 16 * hf);

    // one super-group = 16 MFMA steps = 32 spectral values: eight 16-byte fragments of Wi per lane (sample block 2 c, then 2 c + 1) and this
    // lane half's 16 values of its frame.  Two register buffers take turns, as in the forward kernel.
    auto fetch = [&](float4 (&d)[8], float2 (&x)[8], int c, int sg) {
        const float4* s = p.wi + ((size_t)(c * SG + sg) * 8) * 64 + lane;
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = s[q * 64];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = xr[16 * sg + q];
        if (sg == 0 && hf == 0) x[0].y = nyq;   // q = 1: re[n_fft / 2] in the place of im[0]
        __builtin_amdgcn_sched_barrier(0);
    };
    float4 fa[8], fb[8];
    float2 xa[8], xb[8];
    fetch(fa, xa, c_lo, 0);
#pragma unroll 1
    for (int c = c_lo; c < c_hi; ++c) {
        double d0[16], d1[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) d0[r] = d1[r] = 0.0;
        auto contract = [&](const float4 (&w)[8], const float2 (&x)[8]) {
#pragma unroll
            for (int ch = 0; ch < 16 / MELSPEC_CHUNK; ++ch) {
                stft_f32x16 y0, y1;
#pragma unroll
                for (int r = 0; r < 16; ++r) y0[r] = y1[r] = 0.f;
#pragma unroll
                for (int jj = 0; jj < MELSPEC_CHUNK; ++jj) {
                    const int j = ch * MELSPEC_CHUNK + jj;
                    const float s = (j & 1) ? x[j >> 1].y : x[j >> 1].x;
                    y0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j >> 2][j & 3], s, y0, 0, 0, 0);
                    y1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w[4 + (j >> 2)][j & 3], s, y1, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    d0[r] += (double)y0[r];
                    d1[r] += (double)y1[r];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
#pragma unroll 1
        for (int sg = 0; sg < SG; sg += 4) {
            fetch(fb, xb, c, sg + 1);
            contract(fa, xa);
            fetch(fa, xa, c, sg + 2);
            contract(fb, xb);
            fetch(fb, xb, c, sg + 3);
            contract(fa, xa);
            const bool wrap = sg + 4 == SG;
            fetch(fa, xa, wrap ? (c + 1 < c_hi ? c + 1 : c) : c, wrap ? 0 : sg + 4);
            contract(fb, xb);
        }
        if (live) {
            float* o = p.fr + ((size_t)b * p.spec_cap + f) * (size_t)N + 64 * c + 4 * hf;
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                *(float4*)(o + 8 * rq) = make_float4((float)d0[4 * rq], (float)d0[4 * rq + 1], (float)d0[4 * rq + 2], (float)d0[4 * rq + 3]);
                *(float4*)(o + 32 + 8 * rq) = make_float4((float)d1[4 * rq], (float)d1[4 * rq + 1], (float)d1[4 * rq + 2], (float)d1[4 * rq + 3]);
            }
        }
    }
}

__global__ __launch_bounds__(ISTFT_GATHER) void istft_gather_kernel(const SpecGatherParams p) {
    const int b = blockIdx.x / p.nchunk, chunk = blockIdx.x % p.nchunk;
    int T = p.frames[b];
    T = T < 0 ? 0 : (T > p.tcap ? p.tcap : T);
    const int out_len = T > 0 ? p.hop * (T - 1) : 0;   // <= wav_ld: tcap <= 1 + wav_ld / hop
    if (chunk == 0 && threadIdx.x == 0 && p.out_lens) p.out_lens[b] = out_len;
    const int s = chunk * ISTFT_GATHER + threadIdx.x;
    if (s >= out_len) return;
    const int N = p.n_fft, q = s + N / 2;          // position in the padded signal; frame t covers [t hop, t hop + N)
    const int t_lo = q >= N ? (q - N) / p.hop + 1 : 0;
    const int t_hi = q / p.hop < T - 1 ? q / p.hop : T - 1;
    const float* fr = p.fr + (size_t)b * p.spec_cap * (size_t)N;
    double acc = 0.0, env = 0.0;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int n = q - t * p.hop;
        acc += (double)fr[(size_t)t * N + n];
        env += p.w2[n];
    }
    p.out[(size_t)b * p.wav_ld + s] = (float)(acc / env);
}

std::vector<float> istft_pack_inverse(int n_fft, const std::vector<float>& window) {
    const int N = n_fft, NB = N / 64, SG = N / 32;
    std::vector<double> cs(N), sn(N);
    for (int j = 0; j < N; ++j) {
        cs[j] = cos(2.0 * M_PI * j / N);
        sn[j] = sin(2.0 * M_PI * j / N);
    }
    std::vector<float> out((size_t)NB * SG * 8 * 64 * 4);
    for (int c = 0; c < NB; ++c)
        for (int sg = 0; sg < SG; ++sg)
            for (int part = 0; part < 8; ++part)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int j = 4 * (part & 3) + e, q = 32 * sg + 16 * (lane >> 5) + j, n = 32 * (2 * c + (part >> 2)) + (lane & 31);
                        const int k = q >> 1, ang = (int)(((long long)k * n) % N);
                        const double w = (double)window[n] / N;
                        double v;
                        if (q == 0) v = w;
                        else if (q == 1) v = (n & 1) ? -w : w;   // re[n_fft / 2] in the im slot of bin 0
                        else if (q & 1) v = -2.0 * w * sn[ang];
                        else v = 2.0 * w * cs[ang];
                        out[((((size_t)(c * SG + sg) * 8 + part) * 64) + lane) * 4 + e] = (float)v;
                    }
    return out;
}

double istft_envelope_min(const std::vector<float>& window, int hop) {
    const int N = (int)window.size();
    double worst = INFINITY;
    for (int q = N / 2; q < N / 2 + hop; ++q) {
        double e = 0.0;
        if (q < N) e += (double)window[q] * (double)window[q];
        if (q >= hop) e += (double)window[q - hop] * (double)window[q - hop];
        worst = std::min(worst, e);
    }
    return worst;
}

// The blocks of a frame's output (bin blocks forward, pairs of sample blocks inverse) are independent of each other, so a launch that would
// leave the device short of workgroups hands them out over `split` workgroups per tile: the smallest power of two that reaches `want`
// workgroups, at most `blocks` (itself a power of two).  Every output is still one chain in one order: the split changes no bit.
int istft_split(long long tiles, int blocks, long long want) {
    int split = 1;
    while (split < blocks && tiles * split < want) split *= 2;
    return split;
}

hipError_t spectral_forward_launch(SpecFwdParams p, int n_cu, hipStream_t stream) {
    return spectral_forward_pick<spectral_fwd_kernel<2>, spectral_fwd_kernel<4>>(p, n_cu, stream);
}

hipError_t istft_frames_launch(SpecInvParams p, int n_cu, hipStream_t stream) {
    if (!melspec_supported(p.n_fft, p.n_fft, p.n_fft, 1)) return hipErrorInvalidValue;
    if (p.B < 1 || p.tcap < 1 || p.tcap > p.spec_cap || !p.spec || !p.frames || !p.fr || ((uintptr_t)p.spec & 7) || ((uintptr_t)p.fr & 15)) return hipErrorInvalidValue;
    p.csplit = istft_split((long long)p.ntile * p.B, p.n_fft / 64, 16LL * n_cu);   // one-wave workgroups, four to a CU
    if (p.ntile != (p.tcap + ISTFT_TILE - 1) / ISTFT_TILE || (long long)p.ntile * p.B * p.csplit > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(istft_frames_kernel, dim3((unsigned)(p.ntile * p.B * p.csplit)), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t istft_gather_launch(const SpecGatherParams& p, hipStream_t stream) {
    if (p.B < 1 || p.hop < 1 || p.hop > p.n_fft || p.tcap < 1 || p.tcap > p.spec_cap || p.tcap > 1 + p.wav_ld / p.hop || !p.fr || !p.frames || !p.w2) return hipErrorInvalidValue;
    if ((!p.out && p.wav_ld > 0) || p.nchunk != std::max(1, (p.wav_ld + ISTFT_GATHER - 1) / ISTFT_GATHER) || (long long)p.nchunk * p.B > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(istft_gather_kernel, dim3((unsigned)(p.nchunk * p.B)), dim3(ISTFT_GATHER), 0, stream, p);
    return hipGetLastError();
}

// ---- dtts_finalize_weights(DTTS_PART_ISTFT): "istft.window" [n_fft], zero padded and centred to n_fft as torch.stft applies it -> the plan
// (forward basis, inverse basis, the window's squares).  Finalising again replaces the plan; the packs of the old one stay allocated until
// dtts_destroy (a launch in flight may still read them).
int build_istft(dtts_ctx* h) {
    const char* me = "dtts_finalize_weights(DTTS_PART_ISTFT)";
    Need need{h};
    const HostTensor* wn = need.get("istft.window");
    if (!wn) return fail(h, DTTS_E_NOENT, "%s: missing weight %s", me, need.missing.c_str());
    if (wn->shape.size() != 1) return fail(h, DTTS_E_INVAL, "%s: istft.window must be [n_fft] (got %d dimensions)", me, (int)wn->shape.size());
    const int n_fft = (int)std::min<int64_t>(wn->shape[0], INT_MAX);
    std::string why;
    if (!melspec_supported(n_fft, n_fft, n_fft, 1, &why)) return fail(h, DTTS_E_INVAL, "%s: istft.window: unsupported %s", me, why.c_str());
    for (int k = 0; k < n_fft; ++k)
        if (!std::isfinite(wn->f[k])) return fail(h, DTTS_E_INVAL, "%s: istft.window[%d] is not finite", me, k);
    const SgRange sup = window_support(wn->f);
    if (!sup.hi) return fail(h, DTTS_E_INVAL, "%s: istft.window is all zero", me);
    std::vector<double> w2(n_fft);
    for (int k = 0; k < n_fft; ++k) w2[k] = (double)wn->f[k] * (double)wn->f[k];
    // optional: "istft.inv_mel_basis" [n_fft / 2 + 1][n_mels], the pseudo-inverse of the mel filterbank that Griffin-Lim's mel input goes
    // through (griffinlim.hip), stored transposed, [n_mels][n_fft / 2 + 1], so that neighbouring bins are neighbouring loads
    float* pinv = nullptr;
    int pinv_mels = 0;
    const auto pit = h->w.find("istft.inv_mel_basis");
    if (pit != h->w.end()) {
        const HostTensor& pt = pit->second;
        const int bins = n_fft / 2 + 1;
        if (pt.shape.size() != 2 || pt.shape[0] != bins || pt.shape[1] < 1 || pt.shape[1] > 128)
            return fail(h, DTTS_E_INVAL, "%s: istft.inv_mel_basis must be [n_fft / 2 + 1 = %d][n_mels in 1 .. 128] (got %d dimensions, %lld x %lld)", me, bins,
                        (int)pt.shape.size(), (long long)(pt.shape.size() > 0 ? pt.shape[0] : 0), (long long)(pt.shape.size() > 1 ? pt.shape[1] : 0));
        pinv_mels = (int)pt.shape[1];
        std::vector<float> tr((size_t)pinv_mels * bins);
        for (int k = 0; k < bins; ++k)
            for (int j = 0; j < pinv_mels; ++j) {
                const float v = pt.f[(size_t)k * pinv_mels + j];
                if (!std::isfinite(v)) return fail(h, DTTS_E_INVAL, "%s: istft.inv_mel_basis[%d][%d] is not finite", me, k, j);
                tr[(size_t)j * bins + k] = v;
            }
        if (!(pinv = upload(h, tr))) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
    }
    float* basis = upload(h, melspec_pack_basis(n_fft, wn->f));
    float* wi = upload(h, istft_pack_inverse(n_fft, wn->f));
    double* w2d = upload(h, w2);
    if (!basis || !wi || !w2d) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
    h->is_pinv = pinv;
    h->is_pinv_mels = pinv_mels;
    h->is = StftBasisPlan{basis, n_fft, sup.lo, sup.hi};
    h->is_wi = wi;
    h->is_w2 = w2d;
    h->is_window = wn->f;
    h->is_env.clear();
    h->is_skew_hop = 0;
    h->istft_ready = true;
    return DTTS_OK;
}

// the envelope criterion per (window, hop), fp64 on the host, remembered (0 = met)
int check_envelope(dtts_ctx* h, const char* me, int hop) {
    auto it = h->is_env.find(hop);
    if (it == h->is_env.end()) it = h->is_env.emplace(hop, istft_envelope_min(h->is_window, hop)).first;
    if (!(it->second > ISTFT_ENV_MIN))
        return fail(h, DTTS_E_INVAL, "%s: hop = %d: the window's envelope sum_t w^2[n - t hop] falls to %g at a kept sample (must stay above %g)", me, hop,
                    it->second, ISTFT_ENV_MIN);
    return DTTS_OK;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_SPECTRAL): one launch (FORWARD), two (INVERSE) or three on the caller's stream; no host synchronisation
// unless the workspace grows
int spectral_forward(dtts_ctx* h, const dtts_spectral_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_SPECTRAL)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (int rc = blk.finalized(DTTS_PART_ISTFT)) return rc;
    const int N = h->is.n_fft;
    if (a->mode < 1 || a->mode > 3) return fail(h, DTTS_E_INVAL, "%s: mode = %d (DTTS_SPECTRAL_FORWARD = 1, DTTS_SPECTRAL_INVERSE = 2, or both = 3)", me, a->mode);
    const bool fwd = (a->mode & DTTS_SPECTRAL_FORWARD) != 0, inv = (a->mode & DTTS_SPECTRAL_INVERSE) != 0;
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (a->hop < 1 || a->hop > N) return fail(h, DTTS_E_INVAL, "%s: hop = %d (supported: 1 .. n_fft = %d)", me, a->hop, N);
    if (int e = check_wav_ld(h, me, a->wav_ld, N)) return e;
    const int t_need = 1 + a->wav_ld / a->hop;
    if (a->spec_cap < t_need)
        return fail(h, DTTS_E_INVAL, "%s: spec_cap = %d rows, wav_ld = %d samples at hop %d give %d", me, a->spec_cap, a->wav_ld, a->hop, t_need);
    if (!(a->floor >= 0.f) || !(a->floor < 3.0e38f)) return fail(h, DTTS_E_INVAL, "%s: floor = %g (must be finite and not negative)", me, (double)a->floor);
    if (fwd && !a->wav_dev && a->wav_ld > 0) return fail(h, DTTS_E_INVAL, "%s: null wav_dev (DTTS_SPECTRAL_FORWARD reads it)", me);
    if (inv && !a->out_dev && a->wav_ld > 0) return fail(h, DTTS_E_INVAL, "%s: null out_dev (DTTS_SPECTRAL_INVERSE writes it)", me);
    if (!(fwd && inv) && !a->spec_dev) return fail(h, DTTS_E_INVAL, "%s: null spec_dev (optional only with both mode bits)", me);
    if (!(fwd && inv) && !a->frames_dev) return fail(h, DTTS_E_INVAL, "%s: null frames_dev (optional only with both mode bits)", me);
    if (int rc = blk.aligned(8, {{"spec_dev", a->spec_dev}})) return rc;
    if (inv && a->out_dev && a->wav_dev) {   // the forward loads of one utterance would race with the gather stores of another
        const size_t n = (size_t)a->B * (size_t)a->wav_ld;
        if (a->out_dev < a->wav_dev + n && a->wav_dev < a->out_dev + n)
            return fail(h, DTTS_E_INVAL, "%s: out_dev overlaps wav_dev (out_dev == wav_dev %+lld samples, B wav_ld = %lld: the filter does not run in place)", me,
                        (long long)(a->out_dev - a->wav_dev), (long long)n);
    }
    if (inv)
        if (int e = check_envelope(h, me, a->hop)) return e;
    const long long n_tiles_inv = (long long)a->B * ((t_need + ISTFT_TILE - 1) / ISTFT_TILE);
    const long long n_chunks = (long long)a->B * std::max(1, (a->wav_ld + ISTFT_GATHER - 1) / ISTFT_GATHER);
    if (n_tiles_inv * (N / 64) > INT_MAX || n_chunks > INT_MAX) return fail(h, DTTS_E_INVAL, "%s: B = %d utterances of wav_ld = %d samples", me, a->B, a->wav_ld);

    // ---- the workspace: the spectrum between the stages (unless the caller holds it), the frame counts, the windowed frames
    const size_t rows = (size_t)a->B * (size_t)a->spec_cap;
    const size_t n_spec = a->spec_dev ? 0 : rows * (size_t)(N + 2), n_fr = inv ? rows * (size_t)N : 0, n_frames = a->frames_dev ? 0 : (size_t)a->B;
    HIPCHK(h->a_spec.reserve((n_spec + n_fr + n_frames) * sizeof(float) + 3 * 256, stream));
    float* spec = a->spec_dev;
    int* frames = a->frames_dev;
    float* fr = nullptr;
    if (n_spec && !(spec = h->a_spec.alloc<float>(n_spec))) return blk.workspace();
    if (n_fr && !(fr = h->a_spec.alloc<float>(n_fr))) return blk.workspace();
    if (n_frames && !(frames = h->a_spec.alloc<int>(n_frames))) return blk.workspace();

    if (fwd) {
        if (h->is_skew_hop != a->hop) {
            h->is_skew = melspec_skew_shift(a->hop);
            h->is_skew_hop = a->hop;
        }
        SpecFwdParams p{};
        p.wav = a->wav_dev;
        p.lens = a->lens_dev;
        p.frames = frames;
        p.spec = spec;
        p.g = stft_geom(h->is, a->hop, h->is_skew);
        p.B = a->B;
        p.wav_ld = a->wav_ld;
        p.spec_cap = a->spec_cap;
        p.floor = a->floor;
        LAUNCH(spectral_forward_launch(p, h->n_cu, stream));
    }
    if (inv) {
        SpecInvParams p{};
        p.spec = spec;
        p.frames = frames;
        p.fr = fr;
        p.wi = (const float4*)h->is_wi;
        p.B = a->B;
        p.spec_cap = a->spec_cap;
        p.tcap = t_need;
        p.n_fft = N;
        p.ntile = (t_need + ISTFT_TILE - 1) / ISTFT_TILE;
        LAUNCH(istft_frames_launch(p, h->n_cu, stream));
        SpecGatherParams g{};
        g.fr = fr;
        g.frames = frames;
        g.w2 = h->is_w2;
        g.out = a->out_dev;
        g.out_lens = a->out_lens_dev;
        g.B = a->B;
        g.spec_cap = a->spec_cap;
        g.tcap = t_need;
        g.wav_ld = a->wav_ld;
        g.hop = a->hop;
        g.n_fft = N;
        g.nchunk = std::max(1, (a->wav_ld + ISTFT_GATHER - 1) / ISTFT_GATHER);
        LAUNCH(istft_gather_launch(g, stream));
    }
    return DTTS_OK;
}

} // namespace dtts
