// libdicttts_hip.so — the multi-window mel discriminator on clips of n_sig mels (meldisc.h; dtts_text2mel_fetch(DTTS_OUT_MELDISC)).  One launch
// forms the clip table of every window; then per chunk of signals and per window: block 1 (C_in = 1: VALU, reading the mel at start + t),
// blocks 2 and 3 on the implicit-GEMM kernel, the instance statistics of their maps (fp64, two passes, a launch of their own), the head, and
// the fp64 sums per (signal, window).  A workgroup never waits on another and nothing is accumulated with atomics.
#include "ctx.h"

namespace dtts {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float mlrelu(float v) { return v > 0.f ? v : v * MELDISC_SLOPE; }

struct MelHops {
    int hop[DTTS_MELDISC_MAX_WIN];
};

// ---- the clip table: vlen[s] (0 for a refused length), status[s], cst[w][s * clips_ld + j] = start of slot j or -1
__global__ void meldisc_clips_kernel(const int* lens, const int* starts, int n_sig, int T_ld, int clips_ld, int n_win, MelHops hops, int within,
                                     int* vlen, int* cst, int* status) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n_sig * clips_ld) return;
    const int s = (int)(idx / clips_ld), j = (int)(idx - (long long)s * clips_ld);
    int L = lens ? lens[s] : T_ld;
    const bool bad = L < 0 || L > T_ld;
    if (bad) L = 0;
    if (j == 0) {
        vlen[s] = L;
        status[s] = bad ? DTTS_MELDISC_BAD_LEN : 0;
    }
    for (int w = 0; w < n_win; ++w) {
        const long long st = starts ? (long long)starts[((size_t)w * n_sig + s) * clips_ld + j] : (long long)j * hops.hop[w];
        const bool ok = st >= 0 && st + (32 << w) <= (within ? L : T_ld);
        cst[(size_t)w * n_sig * clips_ld + idx] = ok ? (int)st : -1;
    }
}

// ---- block 1: Conv2d(1 -> H, 3 x 3, stride 2, pad 1) + LeakyReLU on the clip's rows start .. start + win - 1 of its signal's mel; rows at
// or behind the signal's length are zeros.  One thread per output element, nine taps in a fixed order
struct MelEntryParams {
    const float* mel;        // [nsig][T_ld][80]
    const int* vlen;         // [nsig]
    const int* cst;          // [nsig * clips_ld]
    const float *w, *bias;   // [9][H], [H]
    float* y;                // [nclip][win / 2][40][H]
    int clips_ld, T_ld, win, H;
};
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_entry_kernel(const MelEntryParams p) {
    const int clip = blockIdx.x, st = p.cst[clip];
    if (st < 0) return;
    const int e = blockIdx.y * MELDISC_THREADS + threadIdx.x;
    const int F1 = MELDISC_F / 2;
    if (e >= (p.win / 2) * F1 * p.H) return;
    const int c = e % p.H, pos = e / p.H, f1 = pos % F1, t1 = pos / F1;
    const int s = clip / p.clips_ld;
    const int L = min(p.vlen[s], p.T_ld);
    const float* xb = p.mel + (size_t)s * p.T_ld * MELDISC_F;
    float acc = 0.f;
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
        const int tc = 2 * t1 + dt - 1;
        if (tc < 0 || tc >= p.win || st + tc >= L) continue;
#pragma unroll
        for (int df = 0; df < 3; ++df) {
            const int fi = 2 * f1 + df - 1;
            if (fi < 0 || fi >= MELDISC_F) continue;
            acc = fmaf(p.w[(dt * 3 + df) * p.H + c], xb[(size_t)(st + tc) * MELDISC_F + fi], acc);
        }
    }
    p.y[(size_t)clip * (p.win / 2) * F1 * p.H + e] = mlrelu(acc + p.bias[c]);
}

// ---- blocks 2 and 3: Conv2d(H -> H, 3 x 3, stride 2, pad 1) + LeakyReLU as an implicit GEMM on the fp32 matrix cores.  One workgroup = a
// tile of TR x FC = 32 output positions of ONE clip x up to 128 output channels (a wave per co-tile of 32).  Per chunk of 32 input channels
// the (2 TR + 1) x (2 FC + 1) input patch is staged in LDS, normalised on the way in, zero outside the map at all four borders; output
// position (tr, fc), tap (dt, df) reads cell (2 tr + dt, 2 fc + df): one ds_read_b128 gives a lane the four consecutive channels of its
// k-half, spent on four v_mfma_f32_32x32x2_f32 (A[i = l & 31][k = l >> 5]; the weights carry the same permutation: meldisc.h).  One fp32
// accumulation chain per output in (chunk, tap, channel) order.
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_conv_kernel(const MelConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float mlds[];
    const int clip = blockIdx.x;
    if (p.cst[clip] < 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tt = blockIdx.y / p.ntf, tf = blockIdx.y - tt * p.ntf;
    const int t0 = tt * p.TR, f0 = tf * p.FC;
    const int PR = 2 * p.TR + 1, PC = 2 * p.FC + 1;
    const int nt = blockIdx.z * 4 + wave;
    const bool live = nt * 32 < p.H;
    const int m = lane & 31, hh = lane >> 5;
    const int cellbase = (2 * (m >> p.fc_shift)) * PC + 2 * (m & (p.FC - 1));
    const float* xb = p.x + (size_t)clip * p.Tin * p.Fin * p.H;
    const float2* nr = p.nrm + (size_t)clip * p.nrm_ld;
    const f32x4* wv = (const f32x4*)p.w + (size_t)(live ? nt : 0) * p.nch * (9 * 4 * 64) + lane;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ch = 0; ch < p.nch; ++ch) {
        if (ch) __syncthreads();   // the previous chunk's reads are done
        for (int idx = tid; idx < PR * PC * (MELDISC_KC / 4); idx += MELDISC_THREADS) {
            const int cell = idx >> 3, c4 = (idx & 7) * 4;
            const int pr = cell / PC, pc = cell - pr * PC;
            const int ti = 2 * t0 - 1 + pr, fi = 2 * f0 - 1 + pc;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ti >= 0 && ti < p.Tin && fi >= 0 && fi < p.Fin) {
                const int c = ch * MELDISC_KC + c4;
                v = *(const f32x4*)(xb + ((size_t)ti * p.Fin + fi) * p.H + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 ms = nr[c + e];
                    v[e] = fmaf(v[e] - ms.x, ms.y, p.shift[c + e]);
                }
            }
            *(f32x4*)(mlds + cell * MELDISC_PITCH + c4) = v;
        }
        __syncthreads();
        if (live) {
            const f32x4* wc = wv + (size_t)ch * (9 * 4 * 64);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float* a0 = mlds + (cellbase + (tap / 3) * PC + (tap % 3)) * MELDISC_PITCH + 4 * hh;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 a = *(const f32x4*)(a0 + 8 * q);
                    const f32x4 b = wc[(tap * 4 + q) * 64];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
                }
            }
        }
    }
    if (!live) return;
    const int co = nt * 32 + m;
    const float bias = p.bias[co];
    float* yb = p.y + (size_t)clip * p.Tout * p.Fout * p.H + co;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hh;
        const int t = t0 + (i >> p.fc_shift), f = f0 + (i & (p.FC - 1));
        if (t < p.Tout && f < p.Fout) yb[((size_t)t * p.Fout + f) * p.H] = mlrelu(acc[r] + bias);
    }
}

// ---- instance statistics of a map [P positions][H]: per (clip, channel) the mean and the biased variance in fp64 by two passes.  G = 256 / H
// thread groups share a channel's positions (p = g, g + G, ...) and are joined in group order; every thread of a channel forms the same mean
struct MelStatParams {
    const float* x;          // [nclip][P][H]
    const int* cst;
    const float* gamma;      // [H]
    float2* nrm;             // [nclip][H]: (mean, gamma / sqrt(var + eps))
    int P, H, G;
};
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_stats_kernel(const MelStatParams p) {
    __shared__ double red[MELDISC_THREADS];
    const int clip = blockIdx.x;
    if (p.cst[clip] < 0) return;
    const int tid = threadIdx.x, c = tid % p.H, g = tid / p.H;
    const float* xb = p.x + (size_t)clip * p.P * p.H + c;
    double s = 0.0;
    for (int q = g; q < p.P; q += p.G) s += (double)xb[(size_t)q * p.H];
    red[g * p.H + c] = s;
    __syncthreads();
    double mean = 0.0;
    for (int k = 0; k < p.G; ++k) mean += red[k * p.H + c];
    mean /= (double)p.P;
    __syncthreads();
    double v = 0.0;
    for (int q = g; q < p.P; q += p.G) {
        const double d = (double)xb[(size_t)q * p.H] - mean;
        v += d * d;
    }
    red[g * p.H + c] = v;
    __syncthreads();
    if (g) return;
    double var = 0.0;
    for (int k = 0; k < p.G; ++k) var += red[k * p.H + c];
    var /= (double)p.P;
    p.nrm[(size_t)clip * p.H + c] = make_float2((float)mean, (float)((double)p.gamma[c] / sqrt(var + MELDISC_IN_EPS)));
}

// fixed tree over the workgroup's 256 fp64 values per slot
template <int NS>
__device__ __forceinline__ void mel_tree(double (&v)[NS], double* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NS; ++q) red[q * MELDISC_THREADS + tid] = v[q];
    __syncthreads();
    for (int w = MELDISC_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < NS; ++q) red[q * MELDISC_THREADS + tid] += red[q * MELDISC_THREADS + tid + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) v[q] = red[q * MELDISC_THREADS];
}

// ---- the head: D = adv . norm(map) + bias over n elements (the whole map, or one time row under `none`); exact products, fp64 sums, a
// fixed order within the thread and a fixed tree across the workgroup
struct MelHeadParams {
    const float* x;          // [nclip][n_out * n]
    const int* cst;
    const float2* nrm;
    const float* shift;
    const float* w;          // [n] channels-last
    float* dws;              // [nclip][DTTS_MELDISC_D_LD]
    float bias;
    int nrm_ld, H, n, n_out;
};
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_head_kernel(const MelHeadParams p) {
    __shared__ double red[MELDISC_THREADS];
    const int clip = blockIdx.x, o = blockIdx.y;
    if (p.cst[clip] < 0) return;
    const float* xb = p.x + ((size_t)clip * p.n_out + o) * p.n;
    const float2* nr = p.nrm + (size_t)clip * p.nrm_ld;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < p.n; i += MELDISC_THREADS) {
        const int c = i % p.H;
        const float2 ms = nr[c];
        v[0] += (double)fmaf(xb[i] - ms.x, ms.y, p.shift[c]) * (double)p.w[i];
    }
    mel_tree<1>(v, red);
    if (threadIdx.x == 0) p.dws[(size_t)clip * DTTS_MELDISC_D_LD + o] = (float)(v[0] + (double)p.bias);
}

// ---- the sums of one window, a workgroup per signal: its clip slots in order
struct MelScoreParams {
    const float* dws;        // [nsig * clips_ld][DTTS_MELDISC_D_LD]
    const int* cst;
    double* sums;            // + s * 6: this window's two sums
    long long* counts;       // + s * 3
    float* d;                // + s * clips_ld * DTTS_MELDISC_D_LD, or null
    int clips_ld, n_out;
};
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_score_kernel(const MelScoreParams p) {
    __shared__ double red[3 * MELDISC_THREADS];
    const int s = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < p.clips_ld * p.n_out; i += MELDISC_THREADS) {
        const int j = i / p.n_out, o = i - j * p.n_out;
        const size_t clip = (size_t)s * p.clips_ld + j;
        if (p.cst[clip] < 0) continue;
        const float df = p.dws[clip * DTTS_MELDISC_D_LD + o];
        const double D = (double)df;
        v[0] += (1.0 - D) * (1.0 - D);
        v[1] += D * D;
        v[2] += 1.0;
        if (p.d) p.d[clip * DTTS_MELDISC_D_LD + o] = df;
    }
    mel_tree<3>(v, red);
    if (threadIdx.x == 0) {
        p.sums[(size_t)s * 6] = v[0];
        p.sums[(size_t)s * 6 + 1] = v[1];
        p.counts[(size_t)s * 3] = (long long)v[2];
    }
}

// ---- a block's output as the reference's `h` holds it: the norm applied, channels-last
__global__ __launch_bounds__(MELDISC_THREADS) void meldisc_export_kernel(const float* x, const int* cst, const float2* nrm, int nrm_ld, const float* shift,
                                                                         float* out, int n, int H) {
    const int clip = blockIdx.x;
    if (cst[clip] < 0) return;
    const int i = blockIdx.y * MELDISC_THREADS + threadIdx.x;
    if (i >= n) return;
    float v = x[(size_t)clip * n + i];
    if (nrm) {
        const int c = i % H;
        const float2 ms = nrm[(size_t)clip * nrm_ld + c];
        v = fmaf(v - ms.x, ms.y, shift[c]);
    }
    out[(size_t)clip * n + i] = v;
}

// =====================================================================================================================================
// weights
namespace {

std::string mshape(const HostTensor* t) {
    std::string s = "[";
    for (size_t i = 0; i < t->shape.size(); ++i) s += (i ? ", " : "") + std::to_string((long long)t->shape[i]);
    return s + "]";
}

const char* PART = "dtts_finalize_weights(DTTS_PART_MELDISC)";

} // namespace

int build_meldisc(dtts_ctx* h) {
    Need need{h};
    auto missing = [&]() { return fail(h, DTTS_E_NOENT, "%s: missing tensor %s", PART, need.missing.c_str()); };
    const HostTensor* first = need.get("meldisc.0.conv.0.weight");
    if (!first) return missing();
    const int H = first->shape.empty() ? 0 : (int)first->shape[0];
    if (first->shape.size() != 4 || first->numel() != (int64_t)H * 9)
        return fail(h, DTTS_E_INVAL, "%s: meldisc.0.conv.0.weight is %s; the reference's first block is [H, 1, 3, 3]", PART, mshape(first).c_str());
    if (H < 32 || H > DTTS_MELDISC_MAX_HIDDEN || H % 32)
        return fail(h, DTTS_E_INVAL, "%s: mel_disc_hidden_size = %d (supported: the multiples of 32 up to %d)", PART, H, DTTS_MELDISC_MAX_HIDDEN);
    int n_win = 0;
    while (h->w.count("meldisc." + std::to_string(n_win) + ".conv.0.weight")) ++n_win;
    if (n_win > DTTS_MELDISC_MAX_WIN)
        return fail(h, DTTS_E_INVAL, "%s: %d windows (meldisc.%d.conv.0.weight is loaded); disc_win_num is 1 .. 3", PART, n_win, DTTS_MELDISC_MAX_WIN);
    int per_row = -1;
    for (int w = 0; w < n_win; ++w) {
        MelDiscWin& D = h->meldisc[w];
        const std::string base = "meldisc." + std::to_string(w);
        const int T3 = MELDISC_WINS[w] / 8, F3 = MELDISC_F / 8;
        for (int l = 0; l < 3; ++l) {
            const std::string cn = base + ".conv." + std::to_string(l);
            const HostTensor* cw = need.get(cn + ".weight");
            const HostTensor* cb = need.get(cn + ".bias");
            if (!cw || !cb) return missing();
            const int ci = l ? H : 1;
            if (cw->shape != std::vector<int64_t>({(int64_t)H, (int64_t)ci, 3, 3}) || cb->numel() != H)
                return fail(h, DTTS_E_INVAL, "%s: %s.weight is %s with %lld bias entries; the reference's layer is [%d, %d, 3, 3]", PART, cn.c_str(),
                            mshape(cw).c_str(), (long long)cb->numel(), H, ci);
            if (l == 0) {
                std::vector<float> t((size_t)9 * H);
                for (int c = 0; c < H; ++c)
                    for (int tap = 0; tap < 9; ++tap) t[(size_t)tap * H + c] = cw->f[(size_t)c * 9 + tap];
                D.w0 = upload(h, t);
                D.b0 = upload(h, cb->f);
                if (!D.w0 || !D.b0) return fail(h, DTTS_E_NOMEM, "%s: packing %s", PART, cn.c_str());
                continue;
            }
            const int nch = H / MELDISC_KC, ntl = H / 32;
            std::vector<float> pk((size_t)ntl * nch * 9 * 4 * 64 * 4);
            for (int n = 0; n < ntl; ++n)
                for (int ch = 0; ch < nch; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int q = 0; q < 4; ++q)
                            for (int ln = 0; ln < 64; ++ln)
                                for (int e = 0; e < 4; ++e) {
                                    const int o = n * 32 + (ln & 31), i = ch * MELDISC_KC + 8 * q + 4 * (ln >> 5) + e;
                                    pk[((((((size_t)n * nch + ch) * 9 + tap) * 4 + q) * 64 + ln) * 4) + e] = cw->f[((size_t)o * H + i) * 9 + tap];
                                }
            D.wp[l - 1] = upload(h, pk);
            D.bp[l - 1] = upload(h, cb->f);
            if (!D.wp[l - 1] || !D.bp[l - 1]) return fail(h, DTTS_E_NOMEM, "%s: packing %s", PART, cn.c_str());
            // the norm behind this block
            const std::string nn = base + ".norm." + std::to_string(l), an = base + ".affine." + std::to_string(l);
            const bool inst = h->w.count(nn + ".weight") || h->w.count(nn + ".bias");
            const bool aff = h->w.count(an + ".scale") || h->w.count(an + ".shift");
            if (inst && aff) return fail(h, DTTS_E_INVAL, "%s: both %s.* and %s.* are loaded; a block has one norm", PART, nn.c_str(), an.c_str());
            std::vector<float> shift((size_t)H, 0.f);
            std::vector<float2> fixed((size_t)H, make_float2(0.f, 1.f));
            if (inst || aff) {
                const HostTensor* a = need.get(inst ? nn + ".weight" : an + ".scale");
                const HostTensor* b = need.get(inst ? nn + ".bias" : an + ".shift");
                if (!a || !b) return missing();
                if (a->numel() != H || b->numel() != H)
                    return fail(h, DTTS_E_INVAL, "%s: %s has %lld and %lld entries for %d channels", PART, (inst ? nn : an).c_str(), (long long)a->numel(),
                                (long long)b->numel(), H);
                shift = b->f;
                if (inst) {
                    D.gamma[l - 1] = upload(h, a->f);
                    if (!D.gamma[l - 1]) return fail(h, DTTS_E_NOMEM, "%s: packing %s", PART, nn.c_str());
                } else
                    for (int c = 0; c < H; ++c) fixed[c].y = a->f[c];
            }
            D.norm[l - 1] = inst ? MELDISC_NORM_INSTANCE : (aff ? MELDISC_NORM_AFFINE : MELDISC_NORM_NONE);
            D.fixed[l - 1] = upload(h, fixed);
            D.shift[l - 1] = upload(h, shift);
            if (!D.fixed[l - 1] || !D.shift[l - 1]) return fail(h, DTTS_E_NOMEM, "%s: packing the norm of %s", PART, cn.c_str());
        }
        const HostTensor* aw = need.get(base + ".adv.weight");
        const HostTensor* ab = need.get(base + ".adv.bias");
        if (!aw || !ab) return missing();
        const int64_t flat = (int64_t)H * T3 * F3, row = (int64_t)H * F3;
        if ((aw->numel() != flat && aw->numel() != row) || ab->numel() != 1)
            return fail(h, DTTS_E_INVAL,
                        "%s: %s.adv.weight is %s with %lld bias entries; the %d-frame window's head has %lld inputs (disc_reduction stack / sum) or %lld (none)",
                        PART, base.c_str(), mshape(aw).c_str(), (long long)ab->numel(), MELDISC_WINS[w], (long long)flat, (long long)row);
        const int pr = aw->numel() == row ? 1 : 0;
        if (per_row >= 0 && pr != per_row)
            return fail(h, DTTS_E_INVAL, "%s: %s.adv.weight is %s: a head %s, while meldisc.0's is %s", PART, base.c_str(), mshape(aw).c_str(),
                        pr ? "per time row (disc_reduction none)" : "over the whole map", per_row ? "per time row" : "over the whole map");
        per_row = pr;
        const int Th = pr ? 1 : T3;
        std::vector<float> t((size_t)aw->numel());
        for (int c = 0; c < H; ++c)
            for (int tt = 0; tt < Th; ++tt)
                for (int f = 0; f < F3; ++f) t[((size_t)tt * F3 + f) * H + c] = aw->f[((size_t)c * Th + tt) * F3 + f];
        D.wh = upload(h, t);
        D.bh = ab->f[0];
        if (!D.wh) return fail(h, DTTS_E_NOMEM, "%s: packing %s.adv", PART, base.c_str());
    }
    h->meldisc_ident = upload(h, std::vector<float2>((size_t)H, make_float2(0.f, 1.f)));   // what a reader of block 1's map applies: nothing
    h->meldisc_zero = upload(h, std::vector<float>((size_t)H, 0.f));
    if (!h->meldisc_ident || !h->meldisc_zero) return fail(h, DTTS_E_NOMEM, "%s: packing the identity norm", PART);
    h->meldisc_H = H;
    h->meldisc_nwin = n_win;
    h->meldisc_per_row = per_row == 1;
    h->meldisc_ready = true;
    return DTTS_OK;
}

// =====================================================================================================================================
// forward

// h may be null: the block is checked first, so that the refusals are reachable without a device
int meldisc_forward(dtts_ctx* h, const dtts_meldisc_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_MELDISC)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->n_sig < 1 || a->n_sig > 65535) return fail(h, DTTS_E_INVAL, "%s: n_sig = %d (supported: 1 .. 65535)", me, a->n_sig);
    if (a->T_ld < 1 || a->T_ld > (1 << 20)) return fail(h, DTTS_E_INVAL, "%s: T_ld = %d frames (supported: 1 .. %d)", me, a->T_ld, 1 << 20);
    if (a->n_win < 1 || a->n_win > DTTS_MELDISC_MAX_WIN) return fail(h, DTTS_E_INVAL, "%s: n_win = %d (disc_win_num is 1 .. 3)", me, a->n_win);
    if (a->reduction != DTTS_MELDISC_STACK && a->reduction != DTTS_MELDISC_SUM && a->reduction != DTTS_MELDISC_NONE)
        return fail(h, DTTS_E_INVAL, "%s: reduction = %d (DTTS_MELDISC_STACK = 0, DTTS_MELDISC_SUM = 1, DTTS_MELDISC_NONE = 2)", me, a->reduction);
    if (a->flags & ~DTTS_MELDISC_WITHIN_LEN) return fail(h, DTTS_E_INVAL, "%s: flags = %d (DTTS_MELDISC_WITHIN_LEN = 1)", me, a->flags);
    if (a->clips_ld < 1 || a->clips_ld > 65536 || (long long)a->n_sig * a->clips_ld > (1ll << 24))
        return fail(h, DTTS_E_INVAL, "%s: clips_ld = %d for n_sig = %d (supported: 1 .. 65536, n_sig * clips_ld up to 2^24)", me, a->clips_ld, a->n_sig);
    if (!a->starts_dev)
        for (int w = 0; w < a->n_win; ++w)
            if (a->hop[w] < 1) return fail(h, DTTS_E_INVAL, "%s: hop[%d] = %d frames without starts_dev (must be at least 1)", me, w, a->hop[w]);
    if (a->reserved[0] != 0 || a->reserved[1] != 0) return fail(h, DTTS_E_INVAL, "%s: reserved = %d, %d (must be 0)", me, a->reserved[0], a->reserved[1]);
    if (!a->mel_dev || !a->sums_dev || !a->counts_dev || !a->status_dev)
        return fail(h, DTTS_E_INVAL, "%s: null mel_dev / sums_dev / counts_dev / status_dev", me);
    if (int rc = blk.aligned(4, {{"mel_dev", a->mel_dev}, {"lens_dev", a->lens_dev}, {"starts_dev", a->starts_dev}, {"d_dev", a->d_dev}, {"status_dev", a->status_dev},
                                 {"h_dev[0]", a->h_dev[0]}, {"h_dev[1]", a->h_dev[1]}, {"h_dev[2]", a->h_dev[2]}, {"h_dev[3]", a->h_dev[3]}, {"h_dev[4]", a->h_dev[4]},
                                 {"h_dev[5]", a->h_dev[5]}, {"h_dev[6]", a->h_dev[6]}, {"h_dev[7]", a->h_dev[7]}, {"h_dev[8]", a->h_dev[8]}}))
        return rc;
    if (int rc = blk.aligned(8, {{"sums_dev", a->sums_dev}, {"counts_dev", a->counts_dev}})) return rc;
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_MELDISC)) return rc;
    if (a->n_win != h->meldisc_nwin) return fail(h, DTTS_E_INVAL, "%s: n_win = %d, the loaded discriminator has %d windows", me, a->n_win, h->meldisc_nwin);
    if ((a->reduction == DTTS_MELDISC_NONE) != h->meldisc_per_row)
        return fail(h, DTTS_E_INVAL, "%s: reduction = %d, the loaded adv_layer is %s", me, a->reduction,
                    h->meldisc_per_row ? "per time row (disc_reduction none)" : "over the whole map (stack / sum)");

    const int H = h->meldisc_H, n_sig = a->n_sig, cl = a->clips_ld, n_win = a->n_win;
    const int wmax = MELDISC_WINS[n_win - 1];
    const size_t tot = (size_t)n_sig * cl;
    // floats per clip slot of the largest window: the three maps, the two statistics tables, the D row
    const size_t a1 = (size_t)(wmax / 2) * 40 * H, a2 = (size_t)(wmax / 4) * 20 * H, a3 = (size_t)(wmax / 8) * 10 * H;
    const size_t per_clip = (a1 + a2 + a3 + 4 * (size_t)H + DTTS_MELDISC_D_LD) * sizeof(float);
    const size_t tab = (tot * DTTS_MELDISC_MAX_WIN + n_sig) * sizeof(int) + 2 * 256;
    const int Sc = chunk_within(n_sig, DTTS_MELDISC_WS_BYTES, [&](int n) { return per_clip * cl * n; });
    HIPCHK(h->a_meldisc.reserve(per_clip * cl * Sc + tab + 16 * 256, stream));
    Arena& ws = h->a_meldisc;
    int* vlen = ws.alloc<int>((size_t)n_sig);
    int* cst = ws.alloc<int>(tot * DTTS_MELDISC_MAX_WIN);
    const size_t nc = (size_t)Sc * cl;
    float* act1 = ws.alloc<float>(a1 * nc);
    float* act2 = ws.alloc<float>(a2 * nc);
    float* act3 = ws.alloc<float>(a3 * nc);
    float2* nrm[2] = {ws.alloc<float2>((size_t)H * nc), ws.alloc<float2>((size_t)H * nc)};
    float* dws = ws.alloc<float>((size_t)DTTS_MELDISC_D_LD * nc);
    if (!vlen || !cst || !act1 || !act2 || !act3 || !nrm[0] || !nrm[1] || !dws) return blk.workspace();

    MelHops hops{};
    for (int w = 0; w < DTTS_MELDISC_MAX_WIN; ++w) hops.hop[w] = a->hop[w];
    hipLaunchKernelGGL(meldisc_clips_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, a->lens_dev, a->starts_dev, n_sig, a->T_ld, cl, n_win,
                       hops, a->flags & DTTS_MELDISC_WITHIN_LEN, vlen, cst, a->status_dev);
    LAUNCH(hipGetLastError());

    for (int s0 = 0; s0 < n_sig; s0 += Sc) {
        const int S = std::min(Sc, n_sig - s0);
        const unsigned nclip = (unsigned)((size_t)S * cl);
        for (int w = 0; w < n_win; ++w) {
            const MelDiscWin& D = h->meldisc[w];
            const int win = MELDISC_WINS[w];
            const int* c0 = cst + (size_t)w * tot + (size_t)s0 * cl;
            const int T[4] = {win, win / 2, win / 4, win / 8}, F[4] = {80, 40, 20, 10};
            float* act[3] = {act1, act2, act3};
            MelEntryParams e{};
            e.mel = a->mel_dev + (size_t)s0 * a->T_ld * MELDISC_F;
            e.vlen = vlen + s0;
            e.cst = c0;
            e.w = D.w0;
            e.bias = D.b0;
            e.y = act1;
            e.clips_ld = cl;
            e.T_ld = a->T_ld;
            e.win = win;
            e.H = H;
            hipLaunchKernelGGL(meldisc_entry_kernel, dim3(nclip, (unsigned)((T[1] * F[1] * H + MELDISC_THREADS - 1) / MELDISC_THREADS)), dim3(MELDISC_THREADS), 0,
                               stream, e);
            LAUNCH(hipGetLastError());
            // the (mean, scale) rows and the shift a reader of map l applies (l = 0: block 1's map has no norm)
            const float2* rd_nrm[3] = {h->meldisc_ident, nullptr, nullptr};
            const float* rd_shift[3] = {h->meldisc_zero, nullptr, nullptr};
            int rd_ld[3] = {0, 0, 0};
            for (int l = 1; l < 3; ++l) {
                MelConvParams p{};
                p.x = act[l - 1];
                p.y = act[l];
                p.w = D.wp[l - 1];
                p.bias = D.bp[l - 1];
                p.nrm = rd_nrm[l - 1];
                p.nrm_ld = rd_ld[l - 1];
                p.shift = rd_shift[l - 1];
                p.cst = c0;
                p.H = H;
                p.Tin = T[l];
                p.Fin = F[l];
                p.Tout = T[l + 1];
                p.Fout = F[l + 1];
                meldisc_tile_shape(p.Tout, p.Fout, &p.TR, &p.FC);
                p.fc_shift = __builtin_ctz((unsigned)p.FC);
                p.ntf = (p.Fout + p.FC - 1) / p.FC;
                p.nch = H / MELDISC_KC;
                const dim3 grid(nclip, (unsigned)(((p.Tout + p.TR - 1) / p.TR) * p.ntf), (unsigned)((H + 127) / 128));
                hipLaunchKernelGGL(meldisc_conv_kernel, grid, dim3(MELDISC_THREADS), meldisc_conv_lds(p.TR, p.FC), stream, p);
                LAUNCH(hipGetLastError());
                if (D.norm[l - 1] == MELDISC_NORM_INSTANCE) {
                    MelStatParams q{};
                    q.x = act[l];
                    q.cst = c0;
                    q.gamma = D.gamma[l - 1];
                    q.nrm = nrm[l - 1];
                    q.P = T[l + 1] * F[l + 1];
                    q.H = H;
                    q.G = MELDISC_THREADS / H;
                    hipLaunchKernelGGL(meldisc_stats_kernel, dim3(nclip), dim3((unsigned)(q.G * H)), 0, stream, q);
                    LAUNCH(hipGetLastError());
                    rd_nrm[l] = nrm[l - 1];
                    rd_ld[l] = H;
                } else {
                    rd_nrm[l] = D.fixed[l - 1];
                    rd_ld[l] = 0;
                }
                rd_shift[l] = D.shift[l - 1];
            }
            MelHeadParams q{};
            q.x = act3;
            q.cst = c0;
            q.nrm = rd_nrm[2];
            q.nrm_ld = rd_ld[2];
            q.shift = rd_shift[2];
            q.w = D.wh;
            q.dws = dws;
            q.bias = D.bh;
            q.H = H;
            q.n_out = h->meldisc_per_row ? T[3] : 1;
            q.n = T[3] * F[3] * H / q.n_out;
            hipLaunchKernelGGL(meldisc_head_kernel, dim3(nclip, (unsigned)q.n_out), dim3(MELDISC_THREADS), 0, stream, q);
            LAUNCH(hipGetLastError());
            MelScoreParams sc{};
            sc.dws = dws;
            sc.cst = c0;
            sc.sums = a->sums_dev + ((size_t)s0 * 3 + w) * 2;
            sc.counts = (long long*)a->counts_dev + (size_t)s0 * 3 + w;
            sc.d = a->d_dev ? a->d_dev + ((size_t)w * n_sig + s0) * cl * DTTS_MELDISC_D_LD : nullptr;
            sc.clips_ld = cl;
            sc.n_out = q.n_out;
            hipLaunchKernelGGL(meldisc_score_kernel, dim3((unsigned)S), dim3(MELDISC_THREADS), 0, stream, sc);
            LAUNCH(hipGetLastError());
            for (int l = 0; l < 3; ++l) {
                float* out = a->h_dev[3 * w + l];
                if (!out) continue;
                const int n = T[l + 1] * F[l + 1] * H;
                hipLaunchKernelGGL(meldisc_export_kernel, dim3(nclip, (unsigned)((n + MELDISC_THREADS - 1) / MELDISC_THREADS)), dim3(MELDISC_THREADS), 0, stream,
                                   (const float*)act[l], c0, l ? rd_nrm[l] : (const float2*)nullptr, rd_ld[l], rd_shift[l], out + (size_t)s0 * cl * n, n, H);
                LAUNCH(hipGetLastError());
            }
        }
    }
    return DTTS_OK;
}

} // namespace dtts
