// libdicttts_hip.so — the d-vector speaker encoder on B recordings (spkenc.h; dtts_text2mel_fetch(DTTS_OUT_SPKENC)).  Per chunk of utterances:
// the plan (partial counts, their prefix sum and the sequence tables, on the device), the power-mel front end, then per LSTM layer the input
// projection of all steps on conv1d_launch (k = 1, exact fp32 products, fixed order) and the recurrent kernel, then relu(linear) + the row
// norm per sequence and the mean over an utterance's partials + the norm.  Nothing goes through the host.
#include "ctx.h"

namespace dtts {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// ---- the plan of a chunk: one workgroup.  Thread 0 walks the utterances in order (the prefix sum), then all threads fill the tables
struct SpkPlanParams {
    const int* lens;      // [B] or null = wav_ld
    int B, b0, wav_ld, frame_step, mode, T, P_max, F_ld, N_cap;
    double min_coverage;
    int *vlen, *padlen, *frames, *np, *first, *total;   // [B] x 5, [1]
    int *row0, *seq_out, *seq_len;                      // [N_cap]
    int* np_user;                                       // [B] (this chunk's rows)
};
__global__ __launch_bounds__(256) void spkenc_plan_kernel(const SpkPlanParams p) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        int run = 0;
        for (int b = 0; b < p.B; ++b) {
            int count = 1, L = p.T, Lp = p.T;
            if (p.mode == DTTS_SPKENC_FROM_WAV) {
                L = p.lens ? p.lens[b] : p.wav_ld;
                L = L < 0 ? 0 : (L > p.wav_ld ? p.wav_ld : L);
                const int n_frames = L / SPK_HOP + 1;                       // ceil((L + 1) / 160)
                const int steps = max(1, n_frames - SPK_PART + p.frame_step + 1);
                count = (steps - 1) / p.frame_step + 1;
                const int last = (count - 1) * p.frame_step * SPK_HOP;      // first sample of the last partial
                if (count > 1 && (double)(L - last) / (double)(SPK_PART * SPK_HOP) < p.min_coverage) --count;
                Lp = max(L, SPK_HOP * ((count - 1) * p.frame_step + SPK_PART));
            }
            p.vlen[b] = L;
            p.padlen[b] = Lp;
            p.frames[b] = p.mode == DTTS_SPKENC_FROM_WAV ? 1 + Lp / SPK_HOP : p.T;
            p.np[b] = count;
            p.np_user[b] = count;
            p.first[b] = run;
            run += count;
        }
        p.total[0] = run;
    }
    __syncthreads();
    const int total = p.total[0];
    for (int idx = tid; idx < p.B * p.P_max; idx += 256) {
        const int b = idx / p.P_max, i = idx - b * p.P_max;
        if (i >= p.np[b]) continue;
        const int n = p.first[b] + i;
        p.row0[n] = b * p.F_ld + i * p.frame_step;          // (from mels: P_max = 1, F_ld = T, so row0 = b * T)
        p.seq_out[n] = (p.b0 + b) * p.P_max + i;
        p.seq_len[n] = p.T;
    }
    for (int n = total + tid; n < p.N_cap; n += 256) {
        p.row0[n] = -1;
        p.seq_out[n] = -1;
        p.seq_len[n] = 0;
    }
}

// ---- the front end: SPK_MEL_FRAMES centred frames of one utterance per workgroup.  Thread c < 402 owns one column of the windowed DFT
// basis (re or im of one bin) and sums its 400 exact fp32 products per frame in a fixed order; then thread (frame, band) sums band's 201 weighted powers
// in bin order.  Samples behind the utterance's length read as zero up to its padded length; outside that, zero or the reflection.
struct SpkMelParams {
    const float* wav;      // [B][wav_ld]
    const int *vlen, *padlen, *frames;
    const float* basis;    // [400][402]: w[n] cos, -w[n] sin of bin k at columns 2 k, 2 k + 1
    const float* fb;       // [40][201]
    float* mel;            // [B][F_ld][40]
    float* mel_user;       // the same layout, or null
    int wav_ld, F_ld, reflect;
};
__global__ __launch_bounds__(SPK_MEL_THREADS) void spkenc_mel_kernel(const SpkMelParams p) {
    constexpr int SPAN = (SPK_MEL_FRAMES - 1) * SPK_HOP + SPK_NFFT, NC = 2 * SPK_BINS;
    __shared__ float xs[SPAN];
    __shared__ float spec[SPK_MEL_FRAMES * NC];
    const int b = blockIdx.y, f0 = blockIdx.x * SPK_MEL_FRAMES, tid = threadIdx.x;
    const int frames = p.frames[b];
    if (f0 >= frames) return;
    const int L = p.vlen[b], Lp = p.padlen[b];
    const float* x = p.wav + (size_t)b * p.wav_ld;
    for (int j = tid; j < SPAN; j += SPK_MEL_THREADS) {
        int s = f0 * SPK_HOP + j - SPK_NFFT / 2;
        if (p.reflect) {
            if (s < 0) s = -s;
            if (s >= Lp) s = 2 * (Lp - 1) - s;
        }
        xs[j] = (s >= 0 && s < L) ? x[s] : 0.f;
    }
    __syncthreads();
    if (tid < NC) {
        // FIXED order: 16 fma chains of 25 consecutive n, four of them added in order to a group sum, the four group sums in order to the
        // total (a single chain of 400 carries 2 - 3 x the rounding error: LABNOTES.md "Speaker encoder")
        float acc[SPK_MEL_FRAMES], grp[SPK_MEL_FRAMES], seg[SPK_MEL_FRAMES];
#pragma unroll
        for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) acc[fr] = 0.f;
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) grp[fr] = 0.f;
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) seg[fr] = 0.f;
                const int n0 = (g * 4 + s) * SPK_MEL_CHAIN;
                for (int n = n0; n < n0 + SPK_MEL_CHAIN; ++n) {
                    const float bv = p.basis[n * NC + tid];
#pragma unroll
                    for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) seg[fr] = fmaf(bv, xs[fr * SPK_HOP + n], seg[fr]);
                }
#pragma unroll
                for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) grp[fr] += seg[fr];
            }
#pragma unroll
            for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) acc[fr] += grp[fr];
        }
#pragma unroll
        for (int fr = 0; fr < SPK_MEL_FRAMES; ++fr) spec[fr * NC + tid] = acc[fr];
    }
    __syncthreads();
    for (int o = tid; o < SPK_MEL_FRAMES * SPK_MELS; o += SPK_MEL_THREADS) {
        const int fr = o / SPK_MELS, m = o - fr * SPK_MELS;
        if (f0 + fr >= frames) continue;
        float acc = 0.f;
        for (int k = 0; k < SPK_BINS; ++k) {
            const float re = spec[fr * NC + 2 * k], im = spec[fr * NC + 2 * k + 1];
            acc = fmaf(p.fb[m * SPK_BINS + k], fmaf(im, im, re * re), acc);
        }
        const size_t at = ((size_t)b * p.F_ld + f0 + fr) * SPK_MELS + m;
        p.mel[at] = acc;
        if (p.mel_user) p.mel_user[at] = acc;
    }
}

// ---- the recurrence of one layer: a workgroup owns tile_m <= 32 sequences for all T steps.  h_t lives in LDS (the A operand), c_t in
// registers; wave w holds the four gates of hidden units [32 w, 32 w + 32) of every row: acc[q][r] is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5),
// unit 32 w + (lane & 31).  Per step W_hh streams from L2 in packed order (spkenc.h), one fp32 chain per gate over k in steps of
// (8 Q + e, 8 Q + 4 + e); the input projection is added to the finished chain.  No workgroup waits on another.
__device__ __forceinline__ float sigmoid_safe(float v) {
    const float e = expf(-fabsf(v));            // in (0, 1]: no overflow, no inf / inf
    return (v >= 0.f ? 1.f : e) / (1.f + e);
}
__device__ __forceinline__ float tanh_safe(float v) {
    const float m = expm1f(-2.f * fabsf(v));    // exp(-2 |v|) - 1 in (-1, 0], accurate near 0 where 1 - exp(.) would cancel
    return copysignf(-m / (m + 2.f), v);
}

struct SpkLstmParams {
    const float* xproj;    // rows of 1024: row0[n] + t
    const int *row0, *seq_out, *total;   // row0 null: sequence n's rows start at n * T
    const float* whh;
    float* hseq;           // [N_cap][T][256]
    float* hseq_user;      // [.][T][256] at seq_out[n], or null
    int T, tile_m;
};
__global__ __launch_bounds__(512) void spkenc_lstm_kernel(const SpkLstmParams p) {
    __shared__ __attribute__((aligned(16))) float hl[SPK_TILE * SPK_HP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, j = lane & 31;
    const int total = p.total[0], n0 = blockIdx.x * p.tile_m;
    if (n0 >= total) return;
    int xr[16];   // first projection row of the accumulator's sequence, -1 = no sequence in this row of the tile
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * hh;
        const bool ok = i < p.tile_m && n0 + i < total;
        xr[r] = ok ? (p.row0 ? p.row0[n0 + i] : (n0 + i) * p.T) : -1;
    }
    for (int idx = tid; idx < SPK_TILE * SPK_HP; idx += 512) hl[idx] = 0.f;
    float c[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    __syncthreads();
    const int col = w * 32 + j;
    const f32x4* wp = (const f32x4*)p.whh + (size_t)w * 32 * 4 * 64 + lane;
    for (int t = 0; t < p.T; ++t) {
        float xp[4][16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* src = p.xproj + ((size_t)(xr[r] < 0 ? 0 : xr[r]) + t) * SPK_G + col;
#pragma unroll
            for (int q = 0; q < 4; ++q) xp[q][r] = xr[r] >= 0 ? src[q * SPK_H] : 0.f;
        }
        f32x16 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        f32x4 bq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bq[q] = wp[q * 64];
        for (int Q = 0; Q < 32; ++Q) {
            const int Qn = Q < 31 ? Q + 1 : 31;
            f32x4 bn[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bn[q] = wp[(Qn * 4 + q) * 64];
            const f32x4 a = *(const f32x4*)(hl + j * SPK_HP + 8 * Q + 4 * hh);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bq[q][e], acc[q], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) bq[q] = bn[q];
        }
        __syncthreads();   // every wave has read h_{t-1}
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * hh;
            float hv = 0.f;
            if (xr[r] >= 0) {
                const float gi = sigmoid_safe(acc[0][r] + xp[0][r]), gf = sigmoid_safe(acc[1][r] + xp[1][r]);
                const float gg = tanh_safe(acc[2][r] + xp[2][r]), go = sigmoid_safe(acc[3][r] + xp[3][r]);
                c[r] = gf * c[r] + gi * gg;
                hv = go * tanh_safe(c[r]);
                p.hseq[((size_t)(n0 + i) * p.T + t) * SPK_H + col] = hv;
                if (p.hseq_user) p.hseq_user[((size_t)p.seq_out[n0 + i] * p.T + t) * SPK_H + col] = hv;
            }
            hl[i * SPK_HP + col] = hv;
        }
        __syncthreads();
    }
}

// fixed tree over the workgroup's 256 fp64 values
__device__ __forceinline__ double spk_tree(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

// ---- relu(linear(h_T)) and the row norm: one workgroup per sequence, thread o owns output o (one chain over k, then the bias).
// A row of zeros divides to NaN, as the reference's does
struct SpkEmbedParams {
    const float* hseq;     // [N_cap][T][256]
    const int *total, *seq_out;
    const float *wt, *bias;   // linear.weight transposed [k][o], [o]
    float* part;           // [N_cap][256]
    float* part_user;      // [.][256] at seq_out[n], or null
    int T;
};
__global__ __launch_bounds__(256) void spkenc_embed_kernel(const SpkEmbedParams p) {
    __shared__ float hs[SPK_H];
    __shared__ double red[256];
    const int n = blockIdx.x, o = threadIdx.x;
    if (n >= p.total[0]) return;
    hs[o] = p.hseq[((size_t)n * p.T + p.T - 1) * SPK_H + o];
    __syncthreads();
    float acc = 0.f;
    for (int k = 0; k < SPK_H; ++k) acc = fmaf(p.wt[k * SPK_H + o], hs[k], acc);
    const float y = fmaxf(acc + p.bias[o], 0.f);
    const float nrm = (float)sqrt(spk_tree((double)y * (double)y, red));
    const float v = y / nrm;
    p.part[(size_t)n * SPK_H + o] = v;
    if (p.part_user) p.part_user[(size_t)p.seq_out[n] * SPK_H + o] = v;
}

// ---- per utterance: the mean over its partials (an fp64 sum in partial order, rounded once), then the norm
__global__ __launch_bounds__(256) void spkenc_utt_kernel(const float* part, const int* np, const int* first, float* embed) {
    __shared__ double red[256];
    const int b = blockIdx.x, o = threadIdx.x;
    const int P = np[b], f = first[b];
    double s = 0.0;
    for (int i = 0; i < P; ++i) s += (double)part[(size_t)(f + i) * SPK_H + o];
    const float mean = (float)(s / (double)P);
    const float nrm = (float)sqrt(spk_tree((double)mean * (double)mean, red));
    embed[(size_t)b * SPK_H + o] = mean / nrm;
}

// =====================================================================================================================================
// weights
namespace {

std::string shape_of(const HostTensor* t) {
    std::string s = "[";
    for (size_t i = 0; i < t->shape.size(); ++i) s += (i ? ", " : "") + std::to_string((long long)t->shape[i]);
    return s + "]";
}

// the tensor `name` of exactly `want`, or null after recording in rc why not (a missing one is recorded by `need`)
const HostTensor* spk_tensor(dtts_ctx* h, Need& need, const std::string& name, std::vector<int64_t> want, int* rc) {
    const HostTensor* t = need.get(name);
    if (!t) return nullptr;
    if (t->shape != want || t->f.size() != (size_t)t->numel()) {
        HostTensor w;
        w.shape = want;
        *rc = fail(h, DTTS_E_INVAL, "dtts_finalize_weights(DTTS_PART_SPKENC): %s is %s; the encoder's is %s", name.c_str(), shape_of(t).c_str(),
                   shape_of(&w).c_str());
        return nullptr;
    }
    return t;
}

} // namespace

int build_spkenc(dtts_ctx* h) {
    Need need{h};
    int rc = DTTS_OK;
    auto done = [&]() {
        if (rc != DTTS_OK) return rc;
        return fail(h, DTTS_E_NOENT, "dtts_finalize_weights(DTTS_PART_SPKENC): missing tensor %s", need.missing.c_str());
    };
    auto nomem = [&](const char* what) { return fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_SPKENC): packing %s", what); };
    for (int l = 0; l < SPK_LAYERS; ++l) {
        const std::string s = std::to_string(l);
        const int ci = l == 0 ? SPK_MELS : SPK_H;
        const HostTensor* wih = spk_tensor(h, need, "spkenc.lstm.weight_ih_l" + s, {SPK_G, ci}, &rc);
        if (!wih) return done();
        const HostTensor* whh = spk_tensor(h, need, "spkenc.lstm.weight_hh_l" + s, {SPK_G, SPK_H}, &rc);
        if (!whh) return done();
        const HostTensor* bih = spk_tensor(h, need, "spkenc.lstm.bias_ih_l" + s, {SPK_G}, &rc);
        if (!bih) return done();
        const HostTensor* bhh = spk_tensor(h, need, "spkenc.lstm.bias_hh_l" + s, {SPK_G}, &rc);
        if (!bhh) return done();
        std::vector<float> bias(SPK_G);
        for (int o = 0; o < SPK_G; ++o) bias[o] = bih->f[o] + bhh->f[o];
        const float* pw = wih->f.data();
        if (!pack_conv(h, h->spk_layer[l].proj, ENG_F32, SPK_G, ci, 1, [=](int o, int i, int) { return pw[(size_t)o * ci + i]; }, bias, 1, 1, 0))
            return nomem(("lstm.weight_ih_l" + s).c_str());
        std::vector<float> pk((size_t)SPK_G * SPK_H);
        for (int w = 0; w < 8; ++w)
            for (int Q = 0; Q < 32; ++Q)
                for (int q = 0; q < 4; ++q)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e)
                            pk[spkenc_whh_index(w, Q, q, lane, e)] = whh->f[(size_t)(q * SPK_H + 32 * w + (lane & 31)) * SPK_H + 8 * Q + 4 * (lane >> 5) + e];
        if (!(h->spk_layer[l].whh = upload(h, pk))) return nomem(("lstm.weight_hh_l" + s).c_str());
    }
    const HostTensor* lw = spk_tensor(h, need, "spkenc.linear.weight", {SPK_H, SPK_H}, &rc);
    if (!lw) return done();
    const HostTensor* lb = spk_tensor(h, need, "spkenc.linear.bias", {SPK_H}, &rc);
    if (!lb) return done();
    const HostTensor* fb = spk_tensor(h, need, "spkenc.mel_basis", {SPK_MELS, SPK_BINS}, &rc);
    if (!fb) return done();
    const HostTensor* win = spk_tensor(h, need, "spkenc.window", {SPK_NFFT}, &rc);
    if (!win) return done();
    std::vector<float> wt((size_t)SPK_H * SPK_H);
    for (int o = 0; o < SPK_H; ++o)
        for (int k = 0; k < SPK_H; ++k) wt[(size_t)k * SPK_H + o] = lw->f[(size_t)o * SPK_H + k];
    // the windowed basis in fp64, rounded once; the angle from the exact residue of k n mod 400
    std::vector<float> basis((size_t)SPK_NFFT * 2 * SPK_BINS);
    for (int n = 0; n < SPK_NFFT; ++n)
        for (int k = 0; k < SPK_BINS; ++k) {
            const double ang = 2.0 * M_PI * (double)((k * n) % SPK_NFFT) / (double)SPK_NFFT, wn = (double)win->f[n];
            basis[((size_t)n * SPK_BINS + k) * 2] = (float)(wn * cos(ang));
            basis[((size_t)n * SPK_BINS + k) * 2 + 1] = (float)(-wn * sin(ang));
        }
    h->spk_lin_wt = upload(h, wt);
    h->spk_lin_b = upload(h, lb->f);
    h->spk_fb = upload(h, fb->f);
    h->spk_basis = upload(h, basis);
    if (!h->spk_lin_wt || !h->spk_lin_b || !h->spk_fb || !h->spk_basis) return nomem("linear / mel_basis / window");
    h->spkenc_ready = true;
    return DTTS_OK;
}

// =====================================================================================================================================
// forward
namespace {

struct SpkShape {
    int T, P_max, F_ld;
};

// workspace bytes of a chunk of Bc utterances
size_t spk_bytes(const SpkShape& s, int Bc, bool from_wav) {
    const size_t N = (size_t)Bc * s.P_max;
    const size_t xrows = std::max((size_t)Bc * s.F_ld, N * s.T);
    return (from_wav ? (size_t)Bc * s.F_ld * SPK_MELS : 0) * sizeof(float) + xrows * SPK_G * sizeof(float) + 2 * N * s.T * SPK_H * sizeof(float) +
           N * SPK_H * sizeof(float) + (5 * (size_t)Bc + 3 * N + 1) * sizeof(int) + 16 * 256;
}

} // namespace

// h may be null: the block is checked first, so that the refusals are reachable without a device
int spkenc_forward(dtts_ctx* h, const dtts_spkenc_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_SPKENC)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->mode != DTTS_SPKENC_FROM_WAV && a->mode != DTTS_SPKENC_FROM_MELS)
        return fail(h, DTTS_E_INVAL, "%s: mode = %d (DTTS_SPKENC_FROM_WAV = 0 or DTTS_SPKENC_FROM_MELS = 1)", me, a->mode);
    const bool from_wav = a->mode == DTTS_SPKENC_FROM_WAV;
    if (a->B < 1 || a->B > 65535) return fail(h, DTTS_E_INVAL, "%s: B = %d (supported: 1 .. 65535)", me, a->B);
    if (from_wav && (a->wav_ld < 1 || a->wav_ld > (1 << 24))) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 1 .. %d)", me, a->wav_ld, 1 << 24);
    if (!from_wav && (a->wav_ld < 1 || a->wav_ld > DTTS_SPKENC_MAX_T))
        return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d frames per sequence (DTTS_SPKENC_FROM_MELS; supported: 1 .. %d)", me, a->wav_ld, DTTS_SPKENC_MAX_T);
    if (from_wav && (a->frame_step < 1 || a->frame_step > 4096)) return fail(h, DTTS_E_INVAL, "%s: frame_step = %d (supported: 1 .. 4096)", me, a->frame_step);
    if (from_wav && !(a->min_coverage > 0.0 && a->min_coverage <= 1.0))
        return fail(h, DTTS_E_INVAL, "%s: min_coverage = %g (must lie in (0, 1])", me, a->min_coverage);
    if (a->pad_mode != DTTS_SPKENC_PAD_CONSTANT && a->pad_mode != DTTS_SPKENC_PAD_REFLECT)
        return fail(h, DTTS_E_INVAL, "%s: pad_mode = %d (DTTS_SPKENC_PAD_CONSTANT = 0 or DTTS_SPKENC_PAD_REFLECT = 1)", me, a->pad_mode);
    if (a->tile_m != 0 && a->tile_m != 16 && a->tile_m != 32) return fail(h, DTTS_E_INVAL, "%s: tile_m = %d (0 = the default, 16 or 32)", me, a->tile_m);
    if (a->reserved != 0) return fail(h, DTTS_E_INVAL, "%s: reserved = %d (must be 0)", me, a->reserved);
    if (!a->wav_dev || !a->embed_dev || !a->n_partials_dev) return fail(h, DTTS_E_INVAL, "%s: null wav_dev / embed_dev / n_partials_dev", me);
    if (!from_wav && (a->lens_dev || a->mel_dev)) return fail(h, DTTS_E_INVAL, "%s: lens_dev / mel_dev with DTTS_SPKENC_FROM_MELS (wav_dev holds the mels)", me);
    if (int rc = blk.aligned(4, {{"wav_dev", a->wav_dev}, {"lens_dev", a->lens_dev}, {"embed_dev", a->embed_dev}, {"n_partials_dev", a->n_partials_dev},
                                 {"partials_dev", a->partials_dev}, {"mel_dev", a->mel_dev}, {"hseq_dev[0]", a->hseq_dev[0]}, {"hseq_dev[1]", a->hseq_dev[1]},
                                 {"hseq_dev[2]", a->hseq_dev[2]}}))
        return rc;
    if (!from_wav && ((uintptr_t)a->wav_dev & 15)) return fail(h, DTTS_E_INVAL, "%s: wav_dev = %p (the mels) is not aligned to 16 bytes", me, (const void*)a->wav_dev);
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_SPKENC)) return rc;

    SpkShape s;
    s.T = from_wav ? SPK_PART : a->wav_ld;
    s.P_max = from_wav ? spkenc_max_partials(a->wav_ld, a->frame_step) : 1;
    s.F_ld = from_wav ? spkenc_frames_ld(a->wav_ld, a->frame_step) : s.T;
    // (at most 1 361 partials per utterance at 2^24 samples; conv1d takes 65535 sequences)
    const int Bc = chunk_within(std::min(a->B, 65535 / s.P_max), DTTS_SPKENC_WS_BYTES, [&](int n) { return spk_bytes(s, n, from_wav); });
    HIPCHK(h->a_spkenc.reserve(spk_bytes(s, Bc, from_wav), stream));

    for (int b0 = 0; b0 < a->B; b0 += Bc) {
        const int B = std::min(Bc, a->B - b0), N = B * s.P_max;
        // 16 sequences per workgroup while that still leaves a compute unit to each workgroup (more of them run at once: LABNOTES.md), else 32
        const int tile_m = a->tile_m ? a->tile_m : (N <= 16 * h->n_cu ? 16 : DTTS_SPKENC_TILE_M);
        Arena& ws = h->a_spkenc;
        ws.rewind();
        int* tabs = ws.alloc<int>((size_t)5 * B + 3 * N + 1);
        float* mel = from_wav ? ws.alloc<float>((size_t)B * s.F_ld * SPK_MELS) : nullptr;
        float* xproj = ws.alloc<float>(std::max((size_t)B * s.F_ld, (size_t)N * s.T) * SPK_G);
        float* hs[2] = {ws.alloc<float>((size_t)N * s.T * SPK_H), ws.alloc<float>((size_t)N * s.T * SPK_H)};
        float* part = ws.alloc<float>((size_t)N * SPK_H);
        if (!tabs || (from_wav && !mel) || !xproj || !hs[0] || !hs[1] || !part) return blk.workspace();

        SpkPlanParams pp{};
        pp.lens = a->lens_dev ? a->lens_dev + b0 : nullptr;
        pp.B = B;
        pp.b0 = b0;
        pp.wav_ld = a->wav_ld;
        pp.frame_step = from_wav ? a->frame_step : 1;
        pp.mode = a->mode;
        pp.T = s.T;
        pp.P_max = s.P_max;
        pp.F_ld = s.F_ld;
        pp.N_cap = N;
        pp.min_coverage = a->min_coverage;
        pp.vlen = tabs;
        pp.padlen = tabs + B;
        pp.frames = tabs + 2 * B;
        pp.np = tabs + 3 * B;
        pp.first = tabs + 4 * B;
        pp.total = tabs + 5 * B;
        pp.row0 = tabs + 5 * B + 1;
        pp.seq_out = pp.row0 + N;
        pp.seq_len = pp.seq_out + N;
        pp.np_user = a->n_partials_dev + b0;
        hipLaunchKernelGGL(spkenc_plan_kernel, dim3(1), dim3(256), 0, stream, pp);
        LAUNCH(hipGetLastError());

        if (from_wav) {
            SpkMelParams mp{};
            mp.wav = a->wav_dev + (size_t)b0 * a->wav_ld;
            mp.vlen = pp.vlen;
            mp.padlen = pp.padlen;
            mp.frames = pp.frames;
            mp.basis = h->spk_basis;
            mp.fb = h->spk_fb;
            mp.mel = mel;
            mp.mel_user = a->mel_dev ? a->mel_dev + (size_t)b0 * s.F_ld * SPK_MELS : nullptr;
            mp.wav_ld = a->wav_ld;
            mp.F_ld = s.F_ld;
            mp.reflect = a->pad_mode == DTTS_SPKENC_PAD_REFLECT;
            hipLaunchKernelGGL(spkenc_mel_kernel, dim3((unsigned)((s.F_ld + SPK_MEL_FRAMES - 1) / SPK_MEL_FRAMES), (unsigned)B), dim3(SPK_MEL_THREADS), 0, stream, mp);
            LAUNCH(hipGetLastError());
        }
        const float* x0 = from_wav ? mel : a->wav_dev + (size_t)b0 * s.T * SPK_MELS;
        for (int l = 0; l < SPK_LAYERS; ++l) {
            const SpkLayer& L = h->spk_layer[l];
            ConvParams p = l == 0 ? base_params(x0, SPK_MELS, B, s.F_ld, s.F_ld, xproj, SPK_G) : base_params(hs[(l - 1) & 1], SPK_H, N, s.T, s.T, xproj, SPK_G);
            p.in_lens = p.out_lens = l == 0 ? pp.frames : pp.seq_len;
            p.fixed_order = 1;
            LAUNCH(conv1d_launch(L.proj, p, stream));
            SpkLstmParams q{};
            q.xproj = xproj;
            q.row0 = pp.row0;
            q.seq_out = pp.seq_out;
            q.total = pp.total;
            q.whh = L.whh;
            q.hseq = hs[l & 1];
            q.hseq_user = a->hseq_dev[l];
            q.T = s.T;
            q.tile_m = tile_m;
            // layers 1, 2 read the projection of the compact hidden sequences: row n * T
            if (l > 0) q.row0 = nullptr;
            hipLaunchKernelGGL(spkenc_lstm_kernel, dim3((unsigned)((N + tile_m - 1) / tile_m)), dim3(512), 0, stream, q);
            LAUNCH(hipGetLastError());
        }
        SpkEmbedParams ep{};
        ep.hseq = hs[(SPK_LAYERS - 1) & 1];
        ep.total = pp.total;
        ep.seq_out = pp.seq_out;
        ep.wt = h->spk_lin_wt;
        ep.bias = h->spk_lin_b;
        ep.part = part;
        ep.part_user = a->partials_dev;
        ep.T = s.T;
        hipLaunchKernelGGL(spkenc_embed_kernel, dim3((unsigned)N), dim3(256), 0, stream, ep);
        LAUNCH(hipGetLastError());
        hipLaunchKernelGGL(spkenc_utt_kernel, dim3((unsigned)B), dim3(256), 0, stream, (const float*)part, (const int*)pp.np, (const int*)pp.first,
                           a->embed_dev + (size_t)b0 * SPK_H);
        LAUNCH(hipGetLastError());
    }
    return DTTS_OK;
}

} // namespace dtts
