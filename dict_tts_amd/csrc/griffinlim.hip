// Griffin-Lim on the device: the reference's griffin_lim / griffin_lim_torch (utils/audio.py:35-42, 136-158) with _mel_to_linear
// (utils/audio.py:91-95) in front of it for mel input.  Per utterance of T frames
//     A = target magnitudes;  S = A init;  y = istft(S);  n_iter times { X = stft(y);  S = A X / |X|;  y = istft(S) }
// with stft / istft EXACTLY those of istft.hip: the inverse is istft_frames_kernel + istft_gather_kernel as they are, the forward is the
// shared contraction of stft_core.h under the forward launcher's rule (istft.h: spectral_forward_pick), with a third epilogue:
//
// PROJECTION (gl_project_kernel): re / im stay in the accumulators, the lane reads the 16 target magnitudes of its bins (four 16-byte loads
// from A [B][spec_cap][n_fft / 2 + 4]: the row pitch keeps every quad aligned, re[n_fft / 2]'s magnitude sits at column n_fft / 2),
// m = sqrt(fma(re, re, im im)), s = A / m, (re s, im s) leaves as the interleaved pair; m = 0 gives (A, 0), as np.angle(0) = 0 does.  Bins 0
// and n_fft / 2 are real: +A or -A by the sign of the value (+A for a zero of either sign), no division.  The frame count comes from the
// workspace (T frames in, hop (T - 1) samples between, T frames again), not from a length: the kernel writes no frame count.
//
// TARGET AND START (gl_target_kernel), one launch: A = |mag|, or max(1e-10, sum_j P[k][j] 10^mel[t][j]) as ONE fp32 FMA chain in ascending
// j per output (10^mel of eight frames staged in LDS once, P transposed so that a wave reads neighbouring bins); S0 = A init as two fp32
// products per bin (init = NULL: S0 = A); the clamped frame counts, for every later launch.
//
// A call is 1 + 2 + 3 n_iter launches on the caller's stream, no atomics, one summation order everywhere: an utterance is bit-identical
// alone and in any batch, and n_iter = 0 is the inverse of A init bit for bit.
#include "ctx.h"
#include "istft.h"

namespace dtts {

constexpr int GL_TT = 8;          // frames per workgroup of gl_target_kernel
constexpr int GL_THREADS = 256;
constexpr int GL_MAX_MELS = 128;  // melspec_supported's limit

struct GlProjParams {
    const float* mag;        // A [B][spec_cap][mag_ld], 16-byte aligned rows
    int mag_ld;              // n_fft / 2 + 4
    int tcap;                // frames are clamped to 0 .. tcap (<= spec_cap)
};

struct GlTargetParams {
    const float* mag;        // [B][spec_cap][bins], or null
    const float* mel;        // [B][spec_cap][n_mels], or null
    const float* pinv;       // [n_mels][bins] (mel)
    const float* init;       // [B][spec_cap][bins][2], or null
    const int* frames_in;    // [B], or null = spec_cap
    float* A;                // [B][spec_cap][a_ld] out
    float* spec;             // [B][spec_cap][bins][2] out
    int* frames;             // [B] out: clamped
    int B, spec_cap, bins, a_ld, n_mels, ntile;
};

// (The index arithmetic up to the contraction restates spectral_fwd_kernel's: that kernel is to compile to what it did, so nothing of it
// moved into a shared helper.  What differs: T comes from the workspace, the length follows from it, and no frame count is written.)
template <int WT>
__global__ __launch_bounds__(64 * WT) void gl_project_kernel(const SpecFwdParams p, const GlProjParams q) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fi = lane & 31, hf = lane >> 5;
    const int cg = blockIdx.x % p.csplit, bt = blockIdx.x / p.csplit, b = bt / p.g.ntile, tile = bt % p.g.ntile;
    int T = p.frames[b];
    T = T < 0 ? 0 : (T > q.tcap ? q.tcap : T);
    const int len = T > 0 ? p.g.hop * (T - 1) : 0;   // <= wav_ld = hop (spec_cap - 1): what the gather wrote
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
    const size_t rowi = (size_t)b * p.spec_cap + f0 + (live ? f : wv * 32);
    float* row = p.spec + rowi * (size_t)(N + 2);
    const float* arow = q.mag + rowi * (size_t)q.mag_ld;

    stft_contract(p.g.basis, N / 32, p.g.sg_lo, p.g.sg_hi, c_lo, c_hi, slab, abase, p.g.ps, lane, [&](int c, stft_f32x16 re, stft_f32x16 im) {
        float4 a4[4];
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) a4[rq] = *(const float4*)(arow + 32 * c + 8 * rq + 4 * hf);
        // ---- bin 0 is real and its im slot carried re[n_fft / 2], a (real) bin of its own: both keep their sign and take their magnitude
        const bool edge = c == 0 && hf == 0;
        float dc = 0.f, nyq = 0.f;
        if (edge) {
            dc = re[0] < 0.f ? -a4[0].x : a4[0].x;
            nyq = im[0] < 0.f ? -arow[N / 2] : arow[N / 2];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float a = r & 2 ? (r & 1 ? a4[r >> 2].w : a4[r >> 2].z) : (r & 1 ? a4[r >> 2].y : a4[r >> 2].x);
            const float m = __builtin_sqrtf(__builtin_fmaf(re[r], re[r], __fmul_rn(im[r], im[r])));
            const float s = a / m;
            const bool z = m == 0.f;
            re[r] = z ? a : __fmul_rn(re[r], s);
            im[r] = z ? 0.f : __fmul_rn(im[r], s);
        }
        if (edge) {
            re[0] = dc;
            im[0] = 0.f;
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

__global__ __launch_bounds__(GL_THREADS) void gl_target_kernel(const GlTargetParams p) {
    __shared__ float e[GL_TT][GL_MAX_MELS];
    const int tid = threadIdx.x, b = blockIdx.x / p.ntile, tile = blockIdx.x % p.ntile;
    int T = p.frames_in ? p.frames_in[b] : p.spec_cap;
    T = T < 0 ? 0 : (T > p.spec_cap ? p.spec_cap : T);
    if (tile == 0 && tid == 0) p.frames[b] = T;
    const int t0 = tile * GL_TT;
    if (t0 >= T) return;
    const int nt = T - t0 < GL_TT ? T - t0 : GL_TT;
    const size_t row0 = (size_t)b * p.spec_cap + t0;
    if (p.mel) {
        for (int i = tid; i < GL_TT * p.n_mels; i += GL_THREADS) {
            const int tt = i / p.n_mels, j = i - tt * p.n_mels;
            e[tt][j] = tt < nt ? exp10f(p.mel[(row0 + tt) * (size_t)p.n_mels + j]) : 0.f;
        }
        __syncthreads();
    }
    for (int k = tid; k < p.bins; k += GL_THREADS) {
        float a[GL_TT];
        if (p.mel) {
#pragma unroll
            for (int tt = 0; tt < GL_TT; ++tt) a[tt] = 0.f;
            for (int j = 0; j < p.n_mels; ++j) {   // one chain per output, ascending j
                const float w = p.pinv[(size_t)j * p.bins + k];
#pragma unroll
                for (int tt = 0; tt < GL_TT; ++tt) a[tt] = __builtin_fmaf(w, e[tt][j], a[tt]);
            }
#pragma unroll
            for (int tt = 0; tt < GL_TT; ++tt) a[tt] = a[tt] > 1e-10f ? a[tt] : 1e-10f;
        } else {
#pragma unroll
            for (int tt = 0; tt < GL_TT; ++tt) a[tt] = tt < nt ? __builtin_fabsf(p.mag[(row0 + tt) * (size_t)p.bins + k]) : 0.f;
        }
#pragma unroll
        for (int tt = 0; tt < GL_TT; ++tt)
            if (tt < nt) {
                const size_t at = (row0 + tt) * (size_t)p.bins + k;
                const float2 ph = p.init ? ((const float2*)p.init)[at] : make_float2(1.f, 0.f);
                p.A[(row0 + tt) * (size_t)p.a_ld + k] = a[tt];
                ((float2*)p.spec)[at] = make_float2(__fmul_rn(a[tt], ph.x), __fmul_rn(a[tt], ph.y));
            }
    }
}

static hipError_t gl_target_launch(const GlTargetParams& p, hipStream_t stream) {
    if (p.B < 1 || p.spec_cap < 1 || p.bins < 1 || p.a_ld < p.bins || !p.A || !p.spec || !p.frames || (!p.mag == !p.mel)) return hipErrorInvalidValue;
    if (p.mel && (!p.pinv || p.n_mels < 1 || p.n_mels > GL_MAX_MELS)) return hipErrorInvalidValue;
    if (p.ntile != (p.spec_cap + GL_TT - 1) / GL_TT || (long long)p.ntile * p.B > INT_MAX) return hipErrorInvalidValue;
    if (((uintptr_t)p.spec & 7) || ((uintptr_t)p.init & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gl_target_kernel, dim3((unsigned)(p.ntile * p.B)), dim3(GL_THREADS), 0, stream, p);
    return hipGetLastError();
}

static hipError_t gl_project_launch(const SpecFwdParams& p, const GlProjParams& q, int n_cu, hipStream_t stream) {
    if (!q.mag || ((uintptr_t)q.mag & 15) || (q.mag_ld & 3) || q.mag_ld < p.g.n_fft / 2 + 1 || q.tcap < 1 || q.tcap > p.spec_cap) return hipErrorInvalidValue;
    return spectral_forward_pick<gl_project_kernel<2>, gl_project_kernel<4>>(p, n_cu, stream, q);
}

// ---- dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM): 1 + 2 + 3 n_iter launches on the caller's stream; no host synchronisation unless the
// workspace grows
int griffin_lim(dtts_ctx* h, const dtts_griffinlim_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_GRIFFIN_LIM)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (int rc = blk.finalized(DTTS_PART_ISTFT)) return rc;
    const int N = h->is.n_fft, bins = N / 2 + 1;
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (a->spec_cap <= 0) return fail(h, DTTS_E_INVAL, "%s: spec_cap = %d rows", me, a->spec_cap);
    if (a->n_iter < 0) return fail(h, DTTS_E_INVAL, "%s: n_iter = %d", me, a->n_iter);
    if (a->hop < 1 || a->hop > N) return fail(h, DTTS_E_INVAL, "%s: hop = %d (supported: 1 .. n_fft = %d)", me, a->hop, N);
    if (!a->mag_dev == !a->mel_dev)
        return fail(h, DTTS_E_INVAL, "%s: mag_dev = %p and mel_dev = %p (exactly one of the two is given)", me, (const void*)a->mag_dev, (const void*)a->mel_dev);
    if (a->mel_dev) {
        if (!h->is_pinv) return fail(h, DTTS_E_STATE, "%s: mel_dev without the weight istft.inv_mel_basis in the finalised plan", me);
        if (a->n_mels != h->is_pinv_mels)
            return fail(h, DTTS_E_INVAL, "%s: n_mels = %d, istft.inv_mel_basis has %d columns", me, a->n_mels, h->is_pinv_mels);
    }
    const long long L = (long long)a->hop * (a->spec_cap - 1);   // samples of a full utterance
    if (L > INT_MAX || a->wav_ld < L) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples, spec_cap = %d rows at hop %d give %lld", me, a->wav_ld, a->spec_cap, a->hop, L);
    if (int e = check_wav_ld(h, me, (int)L, N)) return e;
    if (!a->out_dev && a->wav_ld > 0) return fail(h, DTTS_E_INVAL, "%s: null out_dev", me);
    if (int rc = blk.aligned(4, {{"mag_dev", a->mag_dev}, {"mel_dev", a->mel_dev}, {"frames_dev", a->frames_dev}, {"out_dev", a->out_dev},
                                 {"out_lens_dev", a->out_lens_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"init_dev", a->init_dev}, {"spec_out_dev", a->spec_out_dev}})) return rc;
    if (int e = check_envelope(h, me, a->hop)) return e;
    const int cap = a->spec_cap, Li = (int)L;
    const long long n_tiles_inv = (long long)a->B * ((cap + ISTFT_TILE - 1) / ISTFT_TILE);
    const long long n_chunks = (long long)a->B * std::max(1, (a->wav_ld + ISTFT_GATHER - 1) / ISTFT_GATHER);
    if (n_tiles_inv * (N / 64) > INT_MAX || n_chunks > INT_MAX || (long long)a->B * ((cap + GL_TT - 1) / GL_TT) > INT_MAX)
        return fail(h, DTTS_E_INVAL, "%s: B = %d utterances of spec_cap = %d rows, wav_ld = %d samples", me, a->B, cap, a->wav_ld);

    // ---- the workspace: A, the spectrum (unless the caller takes it), the windowed frames, the waveform between the iterations, the frame counts
    const int a_ld = N / 2 + 4;
    const size_t rows = (size_t)a->B * (size_t)cap;
    const size_t n_A = rows * (size_t)a_ld, n_spec = a->spec_out_dev ? 0 : rows * (size_t)(N + 2), n_fr = rows * (size_t)N;
    const size_t n_y = a->n_iter > 0 ? (size_t)a->B * (size_t)std::max(Li, 1) : 0;
    HIPCHK(h->a_spec.reserve((n_A + n_spec + n_fr + n_y + (size_t)a->B) * sizeof(float) + 5 * 256, stream));
    float* A = h->a_spec.alloc<float>(n_A);
    float* spec = a->spec_out_dev ? a->spec_out_dev : h->a_spec.alloc<float>(n_spec);
    float* fr = h->a_spec.alloc<float>(n_fr);
    float* y = n_y ? h->a_spec.alloc<float>(n_y) : nullptr;
    int* frames = h->a_spec.alloc<int>((size_t)a->B);
    if (!A || !spec || !fr || (n_y && !y) || !frames) return blk.workspace();

    GlTargetParams t{};
    t.mag = a->mag_dev;
    t.mel = a->mel_dev;
    t.pinv = h->is_pinv;
    t.init = a->init_dev;
    t.frames_in = a->frames_dev;
    t.A = A;
    t.spec = spec;
    t.frames = frames;
    t.B = a->B;
    t.spec_cap = cap;
    t.bins = bins;
    t.a_ld = a_ld;
    t.n_mels = a->mel_dev ? a->n_mels : 0;
    t.ntile = (cap + GL_TT - 1) / GL_TT;
    LAUNCH(gl_target_launch(t, stream));

    SpecInvParams iv{};
    iv.spec = spec;
    iv.frames = frames;
    iv.fr = fr;
    iv.wi = (const float4*)h->is_wi;
    iv.B = a->B;
    iv.spec_cap = cap;
    iv.tcap = cap;
    iv.n_fft = N;
    iv.ntile = (cap + ISTFT_TILE - 1) / ISTFT_TILE;
    SpecGatherParams mid{};   // an iteration's waveform: the workspace, hop (spec_cap - 1) samples a row
    mid.fr = fr;
    mid.frames = frames;
    mid.w2 = h->is_w2;
    mid.out = y;
    mid.B = a->B;
    mid.spec_cap = cap;
    mid.tcap = cap;
    mid.wav_ld = Li;
    mid.hop = a->hop;
    mid.n_fft = N;
    mid.nchunk = std::max(1, (Li + ISTFT_GATHER - 1) / ISTFT_GATHER);
    SpecGatherParams last = mid;   // the result: the caller's buffer and row pitch
    last.out = a->out_dev;
    last.out_lens = a->out_lens_dev;
    last.wav_ld = a->wav_ld;
    last.nchunk = std::max(1, (a->wav_ld + ISTFT_GATHER - 1) / ISTFT_GATHER);

    SpecFwdParams p{};
    GlProjParams q{A, a_ld, cap};
    if (a->n_iter > 0) {
        if (h->is_skew_hop != a->hop) {
            h->is_skew = melspec_skew_shift(a->hop);
            h->is_skew_hop = a->hop;
        }
        p.wav = y;
        p.frames = frames;
        p.spec = spec;
        p.g = stft_geom(h->is, a->hop, h->is_skew);
        p.B = a->B;
        p.wav_ld = Li;
        p.spec_cap = cap;
    }
    for (int i = 0; i <= a->n_iter; ++i) {
        if (i > 0) LAUNCH(gl_project_launch(p, q, h->n_cu, stream));
        LAUNCH(istft_frames_launch(iv, h->n_cu, stream));
        LAUNCH(istft_gather_launch(i == a->n_iter ? last : mid, stream));
    }
    return DTTS_OK;
}

} // namespace dtts
