// BS.1770 integrated loudness and normalisation (loudness.h; dtts_text2mel_fetch(DTTS_OUT_LOUDNESS)).  All arithmetic is fp64 without
// contraction, except the one float32 product and the one float32 division of the normalisation.
//
// The K-weighting is two biquads in cascade: a linear recurrence s' = M s + g x on four state values, 10^5 .. 10^6 dependent steps for one
// utterance.  Every utterance is cut into segments of LOUD_SEG = 256 samples anchored at its sample 0, so that the cut (and with it every
// rounding) is the utterance's own, whatever batch it sits in:
//   ZERO  (loud_zero_kernel)   a lane per segment runs it from a zero state; leaves its end state e_k and max |x|.
//   CHAIN (loud_chain_kernel)  a wave per utterance: s_0 = 0, s_{k+1} = M^S s_k + e_k in segment order by lane 0, 64 segments at a time
//                              through LDS (the loads and stores of the states are the whole wave's); the lanes join the maxima.
//   SUM   (loud_sum_kernel)    a lane per segment runs it again from its true start state s_k, which makes y the sequential filter's up to
//                              the rounding of the carry; y^2 goes to each of the at most six blocks the segment meets, in sample order.
//   BLOCK (loud_block_kernel)  a lane per block adds the segments' shares in ascending segment order and divides by 0.4 rate.
//   GATE  (loud_gate_kernel)   a lane per utterance: the two gates, LUFS, gain, status.
//   APPLY (loud_apply_kernel)  elementwise (mode 1): (float)gain x, divided by the peak when that exceeds 1; zeros behind L.
// Why segments and a re-run, not a scan of 4 x 4 matrices: the scan would need the matrices' products per sample (16 values against 4),
// and its result would depend on the tree; here the only reassociation is the carry through M^S, once per 256 samples, and the re-run
// costs one more pass of a filter that is a dozen operations per sample.  No atomics anywhere; the sums have a fixed order.
#pragma clang fp contract(off)

#include "ctx.h"
#include "loudness.h"

namespace dtts {

namespace {

constexpr double LOUD_PI = 3.14159265358979323846;

__device__ __forceinline__ int loud_len(const LoudParams& p, int b) {
    const int L = p.lens ? p.lens[b] : p.wav_ld;
    return (L < 0 || L > p.wav_ld) ? 0 : L;
}

// The first block that reaches behind sample s0, i.e. the smallest j with hi_j > s0 (nb if none).  hi_j is within one sample of
// 0.1 rate j + 0.4 rate, so the estimate below starts at or before it and the walk is a few steps.  The blocks a segment [s0, s0 + 256)
// meets are then j .. with lo_j < s0 + 256: lo_j lies within one sample of 0.1 rate j, inside an interval of 0.4 rate + 258 samples, and
// 0.1 rate >= 800: at most 5 of them.
__device__ __forceinline__ int loud_first_block(const LoudParams& p, int s0, int nb) {
    int j = (int)floor((double)s0 / (0.1 * p.rate)) - 6;
    j = j > 0 ? j : 0;
    while (j < nb && p.bounds[j].y <= s0) ++j;
    return j;
}

} // namespace

__global__ __launch_bounds__(64) void loud_zero_kernel(LoudParams p) {
    const int b = blockIdx.y, seg = blockIdx.x * 64 + threadIdx.x;
    const int L = loud_len(p, b);
    const int s0 = seg * LOUD_SEG;
    if (seg >= p.nseg_ld || s0 >= L) return;
    const int s1 = s0 + LOUD_SEG < L ? s0 + LOUD_SEG : L;
    const float* x = p.wav + (size_t)b * p.wav_ld;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    float m = 0.f;
    for (int n = s0; n < s1; ++n) {
        const float v = x[n];
        m = fmaxf(m, fabsf(v));
        (void)loud_step(p.c, s, (double)v);
    }
    const size_t k = (size_t)b * p.nseg_ld + seg;
    double* e = p.seg_end + 4 * k;
    e[0] = s[0];
    e[1] = s[1];
    e[2] = s[2];
    e[3] = s[3];
    p.seg_max[k] = m;
}

__global__ __launch_bounds__(64) void loud_chain_kernel(LoudParams p) {
    __shared__ double ev[64][4], sv[64][4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int L = loud_len(p, b);
    const int nseg = (L + LOUD_SEG - 1) / LOUD_SEG;
    const size_t row = (size_t)b * p.nseg_ld;
    float m = 0.f;
    for (int k = t; k < nseg; k += 64) m = fmaxf(m, p.seg_max[row + k]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (t == 0) p.utt_max[b] = m;
    double s[4] = {0.0, 0.0, 0.0, 0.0};                 // (lane 0's)
    for (int k0 = 0; k0 < nseg; k0 += 64) {
        const int n = nseg - k0 < 64 ? nseg - k0 : 64;
        if (t < n) {
            const double* e = p.seg_end + 4 * (row + k0 + t);
            ev[t][0] = e[0];
            ev[t][1] = e[1];
            ev[t][2] = e[2];
            ev[t][3] = e[3];
        }
        __syncthreads();
        if (t == 0) {
            for (int k = 0; k < n; ++k) {
                sv[k][0] = s[0];
                sv[k][1] = s[1];
                sv[k][2] = s[2];
                sv[k][3] = s[3];
                double r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = (((p.ms[i][0] * s[0] + p.ms[i][1] * s[1]) + p.ms[i][2] * s[2]) + p.ms[i][3] * s[3]) + ev[k][i];
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = r[i];
            }
        }
        __syncthreads();
        if (t < n) {
            double* d = p.seg_start + 4 * (row + k0 + t);
            d[0] = sv[t][0];
            d[1] = sv[t][1];
            d[2] = sv[t][2];
            d[3] = sv[t][3];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void loud_sum_kernel(LoudParams p) {
    const int b = blockIdx.y, seg = blockIdx.x * 64 + threadIdx.x;
    const int L = loud_len(p, b);
    const int s0 = seg * LOUD_SEG;
    if (seg >= p.nseg_ld || s0 >= L) return;
    const int nb = loud_n_blocks(L, p.rate);
    const size_t k = (size_t)b * p.nseg_ld + seg;
    double* part = p.part + LOUD_SLOTS * k;
    if (nb == 0) return;                                // (nothing reads the shares of an utterance without a block)
    const int s1 = s0 + LOUD_SEG < L ? s0 + LOUD_SEG : L;
    const int jf = loud_first_block(p, s0, nb);
    int lo[LOUD_SLOTS], hi[LOUD_SLOTS];
    double acc[LOUD_SLOTS];
#pragma unroll
    for (int q = 0; q < LOUD_SLOTS; ++q) {
        const bool in = jf + q < nb;
        const int2 bd = in ? p.bounds[jf + q] : make_int2(0, 0);
        lo[q] = bd.x;
        hi[q] = bd.y;
        acc[q] = 0.0;
    }
    const float* x = p.wav + (size_t)b * p.wav_ld;
    const double* st = p.seg_start + 4 * k;
    double s[4] = {st[0], st[1], st[2], st[3]};
    for (int n = s0; n < s1; ++n) {
        const double y = loud_step(p.c, s, (double)x[n]);
        const double y2 = y * y;
#pragma unroll
        for (int q = 0; q < LOUD_SLOTS; ++q)
            if (n >= lo[q] && n < hi[q]) acc[q] += y2;
    }
#pragma unroll
    for (int q = 0; q < LOUD_SLOTS; ++q) part[q] = acc[q];
}

__global__ __launch_bounds__(64) void loud_block_kernel(LoudParams p) {
    const int b = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    const int L = loud_len(p, b);
    const int nb = loud_n_blocks(L, p.rate);
    if (j == 0) p.n_blocks[b] = nb < p.blocks_ld ? nb : p.blocks_ld;
    if (j >= nb || j >= p.blocks_ld) return;           // (blocks_ld >= the blocks of wav_ld samples is checked on the host)
    const int2 bd = p.bounds[j];
    const int lo = bd.x, hi = bd.y < L ? bd.y : L;
    double sum = 0.0;
    if (lo < hi) {
        const size_t row = (size_t)b * p.nseg_ld;
        for (int seg = lo / LOUD_SEG; seg <= (hi - 1) / LOUD_SEG; ++seg) {
            const int q = j - loud_first_block(p, seg * LOUD_SEG, nb);
            if (q >= 0 && q < LOUD_SLOTS) sum += p.part[LOUD_SLOTS * (row + seg) + q];   // (always)
        }
    }
    p.z[(size_t)b * p.blocks_ld + j] = sum / (0.4 * p.rate);
}

__global__ __launch_bounds__(64) void loud_gate_kernel(LoudParams p) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int L = loud_len(p, b);
    int nb = loud_n_blocks(L, p.rate);
    nb = nb < p.blocks_ld ? nb : p.blocks_ld;
    const double* z = p.z + (size_t)b * p.blocks_ld;
    int status = 0;
    double lufs = __builtin_nan(""), gain = 1.0;
    if (nb == 0) {
        status = DTTS_LOUD_TOO_SHORT;
    } else {
        double sum = 0.0;
        int cnt = 0;
        for (int j = 0; j < nb; ++j) {
            const double l = -0.691 + 10.0 * log10(z[j]);
            if (l >= -70.0) {
                sum += z[j];
                ++cnt;
            }
        }
        double sum2 = 0.0;
        int cnt2 = 0;
        if (cnt > 0) {
            const double gamma = -0.691 + 10.0 * log10(sum / (double)cnt) - 10.0;
            for (int j = 0; j < nb; ++j) {
                const double l = -0.691 + 10.0 * log10(z[j]);
                if (l > gamma && l > -70.0) {
                    sum2 += z[j];
                    ++cnt2;
                }
            }
        }
        if (cnt2 == 0) {
            status = DTTS_LOUD_SILENT;
            lufs = -__builtin_inf();
        } else {
            lufs = -0.691 + 10.0 * log10(sum2 / (double)cnt2);
            gain = pow(10.0, (p.target - lufs) / 20.0);
            if (p.mode == 1 && (float)gain * p.utt_max[b] > 1.f) status |= DTTS_LOUD_PEAK;
        }
    }
    p.lufs[b] = lufs;
    p.gain[b] = gain;
    p.status[b] = status;
}

__global__ __launch_bounds__(256) void loud_apply_kernel(LoudParams p) {
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= p.wav_ld) return;
    const int L = loud_len(p, b);
    float y = 0.f;
    if (n < L) {
        const float x = p.wav[(size_t)b * p.wav_ld + n];
        if (p.status[b] & (DTTS_LOUD_TOO_SHORT | DTTS_LOUD_SILENT)) {
            y = x;
        } else {
            const float g = (float)p.gain[b];
            const float pk = g * p.utt_max[b];          // = max |g x|: the product is monotone in |x|
            y = g * x;
            if (pk > 1.f) y = __fdiv_rn(y, pk);
        }
    }
    p.out[(size_t)b * p.wav_ld + n] = y;
}

// pyloudnorm's IIRfilter coefficients of the two K-weighting stages at `rate`, normalised by a0 (the host's libm, in this order)
LoudCoef loud_coefficients(double rate) {
    LoudCoef c;
    {
        const double G = 4.0, Q = 1.0 / std::sqrt(2.0), fc = 1500.0;
        const double A = std::pow(10.0, G / 40.0), w0 = 2.0 * LOUD_PI * (fc / rate), alpha = std::sin(w0) / (2.0 * Q), cw = std::cos(w0), r = std::sqrt(A);
        const double b0 = A * ((A + 1) + (A - 1) * cw + 2 * r * alpha), b1 = -2 * A * ((A - 1) + (A + 1) * cw), b2 = A * ((A + 1) + (A - 1) * cw - 2 * r * alpha);
        const double a0 = (A + 1) - (A - 1) * cw + 2 * r * alpha, a1 = 2 * ((A - 1) - (A + 1) * cw), a2 = (A + 1) - (A - 1) * cw - 2 * r * alpha;
        c.b0a = b0 / a0;
        c.b1a = b1 / a0;
        c.b2a = b2 / a0;
        c.a1a = a1 / a0;
        c.a2a = a2 / a0;
    }
    {
        const double Q = 0.5, fc = 38.0;
        const double w0 = 2.0 * LOUD_PI * (fc / rate), alpha = std::sin(w0) / (2.0 * Q), cw = std::cos(w0);
        const double b0 = (1 + cw) / 2, b1 = -(1 + cw), b2 = (1 + cw) / 2, a0 = 1 + alpha, a1 = -2 * cw, a2 = 1 - alpha;
        c.b0b = b0 / a0;
        c.b1b = b1 / a0;
        c.b2b = b2 / a0;
        c.a1b = a1 / a0;
        c.a2b = a2 / a0;
    }
    return c;
}

// M^S with S = LOUD_SEG = 2^8: M from the step itself (the images of the unit states at x = 0), then eight squarings
void loud_segment_matrix(const LoudCoef& c, double ms[4][4]) {
    static_assert(LOUD_SEG == 256, "eight squarings");
    double m[4][4];
    for (int j = 0; j < 4; ++j) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[j] = 1.0;
        (void)loud_step(c, s, 0.0);
        for (int i = 0; i < 4; ++i) m[i][j] = s[i];
    }
    for (int it = 0; it < 8; ++it) {
        double r[4][4];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double a = 0.0;
                for (int k = 0; k < 4; ++k) a += m[i][k] * m[k][j];
                r[i][j] = a;
            }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) m[i][j] = r[i][j];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) ms[i][j] = m[i][j];
}

hipError_t loud_launch(const LoudParams& p, hipStream_t stream) {
    if (p.B < 1 || p.B > 65535 || p.wav_ld < 1 || p.nseg_ld != (p.wav_ld + LOUD_SEG - 1) / LOUD_SEG || p.blocks_ld < 1 || !p.bounds || !p.seg_end ||
        !p.seg_start || !p.seg_max || !p.utt_max || !p.part || !p.z || !p.n_blocks || !p.lufs || !p.gain || !p.status || (p.mode == 1 && !p.out))
        return hipErrorInvalidValue;
    const dim3 segs((unsigned)((p.nseg_ld + 63) / 64), (unsigned)p.B);
    hipLaunchKernelGGL(loud_zero_kernel, segs, dim3(64), 0, stream, p);
    hipLaunchKernelGGL(loud_chain_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(loud_sum_kernel, segs, dim3(64), 0, stream, p);
    const int nb_max = loud_n_blocks(p.wav_ld, p.rate);
    hipLaunchKernelGGL(loud_block_kernel, dim3((unsigned)((std::max(nb_max, 1) + 63) / 64), (unsigned)p.B), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)((p.B + 63) / 64)), dim3(64), 0, stream, p);
    if (p.mode == 1) hipLaunchKernelGGL(loud_apply_kernel, dim3((unsigned)((p.wav_ld + 255) / 256), (unsigned)p.B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// ---- dtts_text2mel_fetch(DTTS_OUT_LOUDNESS): five or six launches on the caller's stream; no host synchronisation unless the workspace
// grows or a longer block table is uploaded.  h may be null: the block is checked first, so that the refusals are reachable without a device
int loudness_forward(dtts_ctx* h, const dtts_loudness_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_LOUDNESS)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B <= 0 || a->B > 65535) return fail(h, DTTS_E_INVAL, "%s: B = %d (supported: 1 .. 65535)", me, a->B);
    if (a->wav_ld < 1 || a->wav_ld > LOUD_MAX_WAV) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 1 .. %d)", me, a->wav_ld, LOUD_MAX_WAV);
    if (a->sample_rate < 8000 || a->sample_rate > 48000) return fail(h, DTTS_E_INVAL, "%s: sample_rate = %d (supported: 8000 .. 48000)", me, a->sample_rate);
    if (a->mode != 0 && a->mode != 1) return fail(h, DTTS_E_INVAL, "%s: mode = %d (0 = measure, 1 = measure and normalise)", me, a->mode);
    if (!std::isfinite(a->target_lufs)) return fail(h, DTTS_E_INVAL, "%s: target_lufs = %g (must be finite)", me, a->target_lufs);
    const double rate = (double)a->sample_rate;
    const int nb_max = loud_n_blocks(a->wav_ld, rate);
    if (a->blocks_ld < 1 || a->blocks_ld < nb_max)
        return fail(h, DTTS_E_INVAL, "%s: blocks_ld = %d blocks (must be >= 1; wav_ld = %d samples give %d)", me, a->blocks_ld, a->wav_ld, nb_max);
    if (!a->wav_dev || !a->lufs_dev || !a->gain_dev || !a->status_dev) return fail(h, DTTS_E_INVAL, "%s: null wav_dev / lufs_dev / gain_dev / status_dev", me);
    if (a->mode == 1 && !a->out_dev) return fail(h, DTTS_E_INVAL, "%s: null out_dev with mode = 1", me);
    if (int rc = blk.aligned(4, {{"wav_dev", a->wav_dev}, {"lens_dev", a->lens_dev}, {"status_dev", a->status_dev}, {"out_dev", a->out_dev},
                                 {"n_blocks_dev", a->n_blocks_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"lufs_dev", a->lufs_dev}, {"gain_dev", a->gain_dev}, {"z_dev", a->z_dev}})) return rc;
    if (int rc = blk.handle()) return rc;

    if (h->loud_bounds_rate != a->sample_rate || h->loud_bounds_n < nb_max) {   // numpy's truncations, made here: (int)(0.4 (j 0.25) rate), (int)(0.4 (j 0.25 + 1) rate)
        const int n = nb_max + nb_max / 2 + 64;
        std::vector<int2> bd((size_t)n);
        for (int j = 0; j < n; ++j) {
            bd[j].x = (int)(0.4 * ((double)j * 0.25) * rate);
            bd[j].y = (int)(0.4 * ((double)j * 0.25 + 1.0) * rate);
        }
        const int2* d = upload(h, bd);
        if (!d) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
        h->loud_bounds = d;
        h->loud_bounds_rate = a->sample_rate;
        h->loud_bounds_n = n;
    }
    LoudParams p{};
    p.wav = a->wav_dev;
    p.lens = a->lens_dev;
    p.bounds = h->loud_bounds;
    p.lufs = a->lufs_dev;
    p.gain = a->gain_dev;
    p.status = a->status_dev;
    p.out = a->mode == 1 ? a->out_dev : nullptr;
    p.c = loud_coefficients(rate);
    loud_segment_matrix(p.c, p.ms);
    p.rate = rate;
    p.target = a->target_lufs;
    p.B = a->B;
    p.wav_ld = a->wav_ld;
    p.blocks_ld = a->blocks_ld;
    p.nseg_ld = (a->wav_ld + LOUD_SEG - 1) / LOUD_SEG;
    p.mode = a->mode;
    const size_t segs = (size_t)a->B * p.nseg_ld, n_z = a->z_dev ? 0 : (size_t)a->B * a->blocks_ld, n_nb = a->n_blocks_dev ? 0 : (size_t)a->B;
    HIPCHK(h->a_loud.reserve(segs * (8 + LOUD_SLOTS) * sizeof(double) + segs * sizeof(float) + (size_t)a->B * sizeof(float) + n_z * sizeof(double) +
                                 n_nb * sizeof(int) + 8 * 256, stream));
    p.seg_end = h->a_loud.alloc<double>(4 * segs);
    p.seg_start = h->a_loud.alloc<double>(4 * segs);
    p.part = h->a_loud.alloc<double>(LOUD_SLOTS * segs);
    p.seg_max = h->a_loud.alloc<float>(segs);
    p.utt_max = h->a_loud.alloc<float>((size_t)a->B);
    p.z = a->z_dev ? a->z_dev : h->a_loud.alloc<double>(n_z);
    p.n_blocks = a->n_blocks_dev ? a->n_blocks_dev : h->a_loud.alloc<int>(n_nb);
    if (!p.seg_end || !p.seg_start || !p.part || !p.seg_max || !p.utt_max || !p.z || !p.n_blocks) return blk.workspace();
    LAUNCH(loud_launch(p, stream));
    return DTTS_OK;
}

} // namespace dtts
