// The acoustic model's validation losses (losses.h; dtts_text2mel_fetch(DTTS_OUT_LOSSES)).
//
// MEL (loss_mel_kernel): one workgroup per (utterance, tile of LOSS_TILE_ROWS frames).  Both images, bias added in fp64 and ZERO outside
// [0, T) x [0, n_mel), are staged with a 5-row / 5-bin halo as fp64 in LDS ((32 + 10) (n_mel + 10) 16 bytes: 59 KB at 80 bins, 91 KB at
// 128).  A thread takes the tile's pixels tid, tid + 256, ..; per pixel the five window moments are 121 fp64 taps each, rows then columns
// ascending, the window's fp64 values read through the scalar cache (the address is uniform); neighbouring lanes read neighbouring fp64
// words of a row, which no LDS bank shares.  The quotient is fp64.  A frame's weight is decided while staging (a target value != 0 marks
// its row); the weighted |d|, d^2 and 1 - ssim are summed per thread in pixel order, then over the threads by a fixed tree.
// loss_mel_reduce_kernel adds an utterance's tiles in index order.  No atomics.
//
// DURATION (loss_dur_kernel): one workgroup per utterance; the histogram of mel2word in LDS (integer atomics: order cannot change the
// counts), the terms in fp64 per word, summed per thread in word order and over the threads by the same tree.
#include "ctx.h"
#include "losses.h"

namespace dtts {

// the threads' K-tuples at red[tid * K + k] -> the sum over tid, in red[0 .. K): a tree whose shape depends on nothing but LOSS_THREADS
template <int K>
__device__ __forceinline__ void loss_tree(double* red, int tid) {
    for (int s = LOSS_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s)
            for (int k = 0; k < K; ++k) red[tid * K + k] += red[(tid + s) * K + k];
    }
    __syncthreads();
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_mel_kernel(LossMelParams p) {
    extern __shared__ __attribute__((aligned(16))) double loss_lds[];
    constexpr int R = LOSS_TILE_ROWS, HL = LOSS_HALO, K = LOSS_WIN;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.ntile, tile = blockIdx.x % p.ntile;
    const int r0 = tile * R;
    const int rows = p.T - r0 < R ? p.T - r0 : R;
    const int W = p.n_mel + 2 * HL, H = R + 2 * HL;
    double* X = loss_lds;
    double* Y = X + H * W;
    double* red = Y + H * W;
    int* flag = (int*)(red + 3 * LOSS_THREADS);
    const float* pb = p.pred + (size_t)b * p.pred_ld * p.n_mel;
    const float* tb = p.tgt + (size_t)b * p.tgt_ld * p.n_mel;
    const double bias = (double)p.bias;

    if (tid < R) flag[tid] = 0;
    __syncthreads();
    for (int idx = tid; idx < H * W; idx += LOSS_THREADS) {
        const int rr = idx / W, cc = idx - rr * W;
        const int gr = r0 - HL + rr, gc = cc - HL;
        double x = 0.0, y = 0.0;
        if (gr >= 0 && gr < p.T && gc >= 0 && gc < p.n_mel) {
            const float tv = tb[(size_t)gr * p.n_mel + gc];
            x = (double)pb[(size_t)gr * p.n_mel + gc] + bias;
            y = (double)tv + bias;
            if (tv != 0.0f && rr >= HL && rr < HL + rows) flag[rr - HL] = 1;   // (every writer stores the same word)
        }
        X[idx] = x;
        Y[idx] = y;
    }
    __syncthreads();

    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double a_l1 = 0.0, a_l2 = 0.0, a_ss = 0.0;
    for (int px = tid; px < rows * p.n_mel; px += LOSS_THREADS) {
        const int r = px / p.n_mel, c = px - r * p.n_mel;
        const double* xb = X + r * W + c;   // the window's first tap: staged row r = image row r0 + r - 5
        const double* yb = Y + r * W + c;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll 1   // (one window row = 22 SGPRs at a time; all eleven unrolled spill the scalar file)
        for (int i = 0; i < K; ++i) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double w = p.win[i * K + j];
                const double x = xb[i * W + j], y = yb[i * W + j];
                const double wx = w * x, wy = w * y;
                sx += wx;
                sy += wy;
                sxx = fma(wx, x, sxx);
                syy = fma(wy, y, syy);
                sxy = fma(wx, y, sxy);
            }
        }
        const double m11 = sx * sx, m22 = sy * sy, m12 = sx * sy;
        const double v = ((2.0 * m12 + C1) * (2.0 * (sxy - m12) + C2)) / ((m11 + m22 + C1) * ((sxx - m11) + (syy - m22) + C2));
        const size_t g = (size_t)(r0 + r) * p.n_mel + c;
        if (p.map) p.map[(size_t)b * p.T * p.n_mel + g] = (float)v;
        const double wgt = flag[r] ? 1.0 : 0.0;
        const double d = (double)pb[g] - (double)tb[g];
        a_l1 += wgt * fabs(d);
        a_l2 += wgt * (d * d);
        a_ss += wgt * (1.0 - v);
    }
    red[tid * 3 + 0] = a_l1;
    red[tid * 3 + 1] = a_l2;
    red[tid * 3 + 2] = a_ss;
    loss_tree<3>(red, tid);
    if (tid == 0) {
        int n = 0;
        for (int r = 0; r < rows; ++r) n += flag[r];
        double* out = p.part + ((size_t)b * p.ntile + tile) * 3;
        out[0] = red[0];
        out[1] = red[1];
        out[2] = red[2];
        p.pcount[(size_t)b * p.ntile + tile] = (long long)n * p.n_mel;
    }
}

__global__ __launch_bounds__(64) void loss_mel_reduce_kernel(LossMelReduceParams p) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    long long n = 0;
    for (int t = 0; t < p.ntile; ++t) {
        const double* q = p.part + ((size_t)b * p.ntile + t) * 3;
        s0 += q[0];
        s1 += q[1];
        s2 += q[2];
        n += p.pcount[(size_t)b * p.ntile + t];
    }
    p.sums[(size_t)b * 3 + 0] = s0;
    p.sums[(size_t)b * 3 + 1] = s1;
    p.sums[(size_t)b * 3 + 2] = s2;
    p.count[b] = n;
}

__global__ __launch_bounds__(LOSS_THREADS) void loss_dur_kernel(LossDurParams p) {
    extern __shared__ __attribute__((aligned(16))) double loss_lds[];
    const int tid = threadIdx.x, b = blockIdx.x;
    double* red = loss_lds;
    int* hist = (int*)(red + 5 * LOSS_THREADS);   // [T_w + 1]
    for (int w = tid; w <= p.T_w; w += LOSS_THREADS) hist[w] = 0;
    __syncthreads();
    const long long* m = p.m2w + (size_t)b * p.m2w_ld;
    for (int f = tid; f < p.T_mel; f += LOSS_THREADS) {
        const long long w = m[f];
        if (w >= 1 && w <= (long long)p.T_w) atomicAdd(&hist[(int)w], 1);   // 0 = padding; anything else outside 1 .. T_w is ignored
    }
    __syncthreads();
    const int wl = p.word_len[b];
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int w = tid + 1; w <= p.T_w; w += LOSS_THREADS) {
        const int d = hist[w];
        if (p.dur_gt) p.dur_gt[(size_t)b * p.T_w + (w - 1)] = d;
        const double n = w <= wl ? 1.0 : 0.0;
        const double dp = (double)p.dur_pred[(size_t)b * p.T_w + (w - 1)] * n;
        const double g = (p.log_scale ? log((double)d + 1.0) : (double)d) * n;
        const double dp2 = p.log_scale ? log(dp + 1.0) : dp;
        const double g2 = p.log_scale ? log(g + 1.0) : g;
        const double m2 = g2 > 0.0 ? 1.0 : 0.0;
        a[0] += n * fabs(dp - g);
        a[1] += n;
        a[2] += m2 * fabs(dp2 - g2);
        a[3] += m2;
        a[4] += dp2 - g2;   // (per word: the two sentence sums nearly cancel, their difference keeps its digits this way)
    }
    for (int k = 0; k < 5; ++k) red[tid * 5 + k] = a[k];
    loss_tree<5>(red, tid);
    if (tid == 0) {
        double* out = p.sums + (size_t)b * 5;
        out[0] = red[0];
        out[1] = red[1];
        out[2] = red[2];
        out[3] = red[3];
        out[4] = red[4];
    }
}

template <class Kern>
static hipError_t loss_lds_limit(Kern kern) {
    return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LOSS_LDS_BYTES);
}

hipError_t loss_mel_launch(const LossMelParams& p, hipStream_t stream) {
    if (p.B < 1 || p.T < 1 || p.n_mel < 1 || p.n_mel > LOSS_MAX_MEL || p.pred_ld < p.T || p.tgt_ld < p.T) return hipErrorInvalidValue;
    if (p.ntile != (p.T + LOSS_TILE_ROWS - 1) / LOSS_TILE_ROWS || (long long)p.ntile * p.B > INT_MAX) return hipErrorInvalidValue;
    const size_t lds = loss_mel_lds_bytes(p.n_mel);
    if (lds > (size_t)LOSS_LDS_BYTES) return hipErrorInvalidValue;
    if (hipError_t e = loss_lds_limit(loss_mel_kernel)) return e;
    hipLaunchKernelGGL(loss_mel_kernel, dim3((unsigned)(p.ntile * p.B)), dim3(LOSS_THREADS), lds, stream, p);
    return hipGetLastError();
}

hipError_t loss_mel_reduce_launch(const LossMelReduceParams& p, hipStream_t stream) {
    if (p.B < 1 || p.ntile < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_mel_reduce_kernel, dim3((unsigned)((p.B + 63) / 64)), dim3(64), 0, stream, p);
    return hipGetLastError();
}

hipError_t loss_dur_launch(const LossDurParams& p, hipStream_t stream) {
    if (p.B < 1 || p.T_w < 1 || p.T_w > DTTS_LOSS_MAX_WORDS || p.T_mel < 0 || p.m2w_ld < p.T_mel) return hipErrorInvalidValue;
    const size_t lds = loss_dur_lds_bytes(p.T_w);
    if (lds > (size_t)LOSS_LDS_BYTES) return hipErrorInvalidValue;
    if (hipError_t e = loss_lds_limit(loss_dur_kernel)) return e;
    hipLaunchKernelGGL(loss_dur_kernel, dim3((unsigned)p.B), dim3(LOSS_THREADS), lds, stream, p);
    return hipGetLastError();
}

// ---- dtts_text2mel_fetch(DTTS_OUT_LOSSES): two launches (mel) + one (durations) on the caller's stream; no host synchronisation unless the
// workspace of the tile sums grows
int losses_forward(dtts_ctx* h, const dtts_loss_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_LOSSES)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    const bool mel = a->mel_sums_dev != nullptr, dur = a->dur_sums_dev != nullptr;
    if (!mel && !dur) return fail(h, DTTS_E_INVAL, "%s: mel_sums_dev and dur_sums_dev are both NULL: no half requested", me);
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (int rc = blk.aligned(4, {{"pred_dev", a->pred_dev}, {"tgt_dev", a->tgt_dev}, {"ssim_map_dev", a->ssim_map_dev}, {"dur_pred_dev", a->dur_pred_dev},
                                 {"word_len_dev", a->word_len_dev}, {"dur_gt_dev", a->dur_gt_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"mel_sums_dev", a->mel_sums_dev}, {"mel_count_dev", a->mel_count_dev}, {"mel2word_dev", a->mel2word_dev},
                                 {"dur_sums_dev", a->dur_sums_dev}}))
        return rc;

    LossMelParams mp{};
    if (mel) {
        if (a->T <= 0) return fail(h, DTTS_E_INVAL, "%s: T = %d", me, a->T);
        if (a->n_mel < 1 || a->n_mel > LOSS_MAX_MEL) return fail(h, DTTS_E_INVAL, "%s: n_mel = %d (supported: 1 .. %d)", me, a->n_mel, LOSS_MAX_MEL);
        if (!std::isfinite(a->bias)) return fail(h, DTTS_E_INVAL, "%s: bias = %g", me, (double)a->bias);
        if (a->pred_ld != 0 && a->pred_ld < a->T) return fail(h, DTTS_E_INVAL, "%s: pred_ld = %d rows for T = %d", me, a->pred_ld, a->T);
        if (a->tgt_ld != 0 && a->tgt_ld < a->T) return fail(h, DTTS_E_INVAL, "%s: tgt_ld = %d rows for T = %d", me, a->tgt_ld, a->T);
        if (!a->pred_dev || !a->tgt_dev || !a->mel_count_dev) return fail(h, DTTS_E_INVAL, "%s: null pred_dev / tgt_dev / mel_count_dev", me);
        mp.ntile = (a->T + LOSS_TILE_ROWS - 1) / LOSS_TILE_ROWS;
        if ((long long)mp.ntile * a->B > INT_MAX) return fail(h, DTTS_E_INVAL, "%s: B = %d utterances of %d tiles", me, a->B, mp.ntile);
    }
    if (dur) {
        if (a->T_w < 1 || a->T_w > DTTS_LOSS_MAX_WORDS) return fail(h, DTTS_E_INVAL, "%s: T_w = %d (supported: 1 .. %d)", me, a->T_w, DTTS_LOSS_MAX_WORDS);
        if (a->T_mel < 0) return fail(h, DTTS_E_INVAL, "%s: T_mel = %d", me, a->T_mel);
        if (a->m2w_ld != 0 && a->m2w_ld < a->T_mel) return fail(h, DTTS_E_INVAL, "%s: m2w_ld = %d columns for T_mel = %d", me, a->m2w_ld, a->T_mel);
        if (a->dur_scale != 0 && a->dur_scale != 1) return fail(h, DTTS_E_INVAL, "%s: dur_scale = %d (0 = log, 1 = linear)", me, a->dur_scale);
        if (!a->dur_pred_dev || !a->word_len_dev || (!a->mel2word_dev && a->T_mel > 0))
            return fail(h, DTTS_E_INVAL, "%s: null dur_pred_dev / mel2word_dev / word_len_dev", me);
    }

    if (mel) {
        if (!h->loss_win) {
            std::vector<double> w(LOSS_WIN * LOSS_WIN);
            loss_window(w.data());
            h->loss_win = upload(h, w);
            if (!h->loss_win) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
        }
        const size_t n_part = (size_t)a->B * mp.ntile;
        HIPCHK(h->a_loss.reserve(n_part * 4 * sizeof(double) + 2 * 256, stream));
        mp.part = h->a_loss.alloc<double>(n_part * 3);
        mp.pcount = h->a_loss.alloc<long long>(n_part);
        if (!mp.part || !mp.pcount) return blk.workspace();
        mp.pred = a->pred_dev;
        mp.tgt = a->tgt_dev;
        mp.win = h->loss_win;
        mp.map = a->ssim_map_dev;
        mp.B = a->B;
        mp.T = a->T;
        mp.n_mel = a->n_mel;
        mp.pred_ld = a->pred_ld ? a->pred_ld : a->T;
        mp.tgt_ld = a->tgt_ld ? a->tgt_ld : a->T;
        mp.bias = a->bias;
        LAUNCH(loss_mel_launch(mp, stream));
        LossMelReduceParams rp{mp.part, mp.pcount, a->mel_sums_dev, (long long*)a->mel_count_dev, a->B, mp.ntile};
        LAUNCH(loss_mel_reduce_launch(rp, stream));
    }
    if (dur) {
        LossDurParams dp{a->dur_pred_dev, (const long long*)a->mel2word_dev, a->word_len_dev, a->dur_sums_dev, a->dur_gt_dev, a->B, a->T_w, a->T_mel,
                         a->m2w_ld ? a->m2w_ld : a->T_mel, a->dur_scale == 0 ? 1 : 0};
        LAUNCH(loss_dur_launch(dp, stream));
    }
    return DTTS_OK;
}

} // namespace dtts
