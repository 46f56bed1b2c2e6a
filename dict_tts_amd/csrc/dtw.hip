// Dynamic time warping (dtw.h; dtts_text2mel_fetch(DTTS_OUT_DTW)).
//
// FORWARD (dtw_forward_kernel): one wave per pair, in a workgroup of its own, no barrier.  Lane t owns the DTW_LANE_ROWS = 16 rows
// row0 = 1024 strip + 16 t .. row0 + 15 of the current strip; their x values stay in registers.  At step k the lane walks its rows at
// column j = k - t: `up` is the cell it has just computed, `diag` and `left` are its own values of step k - 1.  The only cross-lane
// traffic per step is one shift by a lane (DPP wave_shr:1): lane t - 1's last-row value at column j (it handled that column one step
// earlier) and y_j, which lane 0 takes from a 64-value register chunk and every other lane inherits.  A longer x runs strip after strip
// in the same wave; the strip's last row goes through LDS (written by lane 63 at step j + 63, read by the whole wave 64 columns at a
// time at step j' <= j of the next strip: one wave, program order).  The sixteen 2-bit direction codes of a lane's column are one dword,
// stored as [strip][k][lane]: with the skewed index k, not j, the wave's store of a step is one coalesced line.
//
// The code is the TRACEBACK's argmin, not the forward min's: the first minimum of the unscaled (diag, up, left).
//
// PATH (dtw_path_kernel): one wave per pair follows the codes backwards.  The wave loads the codes of 64 columns of the current lane's
// rows at once and walks inside that window through v_readlane; lane 0 writes the pairs backwards from the end of the path rows, then the
// wave moves them to the front and fills the rest with -1.
//
// COST (dtw_cost_kernel, F > 1): the cityblock costs in fp64, in the order the wave consumes them, [strip][k][r][lane]; tiles of 8 (f32) or
// 4 (f64) lanes' rows by 64 skewed columns, both sides' rows in LDS.
#include "ctx.h"
#include "dtw.h"

namespace dtts {

// lane t <- lane t - 1 (lane 0 keeps its own value); every lane of the wave must be active
__device__ __forceinline__ int dtw_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }
__device__ __forceinline__ float dtw_shr1(float v) { return __int_as_float(dtw_shr1(__float_as_int(v))); }
__device__ __forceinline__ double dtw_shr1(double v) {
    return __hiloint2double(dtw_shr1(__double2hiint(v)), dtw_shr1(__double2loint(v)));
}
// the value of lane `l` (wave-uniform)
__device__ __forceinline__ float dtw_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double dtw_lane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// the pair's lengths; false = a bad pair (dist = NaN, path_len = 0)
__device__ __forceinline__ bool dtw_pair(const DtwParams& p, int b, int& N, int& M) {
    N = p.x_lens ? p.x_lens[b] : p.x_ld;
    M = p.y_lens ? p.y_lens[b] : p.y_ld;
    if (N < 1 || N > p.x_ld || M < 1 || M > p.y_ld) return false;
    return p.window < 0 || p.window >= (N > M ? N - M : M - N);
}

__device__ __forceinline__ double dtw_wave_sum(double v) {   // the same tree in every lane: a + b = b + a
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// mean, population sigma, skewness, Fisher kurtosis of v[0 .. n): two passes, per lane in index order, then the tree
template <class T>
__device__ void dtw_moments(const T* v, int n, double* out, int lane) {
    double s1 = 0.0;
    for (int i = lane; i < n; i += 64) s1 += (double)v[i];
    const double mean = dtw_wave_sum(s1) / (double)n;
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double d = (double)v[i] - mean, d2 = d * d;
        s2 += d2;
        s3 += d2 * d;
        s4 += d2 * d2;
    }
    const double m2 = dtw_wave_sum(s2) / (double)n, m3 = dtw_wave_sum(s3) / (double)n, m4 = dtw_wave_sum(s4) / (double)n;
    if (lane == 0) {
        out[0] = mean;
        out[1] = sqrt(m2);
        out[2] = m3 / (m2 * sqrt(m2));
        out[3] = m4 / (m2 * m2) - 3.0;
    }
}

template <int MODE> struct DtwIn { typedef float type; };
template <> struct DtwIn<DTW_COST_F64> { typedef double type; };

template <int MODE, bool SCALED, bool ACC>
__global__ __launch_bounds__(64) void dtw_forward_kernel(DtwParams p) {
    extern __shared__ __attribute__((aligned(16))) double dtw_lds[];
    typedef typename DtwIn<MODE>::type X;
    constexpr int R = DTW_LANE_ROWS;
    const int b = blockIdx.x, t = threadIdx.x;
    int N, M;
    if (!dtw_pair(p, b, N, M)) {
        if (t == 0) p.dist[b] = __builtin_nan("");
        if (p.moments && t < 8) p.moments[(size_t)b * 8 + t] = __builtin_nan("");
        return;
    }
    const X* xb = (const X*)p.x + (size_t)b * p.x_ld;   // (F = 1 in the modes that read them)
    const X* yb = (const X*)p.y + (size_t)b * p.y_ld;
    if (MODE != DTW_COST_WS && p.moments) {
        dtw_moments(xb, N, p.moments + (size_t)b * 8, t);
        dtw_moments(yb, M, p.moments + (size_t)b * 8 + 4, t);
    }
    const double INF = __builtin_inf();
    const double s = p.slope;
    const int w = p.window;
    const int nstrips = (N + DTW_STRIP_ROWS - 1) / DTW_STRIP_ROWS;
    unsigned* dirs = p.dirs ? p.dirs + (size_t)b * p.dir_stride : nullptr;
    const double* cost = MODE == DTW_COST_WS ? p.cost + (size_t)b * p.cost_stride : nullptr;
    double* acc = ACC ? p.acc + (size_t)b * p.x_ld * p.y_ld : nullptr;
    double left[R];

    for (int strip = 0; strip < nstrips; ++strip) {
        const int row0 = strip * DTW_STRIP_ROWS + t * R;
        const int rows = N - strip * DTW_STRIP_ROWS < DTW_STRIP_ROWS ? N - strip * DTW_STRIP_ROWS : DTW_STRIP_ROWS;
        const int last = (rows - 1) / R;      // the last lane that owns a row of this strip
        const int nsteps = M + last;
        const size_t kbase = (size_t)strip * (size_t)(M + 63);
        X xr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            xr[r] = (MODE != DTW_COST_WS && row0 + r < N) ? xb[row0 + r] : (X)0;
            left[r] = INF;                                        // column -1
        }
        double top_prev = (strip == 0 && t == 0) ? 0.0 : INF;     // D[row0 - 1][-1]
        double bottom = INF;                                      // this lane's last row at its latest column
        X ycur = 0, ychunk = 0;
        X ynext = (MODE != DTW_COST_WS && t < M) ? yb[t] : (X)0;  // the chunk after `ychunk`, loaded 64 steps ahead of its use
        double cchunk = INF;                                      // the previous strip's last row, 64 columns
        double cn[R];                                             // the costs of the next step
        if (MODE == DTW_COST_WS) {
#pragma unroll
            for (int r = 0; r < R; ++r) cn[r] = cost[(kbase * R + r) * 64 + t];
        }

        for (int k = 0; k < nsteps; ++k) {
            if ((k & 63) == 0) {
                if (MODE != DTW_COST_WS) {
                    ychunk = ynext;
                    ynext = k + 64 + t < M ? yb[k + 64 + t] : (X)0;
                }
                cchunk = (strip > 0 && k + t < M) ? dtw_lds[k + t] : INF;
            }
            double c[R];
            if (MODE == DTW_COST_WS) {
#pragma unroll
                for (int r = 0; r < R; ++r) c[r] = cn[r];
                if (k + 1 < nsteps) {
#pragma unroll
                    for (int r = 0; r < R; ++r) cn[r] = cost[((kbase + k + 1) * R + r) * 64 + t];
                }
            }
            double up_in = dtw_shr1(bottom);
            X yin = dtw_shr1(ycur);
            const double c0 = dtw_lane(cchunk, k & 63);
            const X y0 = dtw_lane(ychunk, k & 63);
            if (t == 0) {
                up_in = c0;
                yin = y0;
            }
            const int j = k - t;
            if (j >= 0 && j < M && t <= last) {
                ycur = yin;
                const int dj = j - row0;
                const int lo = w >= 0 ? dj - w : -(1 << 30), hi = w >= 0 ? dj + w : (1 << 30);   // row r is inside the band iff lo <= r <= hi
                double diag = top_prev, up = up_in;
                unsigned codes = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double lf = left[r];
                    double cc;
                    if (MODE == DTW_COST_F32) cc = (double)fabsf(xr[r] - yin);
                    else if (MODE == DTW_COST_F64) cc = fabs((double)xr[r] - (double)yin);
                    else cc = c[r];
                    const double sl = SCALED ? __dmul_rn(s, lf) : lf, su = SCALED ? __dmul_rn(s, up) : up;
                    double d = cc + fmin(diag, fmin(sl, su));
                    if (r < lo || r > hi) d = INF;
                    const unsigned code = (diag <= up && diag <= lf) ? 0u : (up <= lf ? 1u : 2u);   // _traceback's argmin: unscaled, first minimum
                    codes |= code << (2 * r);
                    if (ACC && row0 + r < N) acc[(size_t)(row0 + r) * p.y_ld + j] = d;
                    left[r] = d;
                    diag = lf;
                    up = d;
                }
                top_prev = up_in;
                bottom = up;
                if (dirs) dirs[(kbase + k) * 64 + t] = codes;
                if (t == 63 && strip + 1 < nstrips) dtw_lds[j] = bottom;
            }
        }
    }
    // every lane that owns rows has finished at column M - 1
    const int rl = (N - 1) - ((nstrips - 1) * DTW_STRIP_ROWS + t * R);
    if (rl >= 0 && rl < R) {
        double d = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r == rl) d = left[r];
        p.dist[b] = d;
    }
}

// One workgroup: LG lanes' rows (16 LG rows of x) against 64 values of the skewed column index k, i.e. 64 + LG - 1 rows of y; both staged
// in LDS at a row stride of F + 1 words (x rows in the order the threads take them).  A thread owns one x row and every NKQ-th k: its
// sums run over f ascending, one accumulator per cell.  Threads that are neighbours in `lane` store neighbouring words.
template <class T, int LG>
__global__ __launch_bounds__(256) void dtw_cost_kernel(DtwParams p) {
    extern __shared__ __attribute__((aligned(16))) double dtw_lds[];
    constexpr int XR = DTW_LANE_ROWS * LG, YR = 64 + LG - 1, NKQ = 256 / XR, NC = 64 / NKQ;
    const int b = blockIdx.x, strip = blockIdx.y / (64 / LG), lg = blockIdx.y % (64 / LG), k0 = blockIdx.z * 64;
    int N, M;
    if (!dtw_pair(p, b, N, M)) return;
    const int i0 = strip * DTW_STRIP_ROWS + lg * XR;
    if (i0 >= N || k0 >= M + 63) return;
    const int F = p.F, ldw = F + 1, tid = threadIdx.x;
    const int jlo = k0 - (lg * LG + LG - 1);
    T* xs = (T*)dtw_lds;
    T* ys = xs + XR * ldw;
    const T* xg = (const T*)p.x + (size_t)b * p.x_ld * F;
    const T* yg = (const T*)p.y + (size_t)b * p.y_ld * F;
    for (int idx = tid; idx < XR * F; idx += 256) {
        const int q = idx / F, f = idx - q * F;
        const int i = i0 + (q % LG) * DTW_LANE_ROWS + q / LG;      // slot q = r LG + lane offset
        xs[q * ldw + f] = i < N ? xg[(size_t)i * F + f] : (T)0;
    }
    for (int idx = tid; idx < YR * F; idx += 256) {
        const int q = idx / F, f = idx - q * F;
        const int j = jlo + q;
        ys[q * ldw + f] = (j >= 0 && j < M) ? yg[(size_t)j * F + f] : (T)0;
    }
    __syncthreads();
    const int q = tid % XR, kq = tid / XR;
    const int lo = q % LG, r = q / LG;
    const T* xr = xs + q * ldw;
    const T* yr = ys + (kq + LG - 1 - lo) * ldw;                   // the y row of this thread's first k; the next one is NKQ rows on
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (int f = 0; f < F; ++f) {
        const double xv = (double)xr[f];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += fabs(xv - (double)yr[c * NKQ * ldw + f]);
    }
    const int lane = lg * LG + lo, i = i0 + lo * DTW_LANE_ROWS + r;
    if (i >= N) return;
    double* out = p.cost_w + (size_t)b * p.cost_stride + (size_t)strip * (size_t)(M + 63) * DTW_LANE_ROWS * 64;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int k = k0 + kq + c * NKQ, j = k - lane;
        if (j >= 0 && j < M) out[((size_t)k * DTW_LANE_ROWS + r) * 64 + lane] = acc[c];
    }
}

__global__ __launch_bounds__(64) void dtw_path_kernel(DtwParams p) {
    const int b = blockIdx.x, t = threadIdx.x;
    int* P = p.path + (size_t)b * 2 * p.path_ld;
    int* Q = P + p.path_ld;
    int N, M;
    if (!dtw_pair(p, b, N, M)) {
        for (int n = t; n < p.path_ld; n += 64) P[n] = Q[n] = -1;
        if (t == 0) p.path_len[b] = 0;
        return;
    }
    const unsigned* dirs = p.dirs + (size_t)b * p.dir_stride;
    int i = N - 1, j = M - 1;
    int pos = p.path_ld - 1;          // path_ld >= x_ld + y_ld - 1 >= N + M - 1 (checked on the host): pos stays >= 0
    int moves = N + M - 2;            // the bound that does not depend on the data
    if (t == 0) {
        P[pos] = i;
        Q[pos] = j;
    }
    while ((i > 0 || j > 0) && moves > 0) {
        const int g = i / DTW_LANE_ROWS, strip = g >> 6, tl = g & 63, jhi = j;
        const int jj = jhi - t;       // this lane's column of the window
        const unsigned word = jj >= 0 ? dirs[((size_t)strip * (size_t)(M + 63) + jj + tl) * 64 + tl] : 0u;
        while ((i > 0 || j > 0) && moves > 0 && i / DTW_LANE_ROWS == g && jhi - j < 64) {
            const unsigned wv = (unsigned)__builtin_amdgcn_readlane((int)word, jhi - j);
            unsigned code = (wv >> (2 * (i % DTW_LANE_ROWS))) & 3u;
            if (i == 0) code = 2;         // row 0 is left only along j, column 0 only along i: each move decrements an index that is > 0
            else if (j == 0) code = 1;
            if (code == 0) {
                --i;
                --j;
            } else if (code == 1) {
                --i;
            } else {
                --j;
            }
            --pos;
            --moves;
            if (t == 0) {
                P[pos] = i;
                Q[pos] = j;
            }
        }
    }
    const int len = p.path_ld - pos;
    __threadfence();                  // lane 0's stores, read back by the whole wave
    if (pos > 0) {
        // chunk c moves [pos + 64 c, ..) to [64 c, ..): a destination never overlaps the source of a later chunk
        for (int n0 = 0; n0 < len; n0 += 64) {
            const int n = n0 + t;
            int a = 0, q = 0;
            if (n < len) {
                a = P[pos + n];
                q = Q[pos + n];
            }
            if (n < len) {
                P[n] = a;
                Q[n] = q;
            }
        }
        for (int n = len + t; n < p.path_ld; n += 64) P[n] = Q[n] = -1;
    }
    if (t == 0) p.path_len[b] = len;
}

template <class T, int LG>
static hipError_t dtw_cost_launch_t(const DtwParams& p, hipStream_t stream) {
    const size_t lds = (size_t)(DTW_LANE_ROWS * LG + 64 + LG - 1) * (p.F + 1) * sizeof(T);   // <= 135 KB at F = 128
    if (hipError_t e = hipFuncSetAttribute((const void*)dtw_cost_kernel<T, LG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)) return e;
    const dim3 grid((unsigned)p.B, (unsigned)(dtw_strips(p.x_ld) * (64 / LG)), (unsigned)((p.y_ld + 63 + 63) / 64));
    hipLaunchKernelGGL((dtw_cost_kernel<T, LG>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

hipError_t dtw_cost_launch(const DtwParams& p, int dtype, hipStream_t stream) {
    if (p.B < 1 || p.F < 2 || p.F > DTW_MAX_F || !p.cost_w) return hipErrorInvalidValue;
    return dtype == 0 ? dtw_cost_launch_t<float, 8>(p, stream) : dtw_cost_launch_t<double, 4>(p, stream);
}

template <int MODE, bool SCALED>
static hipError_t dtw_forward_launch_acc(const DtwParams& p, size_t lds, hipStream_t stream) {
    if (p.acc) hipLaunchKernelGGL((dtw_forward_kernel<MODE, SCALED, true>), dim3((unsigned)p.B), dim3(64), lds, stream, p);
    else hipLaunchKernelGGL((dtw_forward_kernel<MODE, SCALED, false>), dim3((unsigned)p.B), dim3(64), lds, stream, p);
    return hipGetLastError();
}

template <int MODE>
static hipError_t dtw_forward_launch_mode(const DtwParams& p, size_t lds, hipStream_t stream) {
    return p.slope != 1.0 ? dtw_forward_launch_acc<MODE, true>(p, lds, stream) : dtw_forward_launch_acc<MODE, false>(p, lds, stream);
}

hipError_t dtw_forward_launch(const DtwParams& p, int mode, hipStream_t stream) {
    if (p.B < 1 || p.x_ld < 1 || p.x_ld > DTW_MAX_LEN || p.y_ld < 1 || p.y_ld > DTW_MAX_LEN || p.window > DTW_MAX_LEN) return hipErrorInvalidValue;
    if (!(p.slope > 0.0) || (mode == DTW_COST_WS) != (p.cost != nullptr)) return hipErrorInvalidValue;
    const size_t lds = dtw_lds_bytes(p.x_ld, p.y_ld);   // <= 64 KB
    if (mode == DTW_COST_F32) return dtw_forward_launch_mode<DTW_COST_F32>(p, lds, stream);
    if (mode == DTW_COST_F64) return dtw_forward_launch_mode<DTW_COST_F64>(p, lds, stream);
    return dtw_forward_launch_mode<DTW_COST_WS>(p, lds, stream);
}

hipError_t dtw_path_launch(const DtwParams& p, hipStream_t stream) {
    if (p.B < 1 || !p.path || !p.path_len || !p.dirs || p.path_ld < p.x_ld + p.y_ld - 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_path_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// ---- dtts_text2mel_fetch(DTTS_OUT_DTW): up to three launches on the caller's stream; no host synchronisation unless the workspace grows.
// h may be null: the block is checked first, so that the refusals are reachable without a device
int dtw_forward(dtts_ctx* h, const dtts_dtw_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_DTW)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (a->F < 1 || a->F > DTW_MAX_F) return fail(h, DTTS_E_INVAL, "%s: F = %d (supported: 1 .. %d)", me, a->F, DTW_MAX_F);
    if (a->dtype != 0 && a->dtype != 1) return fail(h, DTTS_E_INVAL, "%s: dtype = %d (0 = f32, 1 = f64)", me, a->dtype);
    if (!std::isfinite(a->slope) || !(a->slope > 0.0)) return fail(h, DTTS_E_INVAL, "%s: slope = %g (must be finite and > 0)", me, a->slope);
    if (a->x_ld < 1 || a->x_ld > DTW_MAX_LEN) return fail(h, DTTS_E_INVAL, "%s: x_ld = %d rows (supported: 1 .. %d)", me, a->x_ld, DTW_MAX_LEN);
    if (a->y_ld < 1 || a->y_ld > DTW_MAX_LEN) return fail(h, DTTS_E_INVAL, "%s: y_ld = %d rows (supported: 1 .. %d)", me, a->y_ld, DTW_MAX_LEN);
    if (!a->x_dev || !a->y_dev || !a->dist_dev) return fail(h, DTTS_E_INVAL, "%s: null x_dev / y_dev / dist_dev", me);
    if (a->path_dev && !a->path_len_dev) return fail(h, DTTS_E_INVAL, "%s: path_dev without path_len_dev", me);
    if (a->path_dev && a->path_ld < a->x_ld + a->y_ld - 1)
        return fail(h, DTTS_E_INVAL, "%s: path_ld = %d entries for x_ld + y_ld - 1 = %d", me, a->path_ld, a->x_ld + a->y_ld - 1);
    if (a->moments_dev && a->F > 1) return fail(h, DTTS_E_INVAL, "%s: moments_dev with F = %d (the moments are those of 1-D tracks)", me, a->F);
    if (int rc = blk.aligned(a->dtype == 1 ? 8 : 4, {{"x_dev", a->x_dev}, {"y_dev", a->y_dev}})) return rc;
    if (int rc = blk.aligned(4, {{"x_lens_dev", a->x_lens_dev}, {"y_lens_dev", a->y_lens_dev}, {"path_dev", a->path_dev}, {"path_len_dev", a->path_len_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"dist_dev", a->dist_dev}, {"acc_dev", a->acc_dev}, {"moments_dev", a->moments_dev}})) return rc;
    if (int rc = blk.handle()) return rc;

    DtwParams p{};
    p.x = a->x_dev;
    p.y = a->y_dev;
    p.x_lens = a->x_lens_dev;
    p.y_lens = a->y_lens_dev;
    p.dist = a->dist_dev;
    p.path = a->path_dev;
    p.path_len = a->path_len_dev;
    p.acc = a->acc_dev;
    p.moments = a->moments_dev;
    p.slope = a->slope;
    p.B = a->B;
    p.F = a->F;
    p.x_ld = a->x_ld;
    p.y_ld = a->y_ld;
    p.window = a->window < 0 ? -1 : std::min(a->window, DTW_MAX_LEN);   // (|i - j| < DTW_MAX_LEN: a wider band is no band)
    p.path_ld = a->path_ld;
    const bool ws_cost = a->F > 1;
    const size_t dir_words = a->path_dev ? dtw_dir_words(a->x_ld, a->y_ld) : 0, cost_words = ws_cost ? dtw_cost_words(a->x_ld, a->y_ld) : 0;
    if (dir_words || cost_words) {
        HIPCHK(h->a_dtw.reserve(((size_t)a->B * dir_words * sizeof(unsigned) + 256) + ((size_t)a->B * cost_words * sizeof(double) + 256), stream));
        if (dir_words) {
            p.dirs = h->a_dtw.alloc<unsigned>((size_t)a->B * dir_words);
            if (!p.dirs) return blk.workspace();
        }
        if (cost_words) {
            p.cost_w = h->a_dtw.alloc<double>((size_t)a->B * cost_words);
            if (!p.cost_w) return blk.workspace();
            p.cost = p.cost_w;
        }
        p.dir_stride = dir_words;
        p.cost_stride = cost_words;
    }
    if (ws_cost) LAUNCH(dtw_cost_launch(p, a->dtype, stream));
    LAUNCH(dtw_forward_launch(p, ws_cost ? DTW_COST_WS : (a->dtype == 1 ? DTW_COST_F64 : DTW_COST_F32), stream));
    if (a->path_dev) LAUNCH(dtw_path_launch(p, stream));
    return DTTS_OK;
}

} // namespace dtts
