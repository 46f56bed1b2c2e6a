// F0 extraction by Boersma's autocorrelation method (pitch.h; dtts_text2mel_fetch(DTTS_OUT_PITCH)).  All arithmetic is fp64.
//
// STATS (pitch_stats_kernel): one workgroup per utterance; the global mean (thread t adds samples t, t + 1024, .. in index order, then a
// fixed tree) and the global peak max |x - mean|; writes n_frames.
//
// ACF (pitch_acf_kernel), the hot path: one workgroup per frame.  The frame is staged once in LDS as doubles, zero-padded behind nsw so
// that every lag sums over the same j = 0 .. nsw - 1 (the padded products add exact zeros).  Every wave derives the local mean and peak
// itself (lane-strided in index order, then the xor butterfly: the same value in every lane of every wave), the frame is windowed in
// place, and then lane t owns the PITCH_LAGS = 7 consecutive lags 7 t .. 7 t + 6: per block of PITCH_JBLOCK = 8 values of j it reads the 8
// f[j] (one address for the whole wave: a broadcast) and the 14 values f[j + 7 t ..] its lags meet them with, 22 LDS doubles for 56
// v_fma_f64, each lag's sum running over j ascending in one accumulator.  Seven doubles between neighbouring lanes is an odd number of
// 8-byte words: the 32 lanes of a ds_read_b64 group fall on 32 distinct bank pairs.
//
// CANDIDATES (pitch_candidates_kernel): one wave per frame, r in LDS.  The lanes test 64 lags at a time, the ballot's bits are taken in
// ascending order; the <= 140 terms of a sinc interpolation are split over the lanes (sin(pi (x - i)) is +- sin(pi frac(x)): one sinpi per
// evaluation, one cos per term for the Hanning taper) and joined by the xor butterfly, so every lane holds the same sum and the search
// runs in uniform control flow.  A slot's maximiser is where the interpolant's ANALYTIC derivative changes sign (pitch_maximise).
//
// PATH (pitch_path_kernel): one wave per utterance, no atomics.  Lane 4 c2 + q takes the predecessors c1 = q, q + 4, .. of slot c2 in
// ascending order with a strict >, two xor steps join the four lanes (larger value, then smaller slot); the backpointers go to the
// workspace as one 16-byte row per frame and are followed backwards 64 frames at a time through LDS.  The candidates come in 64 frames
// at a time too, and inside such a block the wave orders its LDS traffic without a barrier (pitch_wave_sync).
#include "ctx.h"
#include "pitch.h"

namespace dtts {

namespace {

constexpr double PITCH_PI = 3.14159265358979323846;
constexpr int PITCH_STATS_THREADS = 1024;   // FIXED: the order of the global mean's sum

__device__ __forceinline__ double pitch_wave_sum(double v) {   // the same tree in every lane: a + b = b + a
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double pitch_wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// Orders the LDS traffic of a workgroup that is ONE wave: the hardware retires a wave's LDS operations in order, so only the compiler has to
// keep them so.  Unlike __syncthreads it waits for no outstanding global store.
__device__ __forceinline__ void pitch_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the utterance's length and frame count; nF = 0 for a bad one
__device__ __forceinline__ int pitch_utt(const PitchParams& p, int b, int& L) {
    L = p.lens ? p.lens[b] : p.wav_ld;
    if (L < 1 || L > p.wav_ld) return 0;
    const int nF = pitch_frames(L, p.g.first, p.hop);
    return nF < p.frames_ld ? nF : p.frames_ld;   // (frames_ld >= the frames of wav_ld samples is checked on the host)
}

} // namespace

__global__ __launch_bounds__(PITCH_STATS_THREADS) void pitch_stats_kernel(PitchParams p) {
    __shared__ double red[PITCH_STATS_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    int L;
    const int nF = pitch_utt(p, b, L);
    if (t == 0) p.n_frames[b] = nF;
    if (nF == 0) {
        if (t == 0) p.gpeak[b] = 0.0;
        return;
    }
    const float* x = p.wav + (size_t)b * p.wav_ld;
    double s = 0.0;
    for (int i = t; i < L; i += PITCH_STATS_THREADS) s += (double)x[i];
    red[t] = s;
    __syncthreads();
    for (int w = PITCH_STATS_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double mean = red[0] / (double)L;
    __syncthreads();
    double m = 0.0;
    for (int i = t; i < L; i += PITCH_STATS_THREADS) m = fmax(m, fabs((double)x[i] - mean));
    red[t] = m;
    __syncthreads();
    for (int w = PITCH_STATS_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = fmax(red[t], red[t + w]);
        __syncthreads();
    }
    if (t == 0) p.gpeak[b] = red[0];
}

// LDS doubles of one frame: the frame, padded to whole j blocks, and the zeros the highest lane's window runs into
inline int pitch_acf_threads(int n_lag) { return ((n_lag + PITCH_LAGS - 1) / PITCH_LAGS + 63) / 64 * 64; }
inline int pitch_acf_lds(int nsw, int threads) { return (nsw + PITCH_JBLOCK - 1) / PITCH_JBLOCK * PITCH_JBLOCK + PITCH_LAGS * threads + PITCH_LAGS; }

__global__ __launch_bounds__(256) void pitch_acf_kernel(PitchParams p, int lds_n) {
    extern __shared__ __attribute__((aligned(16))) double pitch_lds[];
    constexpr int K = PITCH_LAGS, J = PITCH_JBLOCK;
    const int k = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, nt = blockDim.x;
    int L;
    const int nF = pitch_utt(p, b, L);
    if (k >= nF) return;
    const PitchGeometry& g = p.g;
    const int left = (L - nF * p.hop + p.hop - 1 + 2 * k * p.hop) / 2, right = left + 1;   // floor(c_k): 2 c_k is a non-negative integer
    const int s0 = right - g.half;                                                        // the sample of j = 0
    const float* x = p.wav + (size_t)b * p.wav_ld;
    double* fr = pitch_lds;
    for (int j = t; j < lds_n; j += nt) {
        const int i = s0 + j;
        fr[j] = (j < g.nsw && i >= 0 && i < L) ? (double)x[i] : 0.0;
    }
    __syncthreads();
    // the local mean over x[max(0, right - nper) .. min(L - 1, left + nper)], inside the frame since nper < half
    int jlo = (right - g.nper > 0 ? right - g.nper : 0) - s0, jhi = (left + g.nper < L - 1 ? left + g.nper : L - 1) - s0;
    jlo = jlo > 0 ? jlo : 0;
    jhi = jhi < g.nsw - 1 ? jhi : g.nsw - 1;
    double s = 0.0;
    for (int j = jlo + lane; j <= jhi; j += 64) s += fr[j];
    const double mean = pitch_wave_sum(s) / (double)(jhi - jlo + 1);
    const int plo = g.half - g.halfper > 0 ? g.half - g.halfper : 0, phi = g.half + g.halfper < g.nsw ? g.half + g.halfper : g.nsw;
    double m = 0.0;
    for (int j = plo + lane; j < phi; j += 64) m = fmax(m, fabs(fr[j] - mean));
    const double peak = pitch_wave_max(m);
    const size_t frame = (size_t)b * p.frames_ld + k;
    double* r = p.acf + frame * g.n_lag;
    const double gp = p.gpeak[b];
    if (t == 0) p.intensity[frame] = peak == 0.0 ? 0.0 : (peak > gp ? 1.0 : peak / gp);
    __syncthreads();                                   // every wave has read the raw frame
    for (int j = t; j < g.nsw; j += nt) fr[j] = (fr[j] - mean) * p.win[j];
    __syncthreads();

    // The lane's 14 window values are read by explicit ds_read_b64 (2 LDS cycles each, conflict-free at the odd stride): the compiler
    // would pair them into ds_read2_b64, which takes 16 cycles a pair and makes the loop LDS-bound.  The s_waitcnt that follows names the
    // values as operands, so nothing uses them before it.
    static_assert(K == 7 && J == 8, "the window reads below are written out for 14 values");
    const unsigned fw = (unsigned)(size_t)(__attribute__((address_space(3))) double*)(fr + K * t);
    double acc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) acc[q] = 0.0;
    const int nswj = (g.nsw + J - 1) / J * J;
    for (int j0 = 0; j0 < nswj; j0 += J) {
        double a[J], w[J + K - 1];
#pragma unroll
        for (int i = 0; i < J; ++i) a[i] = fr[j0 + i];
        const unsigned wa = fw + 8u * (unsigned)j0;
#define PITCH_WREAD(i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(w[i]) : "v"(wa), "n"(8 * (i)))
        PITCH_WREAD(0); PITCH_WREAD(1); PITCH_WREAD(2); PITCH_WREAD(3); PITCH_WREAD(4); PITCH_WREAD(5); PITCH_WREAD(6);
        PITCH_WREAD(7); PITCH_WREAD(8); PITCH_WREAD(9); PITCH_WREAD(10); PITCH_WREAD(11); PITCH_WREAD(12); PITCH_WREAD(13);
#undef PITCH_WREAD
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]), "+v"(w[9]),
                       "+v"(w[10]), "+v"(w[11]), "+v"(w[12]), "+v"(w[13]));
#pragma unroll
        for (int i = 0; i < J; ++i) {
#pragma unroll
            for (int q = 0; q < K; ++q) acc[q] = fma(a[i], w[i + q], acc[q]);
        }
    }
    __syncthreads();                                   // the frame is no longer read
    if (t == 0) fr[0] = acc[0];
    __syncthreads();
    const double ac0 = fr[0];
    const bool flat = peak == 0.0 || !(ac0 > 0.0);     // only the unvoiced candidate
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const int l = K * t + q;
        if (l < g.n_lag) r[l] = l == 0 ? 1.0 : (flat ? 0.0 : acc[q] / (ac0 * p.wr[l]));
    }
}

namespace {

// Praat's NUM_interpolate_sinc of depth D at the lag x >= 0, on r[0 .. brent] taken symmetrically; the same value in every lane
__device__ double pitch_sinc(const double* r, int brent, double x, int D, int lane) {
    const double fl = floor(x);
    const int ml = (int)fl;
    if (x == fl) return r[ml < 0 ? -ml : ml];
    const int dl = ml + brent + 1, dr = brent - ml;    // the samples on either side
    D = D < dl ? D : dl;
    D = D < dr ? D : dr;
    const double fx = x - fl, sp = sinpi(fx);
    const double wl = fx + (double)D, wrr = (double)D - fx + 1.0;   // x - (mr - D) + 1, (ml + D) - x + 1
    double sum = 0.0;
    for (int m = lane; m < 2 * D; m += 64) {
        const bool lf = m < D;
        const int n = lf ? m : m - D;
        const int i = lf ? ml - n : ml + 1 + n;
        const double phi = PITCH_PI * (lf ? fx + (double)n : 1.0 - fx + (double)n);
        const double sn = (n & 1) ? -sp : sp;
        sum += r[i < 0 ? -i : i] * sn / phi * (0.5 + 0.5 * cos(phi / (lf ? wl : wrr)));
    }
    return pitch_wave_sum(sum);
}

// d sincD / dx at a non-integer lag x (between two integers the term set is fixed); the same value in every lane
__device__ double pitch_dsinc(const double* r, int brent, double x, int D, int lane) {
    const double fl = floor(x);
    const int ml = (int)fl;
    const int dl = ml + brent + 1, dr = brent - ml;
    D = D < dl ? D : dl;
    D = D < dr ? D : dr;
    const double fx = x - fl, sp = sinpi(fx), cp = cospi(fx);
    const double wl = fx + (double)D, wrr = (double)D - fx + 1.0;
    double sum = 0.0;
    for (int m = lane; m < 2 * D; m += 64) {
        const bool lf = m < D;
        const int n = lf ? m : m - D;
        const int i = lf ? ml - n : ml + 1 + n;
        const double sg = lf ? 1.0 : -1.0, W = lf ? wl : wrr;
        const double phi = PITCH_PI * (lf ? fx + (double)n : 1.0 - fx + (double)n);
        const double sn = (n & 1) ? -sp : sp;                       // sin(phi)
        const double cn = ((n & 1) != 0) == lf ? -cp : cp;          // cos(phi): cos(pi (1 - fx)) = -cos(pi fx)
        const double S = sn / phi, dS = sg * PITCH_PI * (cn * phi - sn) / (phi * phi);
        double st, ct;
        sincos(phi / W, &st, &ct);
        const double H = 0.5 + 0.5 * ct, dH = -0.5 * st * sg * (PITCH_PI * W - phi) / (W * W);
        sum += r[i < 0 ? -i : i] * (dS * H + S * dH);
    }
    return pitch_wave_sum(sum);
}

// The maximiser of sincD near the integer lag l, inside [l - 1, l + 1]: where the derivative changes sign from + to -, a zero inside a cell or
// a kink on an integer lag (the term set changes there).  Bracketed around the parabolic vertex, closed in on by the Illinois regula falsi
// to 1e-12; the derivative defines a flat maximum far better than function values do (those to sqrt(2 eps / curvature), about 1e-6).
__device__ double pitch_maximise(const double* r, int brent, int l, int D, int lane) {
    const double eps = 0x1p-30;
    auto d = [&](double x) { return pitch_dsinc(r, brent, x == floor(x) ? x + 0x1p-40 : x, D, lane); };
    const double r0 = r[l - 1], r1 = r[l], r2 = r[l + 1];
    const double xv = (double)l + 0.5 * (r2 - r0) / (2.0 * r1 - r0 - r2);
    double a = fmax(xv - 0.5, (double)(l - 1) + eps), b = fmin(xv + 0.5, (double)(l + 1) - eps);
    double fa = d(a), fb = d(b);
    if (!(fa > 0.0)) {
        a = (double)(l - 1) + eps;
        fa = d(a);
        if (!(fa > 0.0)) return a;
    }
    if (!(fb < 0.0)) {
        b = (double)(l + 1) - eps;
        fb = d(b);
        if (!(fb < 0.0)) return b;
    }
    for (int it = 0; it < 80 && b - a > 1e-12; ++it) {
        double xm = b - fb * (b - a) / (fb - fa);
        if (!(a < xm && xm < b)) xm = 0.5 * (a + b);
        const double fm = d(xm);
        if (fm > 0.0) {
            a = xm;
            fa = fm;
            fb *= 0.5;
        } else if (fm < 0.0) {
            b = xm;
            fb = fm;
            fa *= 0.5;
        } else {
            return xm;
        }
    }
    return 0.5 * (a + b);
}

__device__ __forceinline__ double pitch_vertex(const double* r, int l) {
    const double r0 = r[l - 1], r1 = r[l], r2 = r[l + 1];
    return (double)l + 0.5 * (r2 - r0) / (2.0 * r1 - r0 - r2);
}

} // namespace

__global__ __launch_bounds__(64) void pitch_candidates_kernel(PitchParams p) {
    extern __shared__ __attribute__((aligned(16))) double pitch_lds[];
    __shared__ double cf[16], cs[16];
    __shared__ int cl[16];
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    int L;
    const int nF = pitch_utt(p, b, L);
    if (k >= nF) return;
    const PitchGeometry& g = p.g;
    const size_t frame = (size_t)b * p.frames_ld + k;
    const double* rg = p.acf + frame * g.n_lag;
    double* r = pitch_lds;
    for (int l = lane; l < g.n_lag; l += 64) r[l] = rg[l];
    if (lane < 16) {
        cf[lane] = 0.0;
        cs[lane] = 0.0;
        cl[lane] = 0;
    }
    __syncthreads();
    int n = 1;                                          // slot 0: the unvoiced candidate
    const int lmax = (g.maxlag < g.brent ? g.maxlag : g.brent) - 1;
    const double half_vt = 0.5 * p.vt;
    for (int base = 2; base <= lmax; base += 64) {
        const int l = base + lane;
        const bool is_max = l <= lmax && r[l] > half_vt && r[l] > r[l - 1] && r[l] >= r[l + 1];
        unsigned long long mask = __ballot(is_max);
        while (mask) {                                  // wave-uniform: the maxima in ascending lag
            const int lm = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double x0 = pitch_vertex(r, lm);
            double st = pitch_sinc(r, g.brent, x0, 30, lane);
            if (st > 1.0) st = 1.0 / st;
            const double f = p.sr / x0;
            int place = -1;
            if (n < PITCH_CAND) {
                place = n++;
            } else {
                double weakest = 0.0;
                for (int i = 1; i < PITCH_CAND; ++i) {
                    const double v = cs[i] - p.oc * log2(p.floor_hz / cf[i]);
                    if (place < 0 || v < weakest) {
                        weakest = v;
                        place = i;
                    }
                }
                if (!(st - p.oc * log2(p.floor_hz / f) > weakest)) place = -1;
            }
            if (place >= 0 && lane == 0) {
                cf[place] = f;
                cs[place] = st;
                cl[place] = lm;
            }
            __syncthreads();
        }
    }
    for (int i = 1; i < n; ++i) {
        const double x = pitch_maximise(r, g.brent, cl[i], 70, lane);
        double st = pitch_sinc(r, g.brent, x, 70, lane);
        if (st > 1.0) st = 1.0 / st;
        __syncthreads();
        if (lane == 0) {
            cf[i] = p.sr / x;
            cs[i] = st;
        }
        __syncthreads();
    }
    if (lane < PITCH_CAND) {
        double* c = p.cand + frame * (2 * PITCH_CAND) + 2 * lane;
        c[0] = lane < n ? cf[lane] : 0.0;
        c[1] = lane < n ? cs[lane] : 0.0;
    }
    if (lane == 0) p.n_cand[frame] = n;
}

__global__ __launch_bounds__(64) void pitch_path_kernel(PitchParams p) {
    __shared__ double dl[2][16], fq[2][16], lf[2][16], loc[16], ccand[64][2 * PITCH_CAND], cint[64];
    __shared__ int cnc[64];
    __shared__ __attribute__((aligned(16))) unsigned char rows[64][PITCH_PSI];
    __shared__ int sel[64];
    const int b = blockIdx.x, t = threadIdx.x;
    int L;
    const int nF = pitch_utt(p, b, L);
    const size_t row = (size_t)b * p.frames_ld;
    double* f0 = p.f0 + row;
    int* selected = p.selected ? p.selected + row : nullptr;
    for (int k = nF + t; k < p.frames_ld; k += 64) {
        f0[k] = 0.0;
        if (selected) selected[k] = -1;
    }
    if (nF == 0) return;
    const double* cand = p.cand + row * (2 * PITCH_CAND);
    const int* n_cand = p.n_cand + row;
    const double* inten = p.intensity + row;
    unsigned char* psi = p.psi + row * PITCH_PSI;
    const double NINF = -__builtin_inf(), log2_ceiling = log2(p.ceiling);
    const int c2 = t >> 2, q = t & 3;
    auto clampn = [](int n) { return n < 1 ? 1 : (n > PITCH_CAND ? PITCH_CAND : n); };

    // 64 frames' candidates at a time go to LDS in one coalesced sweep, so that the frame-by-frame chain below waits for no global load
    int nc_prev = 0;
    for (int k0 = 0; k0 < nF; k0 += 64) {
        const int n = nF - k0 < 64 ? nF - k0 : 64;
        for (int i = t; i < n * 2 * PITCH_CAND; i += 64) (&ccand[0][0])[i] = cand[(size_t)k0 * (2 * PITCH_CAND) + i];
        if (t < n) {
            cint[t] = inten[k0 + t];
            cnc[t] = clampn(n_cand[k0 + t]);
        }
        __syncthreads();
        for (int kk = 0; kk < n; ++kk) {
            const int k = k0 + kk, nc = cnc[kk], cur = k & 1;
            if (t < 16) {
                const double f = t < PITCH_CAND ? ccand[kk][2 * t] : 0.0, s = t < PITCH_CAND ? ccand[kk][2 * t + 1] : 0.0, in = cint[kk];
                const bool voiced = t < nc && f > 0.0 && f < p.ceiling;
                const double unv = p.vt + fmax(0.0, 2.0 - in * (1.0 + p.vt) / p.st);
                const double l2 = voiced ? log2(f) : 0.0;                       // one logarithm per slot and frame: log2(a / b) = log2 a - log2 b
                fq[cur][t] = voiced ? f : 0.0;                                  // 0: unvoiced
                lf[cur][t] = l2;
                loc[t] = voiced ? s - p.oc * (log2_ceiling - l2) : unv;
            }
            pitch_wave_sync();
            if (k == 0) {
                if (t < 16) dl[cur][t] = t < nc ? loc[t] : NINF;
            } else {
                const double f2 = fq[cur][c2], l2 = lf[cur][c2];
                double best = NINF;
                int bi = 99;
                for (int c1 = q; c1 < nc_prev; c1 += 4) {
                    const double f1 = fq[cur ^ 1][c1];
                    const double cost = (f1 == 0.0) != (f2 == 0.0) ? p.vu : (f1 == 0.0 ? 0.0 : p.oj * fabs(lf[cur ^ 1][c1] - l2));
                    const double v = dl[cur ^ 1][c1] - cost;
                    if (v > best) {
                        best = v;
                        bi = c1;
                    }
                }
#pragma unroll
                for (int off = 1; off <= 2; off <<= 1) {
                    const double ov = __shfl_xor(best, off, 64);
                    const int oi = __shfl_xor(bi, off, 64);
                    if (ov > best || (ov == best && oi < bi)) {
                        best = ov;
                        bi = oi;
                    }
                }
                if (q == 0) {
                    dl[cur][c2] = c2 < nc ? best + loc[c2] : NINF;
                    if (c2 < nc) psi[(size_t)k * PITCH_PSI + c2] = (unsigned char)bi;
                }
            }
            nc_prev = nc;
            pitch_wave_sync();
        }
        __syncthreads();
    }
    // the last frame's first maximum
    int c = 0;
    {
        const int cur = (nF - 1) & 1;
        double best = dl[cur][0];
        for (int i = 1; i < nc_prev; ++i)
            if (dl[cur][i] > best) {
                best = dl[cur][i];
                c = i;
            }
    }
    __threadfence();                                    // the backpointer rows, read back by other lanes of the wave
    for (int kend = nF - 1; kend >= 0; kend -= 64) {
        const int kstart = kend - 63 > 0 ? kend - 63 : 0;
        if (kstart + t <= kend && kstart + t > 0)       // (frame 0 has no backpointers)
            *(uint4*)rows[t] = *(const uint4*)(psi + (size_t)(kstart + t) * PITCH_PSI);
        __syncthreads();
        if (t == 0) {
            for (int k = kend; k >= kstart; --k) {
                sel[k - kstart] = c;
                if (k > 0) {
                    const int prev = rows[k - kstart][c];
                    c = prev < PITCH_CAND ? prev : 0;   // (always: a written backpointer is a slot)
                }
            }
        }
        __syncthreads();
        c = __shfl(c, 0, 64);
        const int k = kstart + t;
        if (k <= kend) {
            const int sl = sel[t];
            const double f = cand[(size_t)k * (2 * PITCH_CAND) + 2 * sl];
            f0[k] = (f > 0.0 && f < p.ceiling) ? f : 0.0;
            if (selected) selected[k] = sl;
        }
        __syncthreads();
    }
}

static int pitch_max_frames(const PitchParams& p) { return pitch_frames(p.wav_ld, p.g.first, p.hop); }

hipError_t pitch_stats_launch(const PitchParams& p, hipStream_t stream) {
    if (p.B < 1 || !p.gpeak || !p.n_frames) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_stats_kernel, dim3((unsigned)p.B), dim3(PITCH_STATS_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t pitch_acf_launch(const PitchParams& p, hipStream_t stream) {
    const int threads = pitch_acf_threads(p.g.n_lag), nf = pitch_max_frames(p);
    if (p.B < 1 || p.B > 65535 || threads > 256 || p.g.nsw > PITCH_MAX_NSW || !p.acf || !p.intensity || nf > p.frames_ld) return hipErrorInvalidValue;
    if (nf == 0) return hipSuccess;
    const int lds_n = pitch_acf_lds(p.g.nsw, threads);
    hipLaunchKernelGGL(pitch_acf_kernel, dim3((unsigned)nf, (unsigned)p.B), dim3(threads), (size_t)lds_n * sizeof(double), stream, p, lds_n);
    return hipGetLastError();
}

hipError_t pitch_candidates_launch(const PitchParams& p, hipStream_t stream) {
    const int nf = pitch_max_frames(p);
    if (p.B < 1 || p.B > 65535 || !p.acf || !p.cand || !p.n_cand || nf > p.frames_ld) return hipErrorInvalidValue;
    if (nf == 0) return hipSuccess;
    hipLaunchKernelGGL(pitch_candidates_kernel, dim3((unsigned)nf, (unsigned)p.B), dim3(64), (size_t)p.g.n_lag * sizeof(double), stream, p);
    return hipGetLastError();
}

hipError_t pitch_path_launch(const PitchParams& p, hipStream_t stream) {
    if (p.B < 1 || !p.cand || !p.n_cand || !p.intensity || !p.psi || !p.f0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_path_kernel, dim3((unsigned)p.B), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// the window w [nsw] and its normalised autocorrelation wr [n_lag], in float64 (sums carried in long double)
static std::vector<double> pitch_tables(const PitchGeometry& g) {
    std::vector<double> t((size_t)g.nsw + g.n_lag);
    for (int j = 0; j < g.nsw; ++j) t[j] = 0.5 - 0.5 * std::cos(2.0 * PITCH_PI * (double)(j + 1) / (double)(g.nsw + 1));
    long double w0 = 0.0L;
    for (int j = 0; j < g.nsw; ++j) w0 += (long double)t[j] * (long double)t[j];
    for (int l = 0; l < g.n_lag; ++l) {
        long double s = 0.0L;
        for (int j = 0; j + l < g.nsw; ++j) s += (long double)t[j] * (long double)t[j + l];
        t[(size_t)g.nsw + l] = (double)(s / w0);
    }
    return t;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_PITCH): four launches on the caller's stream; no host synchronisation unless the workspace grows or a
// new window length uploads its tables.  h may be null: the block is checked first, so that the refusals are reachable without a device
int pitch_forward(dtts_ctx* h, const dtts_pitch_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_PITCH)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B <= 0 || a->B > 65535) return fail(h, DTTS_E_INVAL, "%s: B = %d (supported: 1 .. 65535)", me, a->B);
    if (a->wav_ld < 1 || a->wav_ld > PITCH_MAX_WAV) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 1 .. %d)", me, a->wav_ld, PITCH_MAX_WAV);
    if (a->sample_rate < 8000 || a->sample_rate > 48000) return fail(h, DTTS_E_INVAL, "%s: sample_rate = %d (supported: 8000 .. 48000)", me, a->sample_rate);
    if (a->hop < 1 || a->hop > 4096) return fail(h, DTTS_E_INVAL, "%s: hop = %d (supported: 1 .. 4096)", me, a->hop);
    if (!std::isfinite(a->pitch_floor) || a->pitch_floor < 10.0) return fail(h, DTTS_E_INVAL, "%s: pitch_floor = %g (must be finite and >= 10)", me, a->pitch_floor);
    const PitchGeometry g = pitch_geometry(a->sample_rate, a->pitch_floor);
    if (g.nsw < 32 || g.nsw > PITCH_MAX_NSW)
        return fail(h, DTTS_E_INVAL, "%s: pitch_floor = %g gives a window of %d samples at sample_rate = %d (supported: 32 .. %d)", me, a->pitch_floor, g.nsw,
                    a->sample_rate, PITCH_MAX_NSW);
    if (!std::isfinite(a->pitch_ceiling) || !(a->pitch_ceiling > a->pitch_floor))
        return fail(h, DTTS_E_INVAL, "%s: pitch_ceiling = %g (must be finite and above pitch_floor = %g)", me, a->pitch_ceiling, a->pitch_floor);
    if (!std::isfinite(a->voicing_threshold) || !(a->voicing_threshold > 0.0))
        return fail(h, DTTS_E_INVAL, "%s: voicing_threshold = %g (must be finite and > 0)", me, a->voicing_threshold);
    if (!std::isfinite(a->silence_threshold) || !(a->silence_threshold > 0.0))
        return fail(h, DTTS_E_INVAL, "%s: silence_threshold = %g (must be finite and > 0)", me, a->silence_threshold);
    const std::pair<const char*, double> costs[] = {{"octave_cost", a->octave_cost}, {"octave_jump_cost", a->octave_jump_cost},
                                                    {"voiced_unvoiced_cost", a->voiced_unvoiced_cost}};
    for (const auto& c : costs)
        if (!std::isfinite(c.second) || c.second < 0.0) return fail(h, DTTS_E_INVAL, "%s: %s = %g (must be finite and >= 0)", me, c.first, c.second);
    const int nf_max = pitch_frames(a->wav_ld, g.first, a->hop);
    if (a->frames_ld < 1 || a->frames_ld > PITCH_MAX_FRAMES || a->frames_ld < nf_max)
        return fail(h, DTTS_E_INVAL, "%s: frames_ld = %d frames (supported: 1 .. %d; wav_ld = %d samples give %d)", me, a->frames_ld, PITCH_MAX_FRAMES, a->wav_ld, nf_max);
    if (!a->wav_dev || !a->f0_dev || !a->n_frames_dev) return fail(h, DTTS_E_INVAL, "%s: null wav_dev / f0_dev / n_frames_dev", me);
    if (int rc = blk.aligned(4, {{"wav_dev", a->wav_dev}, {"lens_dev", a->lens_dev}, {"n_frames_dev", a->n_frames_dev}, {"n_cand_dev", a->n_cand_dev},
                                 {"selected_dev", a->selected_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"f0_dev", a->f0_dev}, {"acf_dev", a->acf_dev}, {"cand_dev", a->cand_dev}, {"intensity_dev", a->intensity_dev}})) return rc;
    if (int rc = blk.handle()) return rc;

    auto it = h->pitch_tabs.find(g.nsw);
    if (it == h->pitch_tabs.end()) {
        double* d = upload(h, pitch_tables(g));
        if (!d) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
        it = h->pitch_tabs.emplace(g.nsw, d).first;
    }
    PitchParams p{};
    p.wav = a->wav_dev;
    p.lens = a->lens_dev;
    p.win = it->second;
    p.wr = it->second + g.nsw;
    p.f0 = a->f0_dev;
    p.n_frames = a->n_frames_dev;
    p.selected = a->selected_dev;
    p.sr = (double)a->sample_rate;
    p.floor_hz = a->pitch_floor;
    p.ceiling = std::min(a->pitch_ceiling, 0.5 * (double)a->sample_rate);
    p.vt = a->voicing_threshold;
    p.st = a->silence_threshold;
    p.oc = a->octave_cost;
    const double corr = 0.01 / ((double)a->hop / (double)a->sample_rate);
    p.oj = a->octave_jump_cost * corr;
    p.vu = a->voiced_unvoiced_cost * corr;
    p.B = a->B;
    p.wav_ld = a->wav_ld;
    p.frames_ld = a->frames_ld;
    p.hop = a->hop;
    p.g = g;
    const size_t frames = (size_t)a->B * a->frames_ld;
    const size_t n_acf = a->acf_dev ? 0 : frames * g.n_lag, n_cand = a->cand_dev ? 0 : frames * 2 * PITCH_CAND, n_nc = a->n_cand_dev ? 0 : frames,
                 n_in = a->intensity_dev ? 0 : frames;
    HIPCHK(h->a_pitch.reserve((size_t)a->B * sizeof(double) + (n_acf + n_cand + n_in) * sizeof(double) + n_nc * sizeof(int) + frames * PITCH_PSI + 6 * 256, stream));
    p.gpeak = h->a_pitch.alloc<double>((size_t)a->B);
    p.acf = a->acf_dev ? a->acf_dev : h->a_pitch.alloc<double>(n_acf);
    p.cand = a->cand_dev ? a->cand_dev : h->a_pitch.alloc<double>(n_cand);
    p.n_cand = a->n_cand_dev ? a->n_cand_dev : h->a_pitch.alloc<int>(n_nc);
    p.intensity = a->intensity_dev ? a->intensity_dev : h->a_pitch.alloc<double>(n_in);
    p.psi = h->a_pitch.alloc<unsigned char>(frames * PITCH_PSI);
    if (!p.gpeak || !p.acf || !p.cand || !p.n_cand || !p.intensity || !p.psi) return blk.workspace();
    LAUNCH(pitch_stats_launch(p, stream));
    LAUNCH(pitch_acf_launch(p, stream));
    LAUNCH(pitch_candidates_launch(p, stream));
    LAUNCH(pitch_path_launch(p, stream));
    return DTTS_OK;
}

} // namespace dtts
