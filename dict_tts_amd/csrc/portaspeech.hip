// libdicttts_hip.so — the PortaSpeech baseline (modules/portaspeech/model.py::PortaSpeech, dur_level: word): kernels of its linguistic
// front (portaspeech.h), its weights (DTTS_PART_PORTASPEECH) and its encode (dtts_text2mel_fetch(DTTS_PS_ENCODE)).  The duration predictor, the
// FFT block stack of the word encoder, the length regulator and the FVAE are the Dict-TTS path's (text2mel.hip, fft_blocks.hip, ops.hip).
#include "ctx.h"

namespace dtts {

namespace {

__device__ __forceinline__ float ps_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float ps_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ long long ps_wave_min_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------
__global__ void ps_ln_relu_kernel(const float* x, float* y, const float* gamma, const float* beta, float eps, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (long long)row * C;
    float* yr = y + (long long)row * C;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += xr[c];
    const float mean = ps_wave_sum(sum) / (float)C;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = xr[c] - mean;
        sq += d * d;
    }
    const float inv = 1.0f / sqrtf(ps_wave_sum(sq) / (float)C + eps);
    for (int c = lane; c < C; c += 64) yr[c] = fmaxf((xr[c] - mean) * inv * gamma[c] + beta[c], 0.f);
}

// ---------------------------------------------------------------------------------------------------------
// Relative-position attention in the form of mha_kernel (ops.hip): block = 4 waves x 4 queries, K / V tiles of 64 keys in LDS, a lane
// owns a key of the tile, online softmax.  Per query the 2 w + 1 band logits q_i.Ek[m] are formed before the key loop and added where the
// tile covers j = i + m - w; the band's unnormalised probabilities are carried in LDS, rescaled with the running maximum like the output,
// and meet Ev in the epilogue.
constexpr int PSA_QT = 16, PSA_KT = 64, PSA_DK = 96, PSA_NREL = 2 * PS_MAX_WINDOW + 1;
__global__ __launch_bounds__(256) void ps_rel_attn_kernel(const float* qkv, float* out, const int* lens, const float* ek, const float* ev,
                                                          int window, int T, int C, int dk) {
    __shared__ float qs[PSA_QT][PSA_DK];
    __shared__ float ks[PSA_KT][PSA_DK + 1];
    __shared__ float vs[PSA_KT][PSA_DK];
    __shared__ float ps[PSA_QT][PSA_KT];
    __shared__ float bl[PSA_QT][PSA_NREL];   // band logits q_i . Ek[m]
    __shared__ float bp[PSA_QT][PSA_NREL];   // band probabilities (unnormalised, at the running maximum)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * PSA_QT;
    const int len = min(max(lens[b], 0), T), nrel = 2 * window + 1;
    const float* base = qkv + (long long)b * T * 3 * C;
    const float inv_sqrt = 1.0f / sqrtf((float)dk);
    if (q0 >= len) {   // a tile of padded queries: zeros (the caller masks these rows)
        for (int idx = tid; idx < PSA_QT * dk; idx += 256) {
            const int i = idx / dk, d = idx % dk;
            if (q0 + i < T) out[((long long)b * T + q0 + i) * C + h * dk + d] = 0.f;
        }
        return;
    }
    for (int idx = tid; idx < PSA_QT * dk; idx += 256) {
        const int i = idx / dk, d = idx % dk;
        qs[i][d] = (q0 + i < len) ? base[(long long)(q0 + i) * 3 * C + h * dk + d] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < PSA_QT * nrel; idx += 256) {
        const int i = idx / nrel, m = idx % nrel;
        float acc = 0.f;
        for (int d = 0; d < dk; ++d) acc += qs[i][d] * ek[m * dk + d];
        bl[i][m] = acc;
        bp[i][m] = 0.f;
    }
    float m_[4], l[4], o0[4], o1[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) { m_[qi] = -1e30f; l[qi] = 0.f; o0[qi] = 0.f; o1[qi] = 0.f; }
    for (int j0 = 0; j0 < len; j0 += PSA_KT) {
        __syncthreads();
        for (int idx = tid; idx < PSA_KT * dk; idx += 256) {
            const int j = idx / dk, d = idx % dk;
            const bool ok = j0 + j < len;
            const float* r = base + (long long)(j0 + j) * 3 * C + h * dk + d;
            ks[j][d] = ok ? r[C] : 0.f;
            vs[j][d] = ok ? r[2 * C] : 0.f;
        }
        __syncthreads();
        const int j = j0 + lane;
        float sc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < dk; ++d) {
            const float kv = ks[lane][d];
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) sc[qi] += qs[wave * 4 + qi][d] * kv;
        }
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            const int q = wave * 4 + qi, i = q0 + q;
            const int rel = j - i + window;
            const bool live = j < len, band = live && rel >= 0 && rel < nrel;
            float s = sc[qi] * inv_sqrt;
            if (band) s += bl[q][rel] * inv_sqrt;
            const float tmax = ps_wave_max(live ? s : -1e30f);
            const float mn = fmaxf(m_[qi], tmax);
            const float alpha = expf(m_[qi] - mn);
            const float p = live ? expf(s - mn) : 0.f;   // a key past the end: the reference's -1e4 fill underflows to exactly 0
            l[qi] = l[qi] * alpha + ps_wave_sum(p);
            o0[qi] *= alpha;
            o1[qi] *= alpha;
            m_[qi] = mn;
            ps[q][lane] = p;
            if (lane < nrel) bp[q][lane] *= alpha;
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the rescale lands before the band's own write (rows are private to the wave)
            __builtin_amdgcn_wave_barrier();
            if (band) bp[q][rel] = p;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
        const int jn = min(PSA_KT, len - j0);
        for (int jj = 0; jj < jn; ++jj) {
            const float v0 = vs[jj][lane];
            const float v1 = (lane + 64 < dk) ? vs[jj][lane + 64] : 0.f;
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const float p = ps[wave * 4 + qi][jj];
                o0[qi] += p * v0;
                o1[qi] += p * v1;
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
        const int q = wave * 4 + qi, i = q0 + q;
        if (i >= T) continue;
        float* dst = out + ((long long)b * T + i) * C + h * dk;
        if (i >= len) {
            if (lane < dk) dst[lane] = 0.f;
            if (lane + 64 < dk) dst[lane + 64] = 0.f;
            continue;
        }
        float r0 = 0.f, r1 = 0.f;   // sum_m p_band[m] Ev[m], ascending m
        for (int m = 0; m < nrel; ++m) {
            const float p = bp[q][m];
            if (lane < dk) r0 += p * ev[m * dk + lane];
            if (lane + 64 < dk) r1 += p * ev[m * dk + lane + 64];
        }
        const float inv = 1.0f / l[qi];
        if (lane < dk) dst[lane] = (o0[qi] + r0) * inv;
        if (lane + 64 < dk) dst[lane + 64] = (o1[qi] + r1) * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------
// the first violation of an utterance as one comparable word: position in the high bits, then the code; value kept beside it
__device__ __forceinline__ long long ps_key(int pos, int code) { return ((long long)pos << 8) | code; }
constexpr long long PS_NO_KEY = 0x7fffffffffffffffLL;

__global__ __launch_bounds__(64) void ps_scan_phonemes_kernel(const int64_t* txt, const int64_t* ph2word, int n_phone, int T_ph, int T_w, int* wstart,
                                                              int* wcnt, float* ph_pos, long long* ustat) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* tk = txt + (long long)b * T_ph;
    const int64_t* pw = ph2word + (long long)b * T_ph;
    int* ws = wstart + (long long)b * (T_w + 1);
    int* wc = wcnt + (long long)b * (T_w + 1);
    int n = 0;
    for (int t = lane; t < T_ph; t += 64) n += tk[t] > 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    const int len = n;
    for (int w = lane; w <= T_w; w += 64) {
        ws[w] = 0;
        wc[w] = 0;
    }
    long long key = PS_NO_KEY, val = 0;
    for (int t = lane; t < T_ph && key == PS_NO_KEY; t += 64) {   // ascending t per lane: a lane's first violation is its lowest
        const long long tok = tk[t], w = pw[t], prev = t > 0 ? pw[t - 1] : 0;
        int code = 0;
        long long v = 0;
        if (tok < 0 || tok >= n_phone) { code = DTTS_PS_BAD_TOKEN; v = tok; }
        else if (t < len && tok == 0) { code = DTTS_PS_ZERO_TOKEN; v = tok; }
        else if (w < 0 || w > T_w || (t < len && (w < prev || w > prev + 1)) || (t >= len && w != 0)) { code = DTTS_PS_BAD_PH2WORD; v = w; }
        if (code) {
            key = ps_key(t, code);
            val = v;
        }
    }
    const long long first = ps_wave_min_ll(key);
    if (first != PS_NO_KEY) {   // refused: empty spans, zero positions
        for (int t = lane; t < T_ph; t += 64) ph_pos[(long long)b * T_ph + t] = 0.f;
        if (key == first) {   // exactly one lane holds the lowest position
            ustat[b * 4 + 0] = b + 1;
            ustat[b * 4 + 1] = first & 0xff;
            ustat[b * 4 + 2] = val;
            ustat[b * 4 + 3] = first >> 8;
        }
        return;
    }
    if (lane < 4) ustat[b * 4 + lane] = 0;
    __syncthreads();
    // a word is one run of the live prefix: its first phoneme writes the start, its last one the end (kept in wcnt until the next step)
    for (int t = lane; t < len; t += 64) {
        const int w = (int)pw[t];
        if (w < 1) continue;
        if (t == 0 || pw[t - 1] != w) ws[w] = t;
        if (t == len - 1 || pw[t + 1] != w) wc[w] = t + 1;
    }
    __syncthreads();
    for (int w = 1 + lane; w <= T_w; w += 64)
        if (wc[w] > 0) wc[w] -= ws[w];
    __syncthreads();
    for (int t = lane; t < T_ph; t += 64) {
        const int w = t < len ? (int)pw[t] : 0;
        ph_pos[(long long)b * T_ph + t] = w >= 1 ? (float)(t - ws[w] + 1) / (float)wc[w] : 0.f;
    }
}

__global__ __launch_bounds__(64) void ps_scan_frames_kernel(const int64_t* m2w, const int* wcnt, int T_mel, int T_w, int* fstart, int* fcnt,
                                                            long long* ustat) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* mw = m2w + (long long)b * T_mel;
    const int* wc = wcnt + (long long)b * (T_w + 1);
    int* fs = fstart + (long long)b * (T_w + 1);
    int* fc = fcnt + (long long)b * (T_w + 1);
    for (int w = lane; w <= T_w; w += 64) {
        fs[w] = 0;
        fc[w] = 0;
    }
    long long key = PS_NO_KEY, val = 0;
    for (int f = lane; f < T_mel && key == PS_NO_KEY; f += 64) {
        const long long w = mw[f], prev = f > 0 ? mw[f - 1] : -1;
        int code = 0;
        if (w < 0 || w > T_w || (f > 0 && (prev == 0 ? w != 0 : (w != 0 && w < prev)))) code = DTTS_PS_BAD_MEL2WORD;
        else if (w >= 1 && wc[w] <= 0) code = DTTS_PS_EMPTY_WORD;
        if (code) {
            key = ps_key(f, code);
            val = w;
        }
    }
    const long long first = ps_wave_min_ll(key);
    if (first != PS_NO_KEY) {
        if (key == first) {
            ustat[b * 4 + 0] = b + 1;
            ustat[b * 4 + 1] = first & 0xff;
            ustat[b * 4 + 2] = val;
            ustat[b * 4 + 3] = first >> 8;
        }
        if ((first & 0xff) == DTTS_PS_BAD_MEL2WORD) return;   // no spans: every frame of the utterance gets position 0
    } else if (lane < 4) {
        ustat[b * 4 + lane] = 0;
    }
    __syncthreads();
    for (int f = lane; f < T_mel; f += 64) {
        const int w = (int)mw[f];
        if (w < 1) continue;
        if (f == 0 || mw[f - 1] != w) fs[w] = f;
        if (f == T_mel - 1 || mw[f + 1] != w) fc[w] = f + 1;
    }
    __syncthreads();
    for (int w = 1 + lane; w <= T_w; w += 64)
        if (fc[w] > 0) fc[w] -= fs[w];
}

__global__ __launch_bounds__(64) void ps_status_kernel(const long long* ustat, int B, int merge, int64_t* status) {
    const int lane = threadIdx.x;
    long long first = PS_NO_KEY;
    for (int b = lane; b < B && first == PS_NO_KEY; b += 64)
        if (ustat[b * 4] != 0) first = b;
    first = ps_wave_min_ll(first);
    if (lane >= 4) return;
    if (merge && status[0] != 0) return;
    status[lane] = first == PS_NO_KEY ? 0 : ustat[first * 4 + lane];
}

// ---------------------------------------------------------------------------------------------------------
__global__ void ps_segment_mean_kernel(const float* ph_out, const int* wstart, const int* wcnt, float* word_in, int T_ph, int T_w, int C, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row / T_w, w = row % T_w + 1;
    const int s0 = wstart[(long long)b * (T_w + 1) + w];
    const int n = min(wcnt[(long long)b * (T_w + 1) + w], T_ph - s0);
    const float div = (float)max(n, 1);
    for (int c = lane; c < C; c += 64) {
        float acc = 0.f;
        for (int t = 0; t < n; ++t) acc += ph_out[((long long)b * T_ph + s0 + t) * C + c];
        word_in[(long long)row * C + c] = acc / div;
    }
}

__global__ void ps_dur_sum_kernel(const float* dur_ph, const int* wstart, const int* wcnt, const int* ilens_ph, float* dur_w, int* ilens_w, int B,
                                  int T_ph, int T_w) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < B) ilens_w[idx] = min(ilens_ph[idx], T_w);
    if (idx >= B * T_w) return;
    const int b = idx / T_w, w = idx % T_w + 1;
    const int s0 = wstart[(long long)b * (T_w + 1) + w];
    const int n = min(wcnt[(long long)b * (T_w + 1) + w], T_ph - s0);
    float acc = 0.f;
    for (int t = 0; t < n; ++t) acc += dur_ph[(long long)b * T_ph + s0 + t];
    dur_w[idx] = acc;
}

// [src | sin(pos f), cos(pos f)]: the sinusoid in fp32, as SinusoidalPosEmb computes it
__device__ __forceinline__ void ps_cat_row(const float* src, float pos, const float* freq, float* dst, int C, int lane) {
    const int half = C / 2;
    for (int c = lane; c < C; c += 64) dst[c] = src ? src[c] : 0.f;
    for (int i = lane; i < half; i += 64) {
        const float a = pos * freq[i];
        dst[C + i] = sinf(a);
        dst[C + half + i] = cosf(a);
    }
}
__global__ void ps_cat_phonemes_kernel(const float* ph_out, const float* ph_pos, const float* freq, float* out, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    ps_cat_row(ph_out + (long long)row * C, ph_pos[row], freq, out + (long long)row * 2 * C, C, lane);
}
__global__ void ps_cat_frames_kernel(const float* weo, const int64_t* m2w, const int* fstart, const int* fcnt, const float* freq, float* out,
                                     float* x_mask, int T_mel, int T_w, int C, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row / T_mel, f = row % T_mel;
    const long long w = m2w[row];
    const bool word = w >= 1 && w <= T_w;
    float pos = 0.f;
    if (word) {
        const int n = fcnt[(long long)b * (T_w + 1) + w];
        if (n > 0) pos = (float)(f - fstart[(long long)b * (T_w + 1) + w] + 1) / (float)n;
    }
    ps_cat_row(word ? weo + ((long long)b * T_w + (w - 1)) * C : nullptr, pos, freq, out + (long long)row * 2 * C, C, lane);
    if (lane == 0) x_mask[row] = w > 0 ? 1.f : 0.f;
}

// ---------------------------------------------------------------------------------------------------------
template <int HPL>
__global__ __launch_bounds__(256) void ps_frame_attn_kernel(const float* q, const float* kv, const int64_t* m2w, const int* wstart, const int* wcnt,
                                                            float* att, float* attn, int T_mel, int T_ph, int T_w, int rows) {
    constexpr int C = HPL * 64;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row / T_mel;
    const long long w = m2w[row];
    int s0 = 0, n = 0;
    if (w >= 1 && w <= T_w) {
        s0 = wstart[(long long)b * (T_w + 1) + w];
        n = wcnt[(long long)b * (T_w + 1) + w];
        if (s0 < 0 || s0 >= T_ph) n = 0;
        n = max(min(n, T_ph - s0), 0);
    }
    float* ar = att + (long long)row * C;
    float* wr = attn ? attn + (long long)row * T_ph : nullptr;
    if (wr)
        for (int t = lane; t < T_ph; t += 64)
            if (t < s0 || t >= s0 + n) wr[t] = 0.f;
    if (n == 0) {
#pragma unroll
        for (int c = 0; c < HPL; ++c) ar[lane + 64 * c] = 0.f;
        return;
    }
    float qv[HPL], o[HPL];
#pragma unroll
    for (int c = 0; c < HPL; ++c) {
        qv[c] = q[(long long)row * C + lane + 64 * c];
        o[c] = 0.f;
    }
    const float* kr0 = kv + ((long long)b * T_ph + s0) * 2 * C;
    float m = -1e30f, l = 0.f;
    for (int t = 0; t < n; ++t) {
        const float* kr = kr0 + (long long)t * 2 * C;
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < HPL; ++c) d += qv[c] * kr[lane + 64 * c];
        d = ps_wave_sum(d);
        if (wr && lane == (t & 63)) wr[s0 + t] = d;   // the raw logit, normalised below by the lane that wrote it
        const float mn = fmaxf(m, d), alpha = expf(m - mn), p = expf(d - mn);
        l = l * alpha + p;
#pragma unroll
        for (int c = 0; c < HPL; ++c) o[c] = o[c] * alpha + p * kr[C + lane + 64 * c];
        m = mn;
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int c = 0; c < HPL; ++c) ar[lane + 64 * c] = o[c] * inv;
    if (wr)   // the weights from the logits kept above (a span of 1: exp(0) / 1 = 1 exactly); a lane reads back its own stores only
        for (int t = lane; t < n; t += 64) wr[s0 + t] = expf(wr[s0 + t] - m) * inv;
}

} // namespace

// ---------------------------------------------------------------------------------------------------------
hipError_t ps_ln_relu_launch(const float* x, float* y, const float* gamma, const float* beta, float eps, int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(ps_ln_relu_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, y, gamma, beta, eps, rows, C);
    return hipGetLastError();
}
hipError_t ps_rel_attn_launch(const float* qkv, float* out, const int* lens, const float* ek, const float* ev, int window, int B, int T, int C,
                              int heads, hipStream_t s) {
    if (heads < 1 || C % heads || C / heads > PSA_DK || window < 1 || window > PS_MAX_WINDOW || !lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ps_rel_attn_kernel, dim3((T + PSA_QT - 1) / PSA_QT, heads, B), dim3(256), 0, s, qkv, out, lens, ek, ev, window, T, C, C / heads);
    return hipGetLastError();
}
hipError_t ps_scan_phonemes_launch(const int64_t* txt, const int64_t* ph2word, int n_phone, int B, int T_ph, int T_w, int* wstart, int* wcnt,
                                   float* ph_pos, long long* ustat, hipStream_t s) {
    hipLaunchKernelGGL(ps_scan_phonemes_kernel, dim3(B), dim3(64), 0, s, txt, ph2word, n_phone, T_ph, T_w, wstart, wcnt, ph_pos, ustat);
    return hipGetLastError();
}
hipError_t ps_scan_frames_launch(const int64_t* m2w, const int* wcnt, int B, int T_mel, int T_w, int* fstart, int* fcnt, long long* ustat,
                                 hipStream_t s) {
    hipLaunchKernelGGL(ps_scan_frames_kernel, dim3(B), dim3(64), 0, s, m2w, wcnt, T_mel, T_w, fstart, fcnt, ustat);
    return hipGetLastError();
}
hipError_t ps_status_launch(const long long* ustat, int B, int merge, int64_t* status, hipStream_t s) {
    hipLaunchKernelGGL(ps_status_kernel, dim3(1), dim3(64), 0, s, ustat, B, merge, status);
    return hipGetLastError();
}
hipError_t ps_segment_mean_launch(const float* ph_out, const int* wstart, const int* wcnt, float* word_in, int B, int T_ph, int T_w, int C,
                                  hipStream_t s) {
    hipLaunchKernelGGL(ps_segment_mean_kernel, dim3((B * T_w + 3) / 4), dim3(256), 0, s, ph_out, wstart, wcnt, word_in, T_ph, T_w, C, B * T_w);
    return hipGetLastError();
}
hipError_t ps_dur_sum_launch(const float* dur_ph, const int* wstart, const int* wcnt, const int* ilens_ph, float* dur_w, int* ilens_w, int B,
                             int T_ph, int T_w, hipStream_t s) {
    const int n = std::max(B * T_w, B);
    hipLaunchKernelGGL(ps_dur_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dur_ph, wstart, wcnt, ilens_ph, dur_w, ilens_w, B, T_ph, T_w);
    return hipGetLastError();
}
hipError_t ps_cat_phonemes_launch(const float* ph_out, const float* ph_pos, const float* freq, float* out, int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(ps_cat_phonemes_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, ph_out, ph_pos, freq, out, rows, C);
    return hipGetLastError();
}
hipError_t ps_cat_frames_launch(const float* weo, const int64_t* m2w, const int* fstart, const int* fcnt, const float* freq, float* out,
                                float* x_mask, int B, int T_mel, int T_w, int C, hipStream_t s) {
    hipLaunchKernelGGL(ps_cat_frames_kernel, dim3((B * T_mel + 3) / 4), dim3(256), 0, s, weo, m2w, fstart, fcnt, freq, out, x_mask, T_mel, T_w, C,
                       B * T_mel);
    return hipGetLastError();
}
hipError_t ps_frame_attn_launch(const float* q, const float* kv, const int64_t* m2w, const int* wstart, const int* wcnt, float* att, float* attn,
                                int B, int T_mel, int T_ph, int T_w, int C, hipStream_t s) {
    if (C % 64 || C < 64 || C > PS_MAX_HIDDEN) return hipErrorInvalidValue;
    const int rows = B * T_mel;
    const dim3 grid((rows + 3) / 4), block(256);
#define PS_FA(N)                                                                                                                       \
    case N:                                                                                                                            \
        hipLaunchKernelGGL(ps_frame_attn_kernel<N>, grid, block, 0, s, q, kv, m2w, wstart, wcnt, att, attn, T_mel, T_ph, T_w, rows); \
        break;
    switch (C / 64) {
        PS_FA(1) PS_FA(2) PS_FA(3) PS_FA(4) PS_FA(5) PS_FA(6) PS_FA(7) PS_FA(8)
    }
#undef PS_FA
    return hipGetLastError();
}

// =====================================================================================================================================
// weights
static const char* PS_ME = "dtts_finalize_weights(DTTS_PART_PORTASPEECH)";

static std::string ps_shape(const std::vector<int64_t>& s) {
    std::string r = "[";
    for (size_t i = 0; i < s.size(); ++i) r += (i ? ", " : "") + std::to_string(s[i]);
    return r + "]";
}

// the tensor `name` with exactly `shape`, or null with *rc set: DTTS_E_NOENT when absent, DTTS_E_INVAL on another shape
static const HostTensor* ps_tensor(dtts_ctx* h, const std::string& name, std::initializer_list<int64_t> shape, int* rc) {
    auto it = h->w.find(name);
    if (it == h->w.end()) {
        *rc = fail(h, DTTS_E_NOENT, "missing weight tensor '%s'", name.c_str());
        return nullptr;
    }
    const HostTensor& t = it->second;
    if (t.shape != std::vector<int64_t>(shape) || t.f.size() != (size_t)t.numel()) {
        *rc = fail(h, DTTS_E_INVAL, "%s: %s is %s; the model's is %s", PS_ME, name.c_str(), ps_shape(t.shape).c_str(),
                   ps_shape(std::vector<int64_t>(shape)).c_str());
        return nullptr;
    }
    return &t;
}

// nn.Linear(2C -> C) with bias, rows of W as output channels
static bool ps_pack_linear(dtts_ctx* h, PackedConv& L, const HostTensor* w, int C_out, int C_in, int row0, const std::vector<float>& bias) {
    const float* p = w->f.data() + (size_t)row0 * C_in;
    return pack_conv(h, L, ENG_F32, C_out, C_in, 1, [=](int co, int ci, int) { return p[(size_t)co * C_in + ci]; }, bias, 1, 1, 0);
}

int build_ps(dtts_ctx* h) {
    if (h->acoustic_ready)
        return fail(h, DTTS_E_STATE, "%s: this context holds the Dict-TTS acoustic model (DTTS_PART_ACOUSTIC); a context holds one acoustic model", PS_ME);
    const dtts_config& c = h->cfg;
    const int C = c.hidden_size, heads = c.num_heads, K = c.enc_ffn_kernel_size, n_layers = c.enc_layers;
    if (heads < 1 || C % heads || C / heads > 96 || C % 64 || C > PS_MAX_HIDDEN || n_layers < 1 || K < 1 || !(K & 1) || c.n_phone < 1)
        return fail(h, DTTS_E_INVAL, "%s: unsupported configuration (hidden_size %d a multiple of 64 up to %d, heads of at most 96 channels: num_heads %d; "
                    "enc_layers %d, an odd enc_ffn_kernel_size: %d, n_phone %d)", PS_ME, C, PS_MAX_HIDDEN, heads, n_layers, K, c.n_phone);
    const int dk = C / heads;
    int rc = DTTS_OK;
    const HostTensor* cfg = ps_tensor(h, "ps.config", {2}, &rc);
    if (!cfg) return rc;
    const int window = (int)cfg->f[0], word_layers = (int)cfg->f[1];
    if (window < 1 || window > PS_MAX_WINDOW || (float)window != cfg->f[0])
        return fail(h, DTTS_E_INVAL, "%s: ps.config window_size = %g (supported: 1 .. %d)", PS_ME, (double)cfg->f[0], PS_MAX_WINDOW);
    if (word_layers < 1 || word_layers > 64 || (float)word_layers != cfg->f[1])
        return fail(h, DTTS_E_INVAL, "%s: ps.config word_enc_layers = %g (supported: 1 .. 64)", PS_ME, (double)cfg->f[1]);
    const int nrel = 2 * window + 1;
    Need need{h, ""};
    bool ok = true;
    const std::string pe = "ps.ph_encoder.";
    const HostTensor* emb = ps_tensor(h, pe + "emb.weight", {c.n_phone, C}, &rc);
    if (!emb) return rc;
    h->ps_emb = upload(h, emb->f);
    ok = ok && h->ps_emb;
    for (int i = 0; ok && i < 3; ++i) {   // ConvReluNorm(kernel_size = 5, n_layers = 3): model.py:105-106
        const std::string p = pe + "pre.";
        if (!ps_tensor(h, p + "conv_layers." + std::to_string(i) + ".weight", {C, C, 5}, &rc)) return rc;
        ok = ok && pack_plain(h, need, h->ps_pre[i], ENG_F32, p + "conv_layers." + std::to_string(i), 1, 1, 2);
        h->ps_pre_g[i] = upload_named(h, need, p + "norm_layers." + std::to_string(i) + ".gamma");
        h->ps_pre_b[i] = upload_named(h, need, p + "norm_layers." + std::to_string(i) + ".beta");
        ok = ok && h->ps_pre_g[i] && h->ps_pre_b[i];
    }
    ok = ok && pack_plain(h, need, h->ps_pre_proj, ENG_F32, pe + "pre.proj", 1, 1, 0);
    h->ps_layers.assign(n_layers, PsLayer());
    for (int i = 0; ok && i < n_layers; ++i) {
        PsLayer& l = h->ps_layers[i];
        const std::string a = pe + "encoder.attn_layers." + std::to_string(i), f = pe + "encoder.ffn_layers." + std::to_string(i);
        const HostTensor *wq = need.get(a + ".conv_q.weight"), *wk = need.get(a + ".conv_k.weight"), *wv = need.get(a + ".conv_v.weight");
        const HostTensor *bq = need.get(a + ".conv_q.bias"), *bk = need.get(a + ".conv_k.bias"), *bv = need.get(a + ".conv_v.bias");
        if (!wq || !wk || !wv || !bq || !bk || !bv) {
            ok = false;
            break;
        }
        for (const HostTensor* t : {wq, wk, wv})
            if (t->numel() != (int64_t)C * C) return fail(h, DTTS_E_INVAL, "%s: %s.conv_q / _k / _v.weight must be [%d, %d, 1]", PS_ME, a.c_str(), C, C);
        for (const HostTensor* t : {bq, bk, bv})
            if (t->numel() != C) return fail(h, DTTS_E_INVAL, "%s: %s.conv_q / _k / _v.bias must be [%d]", PS_ME, a.c_str(), C);
        std::vector<float> bias(3 * C);
        for (int ch = 0; ch < C; ++ch) {
            bias[ch] = bq->f[ch];
            bias[C + ch] = bk->f[ch];
            bias[2 * C + ch] = bv->f[ch];
        }
        const float *pq = wq->f.data(), *pk = wk->f.data(), *pv = wv->f.data();
        ok = ok && pack_conv(h, l.qkv, ENG_F32, 3 * C, C, 1,
                             [=](int co, int ci, int) { return (co < C ? pq : co < 2 * C ? pk : pv)[(size_t)(co % C) * C + ci]; }, bias, 1, 1, 0);
        ok = ok && pack_plain(h, need, l.o, ENG_F32, a + ".conv_o", 1, 1, 0);
        const HostTensor* ekt = ps_tensor(h, a + ".emb_rel_k", {1, nrel, dk}, &rc);
        if (!ekt) return rc;
        const HostTensor* evt = ps_tensor(h, a + ".emb_rel_v", {1, nrel, dk}, &rc);
        if (!evt) return rc;
        l.ek = upload(h, ekt->f);
        l.ev = upload(h, evt->f);
        ok = ok && l.ek && l.ev;
        ok = ok && pack_plain(h, need, l.ffn1, ENG_F32, f + ".conv_1", 1, 1, K / 2);
        ok = ok && pack_plain(h, need, l.ffn2, ENG_F32, f + ".conv_2", 1, 1, 0);
        if (ok && (l.ffn1.K != K || l.ffn1.C_out != 4 * C || l.ffn1.C_in != C))
            return fail(h, DTTS_E_INVAL, "%s: %s.conv_1.weight must be [%d, %d, %d] (enc_ffn_kernel_size %d)", PS_ME, f.c_str(), 4 * C, C, K, K);
        l.g1 = upload_named(h, need, pe + "encoder.norm_layers_1." + std::to_string(i) + ".gamma");
        l.b1 = upload_named(h, need, pe + "encoder.norm_layers_1." + std::to_string(i) + ".beta");
        l.g2 = upload_named(h, need, pe + "encoder.norm_layers_2." + std::to_string(i) + ".gamma");
        l.b2 = upload_named(h, need, pe + "encoder.norm_layers_2." + std::to_string(i) + ".beta");
        ok = ok && l.g1 && l.b1 && l.g2 && l.b2;
    }
    if (ok) {   // word_encoder = FastspeechDecoder(hidden, word_enc_layers, kernel 1): FFTBlocks with the position table and the last norm
        h->ps_word.K = 1;
        h->ps_word.pos = true;
        h->ps_word.last_norm = true;
        bool wok = true;
        if (int r = build_fft_stack(h, need, h->ps_word, "ps.word_encoder.", word_layers, C, heads, &wok)) return r;
        ok = wok;
    }
    if (ok) {
        auto it = h->w.find("ps.word_encoder.pos_table");
        if (it == h->w.end()) return fail(h, DTTS_E_NOENT, "missing weight tensor 'ps.word_encoder.pos_table'");
        const HostTensor& t = it->second;
        if (t.shape.size() != 2 || t.shape[0] < 2 || t.shape[0] > (1 << 20) || t.shape[1] != C)
            return fail(h, DTTS_E_INVAL, "%s: ps.word_encoder.pos_table is %s; the model's is [n_pos >= 2, %d]", PS_ME, ps_shape(t.shape).c_str(), C);
        h->ps_pos_table = upload(h, t.f);
        h->ps_n_pos = (int)t.shape[0];
        ok = h->ps_pos_table != nullptr;
    }
    if (ok) {   // the attention of the frames: Linear(2C -> C) x 3, in_proj_weight [3C][C] (q, k, v rows), out_proj [C][C], no attention biases
        const HostTensor* we = ps_tensor(h, "ps.enc_pos_proj.weight", {C, 2 * C}, &rc);
        if (!we) return rc;
        const HostTensor* be = ps_tensor(h, "ps.enc_pos_proj.bias", {C}, &rc);
        if (!be) return rc;
        const HostTensor* wdq = ps_tensor(h, "ps.dec_query_proj.weight", {C, 2 * C}, &rc);
        if (!wdq) return rc;
        const HostTensor* bdq = ps_tensor(h, "ps.dec_query_proj.bias", {C}, &rc);
        if (!bdq) return rc;
        const HostTensor* wdr = ps_tensor(h, "ps.dec_res_proj.weight", {C, 2 * C}, &rc);
        if (!wdr) return rc;
        const HostTensor* bdr = ps_tensor(h, "ps.dec_res_proj.bias", {C}, &rc);
        if (!bdr) return rc;
        const HostTensor* win = ps_tensor(h, "ps.attn.in_proj_weight", {3 * C, C}, &rc);
        if (!win) return rc;
        const HostTensor* wout = ps_tensor(h, "ps.attn.out_proj.weight", {C, C}, &rc);
        if (!wout) return rc;
        ok = ps_pack_linear(h, h->ps_enc_pos, we, C, 2 * C, 0, be->f);
        std::vector<float> bqr(bdq->f);
        bqr.insert(bqr.end(), bdr->f.begin(), bdr->f.end());
        const float *p1 = wdq->f.data(), *p2 = wdr->f.data();
        const int C2 = 2 * C;
        ok = ok && pack_conv(h, h->ps_dec_qr, ENG_F32, 2 * C, C2, 1, [=](int co, int ci, int) { return (co < C ? p1 : p2)[(size_t)(co % C) * C2 + ci]; },
                             bqr, 1, 1, 0);
        ok = ok && ps_pack_linear(h, h->ps_q, win, C, C, 0, {});
        ok = ok && ps_pack_linear(h, h->ps_kv, win, 2 * C, C, C, {});
        ok = ok && ps_pack_linear(h, h->ps_out, wout, C, C, 0, {});
        // sin_pos frequencies exp(-i ln(10000) / (C/2 - 1)) in fp32, as SinusoidalPosEmb forms them (model.py:30-32)
        const int half = C / 2;
        std::vector<float> freq(half);
        const float step = (float)(-(std::log(10000.0) / (half - 1)));
        for (int i = 0; i < half; ++i) freq[i] = expf((float)i * step);
        h->ps_freq = upload(h, freq);
        ok = ok && h->ps_freq;
    }
    ok = ok && build_dur_predictor(h, need, "ps.");
    if (ok) {
        int r = DTTS_OK;
        ok = build_fvae(h, need, "ps.", &r);
        if (r) return r;
    }
    if (!ok) {
        if (!need.missing.empty()) return fail(h, DTTS_E_NOENT, "missing weight tensor '%s'", need.missing.c_str());
        if (h->err.empty()) return fail(h, DTTS_E_NOMEM, "%s: packing / uploading the weights failed", PS_ME);
        return DTTS_E_INVAL;
    }
    h->spk_kind = 0;
    h->post_ready = false;
    h->post_missing.clear();
    h->post_unsupported = "the posterior pass of the PortaSpeech baseline is not implemented";
    h->ps_window = window;
    h->ps_ready = true;
    return DTTS_OK;
}

// =====================================================================================================================================
// encode
static const char* ps_code_name(long long code) {
    switch (code) {
        case DTTS_PS_BAD_TOKEN: return "DTTS_PS_BAD_TOKEN: a token outside [0, n_phone)";
        case DTTS_PS_ZERO_TOKEN: return "DTTS_PS_ZERO_TOKEN: a zero token inside the live prefix";
        case DTTS_PS_BAD_PH2WORD: return "DTTS_PS_BAD_PH2WORD: ph2word must start at 0 or 1, grow by 0 or 1 per live phoneme up to T_w, and be 0 past the live prefix";
        case DTTS_PS_EMPTY_WORD: return "DTTS_PS_EMPTY_WORD: a live frame whose word has no phonemes";
        case DTTS_PS_BAD_MEL2WORD: return "DTTS_PS_BAD_MEL2WORD: mel2word must lie in [0, T_w], be non-decreasing over its non-zero prefix and 0 behind it";
    }
    return "unknown code";
}

int ps_forward(dtts_ctx* h, const dtts_ps_args* a, hipStream_t s) {
    const char* me = "dtts_text2mel_fetch(DTTS_PS_ENCODE)";
    const Block blk{h, me};
    // h may be null: the block is checked first, so that the refusals are reachable without a device
    if (!a) return fail(h, DTTS_E_INVAL, "%s: null argument block", me);
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B < 1 || a->T_ph < 1 || a->T_w < 1 || a->B > (1 << 16) || a->T_ph > (1 << 16) || a->T_w > (1 << 16))
        return fail(h, DTTS_E_INVAL, "%s: B = %d, T_ph = %d, T_w = %d (each 1 .. 65536)", me, a->B, a->T_ph, a->T_w);
    if (a->T_m2w < 0 || a->T_m2w > (1 << 20) || (a->mel2word_dev != nullptr) != (a->T_m2w > 0))
        return fail(h, DTTS_E_INVAL, "%s: T_m2w = %d with mel2word_dev %s (the columns of mel2word_dev, 1 .. %d, or 0 without it)", me, a->T_m2w,
                    a->mel2word_dev ? "given" : "null", 1 << 20);
    if (!a->txt_tokens_dev || !a->ph2word_dev || !a->status_dev || !a->T_mel_host)
        return fail(h, DTTS_E_INVAL, "%s: null txt_tokens_dev / ph2word_dev / status_dev / T_mel_host", me);
    if (int rc = blk.aligned(8, {{"txt_tokens_dev", a->txt_tokens_dev}, {"ph2word_dev", a->ph2word_dev}, {"mel2word_dev", a->mel2word_dev},
                                 {"status_dev", a->status_dev}}))
        return rc;
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_PORTASPEECH)) return rc;

    const dtts_config& c = h->cfg;
    const int B = a->B, T = a->T_ph, T_w = a->T_w, C = c.hidden_size, F = 4 * C, heads = c.num_heads, DC = c.dur_chans;
    if (T_w >= h->ps_n_pos)
        return fail(h, DTTS_E_INVAL, "%s: T_w = %d needs a word_encoder.pos_table of more than T_w rows (it has %d)", me, T_w, h->ps_n_pos);
    const size_t rows = (size_t)B * T, wrows = (size_t)B * T_w, spans = (size_t)B * (T_w + 1);
    if (rows * (size_t)F > (size_t)INT_MAX || wrows * (size_t)F > (size_t)INT_MAX)
        return fail(h, DTTS_E_INVAL, "%s: B * T_ph = %zu / B * T_w = %zu rows (one call takes at most %d / (4 hidden_size))", me, rows, wrows, INT_MAX);
    h->encoded = false;
    h->ps_encoded = false;
    h->spk_armed_B = 0;
    h->enc_spk = false;
    HIPCHK(h->a_ps.reserve((rows * (size_t)(4 * C + 3 * C + F + 2 * C + C + 2 * C + 2 * DC + 2) + wrows * (size_t)(2 * C + 3 * C + 3 * C + F + 3) +
                            spans * 3 + (size_t)B * 16) * sizeof(float) + 64 * 256, s));
    Arena& A = h->a_ps;
    float* x0 = A.alloc<float>(rows * C);
    float* hb = A.alloc<float>(rows * C);
    float* tmp = A.alloc<float>(rows * C);
    float* x = A.alloc<float>(rows * C);       // the encoder's running rows; in the end ph_encoder_out
    float* qkv = A.alloc<float>(rows * 3 * C);
    float* ff = A.alloc<float>(rows * F);
    float* cat = A.alloc<float>(rows * 2 * C);
    float* kvin = A.alloc<float>(rows * C);
    float* kv = A.alloc<float>(rows * 2 * C);
    float* d0 = A.alloc<float>(rows * DC);
    float* d1 = A.alloc<float>(rows * DC);
    float* dur_ph = A.alloc<float>(rows);
    float* ph_pos = A.alloc<float>(rows);
    float* word_in = A.alloc<float>(wrows * C);
    h->weo = A.alloc<float>(wrows * C);
    h->dur = A.alloc<float>(wrows);
    FftBufs fw;
    fw.x = A.alloc<float>(wrows * C);
    fw.hb = A.alloc<float>(wrows * C);
    fw.qkv = A.alloc<float>(wrows * 3 * C);
    fw.att = A.alloc<float>(wrows * C);
    fw.ff = A.alloc<float>(wrows * F);
    fw.lens = A.alloc<int>(B);
    fw.pos = A.alloc<int>(wrows);
    int* wstart = A.alloc<int>(spans);
    int* wcnt = A.alloc<int>(spans);
    int* starts = A.alloc<int>(spans);
    long long* ustat = A.alloc<long long>((size_t)B * 4);
    int* lens = A.alloc<int>(B);
    int* ilens_ph = A.alloc<int>(B);
    h->lens = A.alloc<int>(B);   // the words the length regulator covers: min(live phonemes, T_w)
    h->mel_lens = A.alloc<int>(B);
    if (!x0 || !hb || !tmp || !x || !qkv || !ff || !cat || !kvin || !kv || !d0 || !d1 || !dur_ph || !ph_pos || !word_in || !h->weo || !h->dur || !fw.x ||
        !fw.hb || !fw.qkv || !fw.att || !fw.ff || !fw.lens || !fw.pos || !wstart || !wcnt || !starts || !ustat || !lens || !ilens_ph || !h->lens ||
        !h->mel_lens)
        return blk.workspace();
    float* att = hb;   // the attention's output shares the prenet's rows (free once the prenet is done)
    h->B = B;
    h->T_w = T_w;
    h->L_k = 0;
    h->P = 0;
    h->pron_attn = h->dict_attn = h->context = nullptr;
    h->ps_ph_out = x;
    h->ps_T_ph = T;
    h->ps_g = h->ps_attn = nullptr;
    Timed t_encoder(h, DTTS_TIMER_STAGE_ENCODER, s);

    // ---- words and the status of the inputs
    LAUNCH(ps_scan_phonemes_launch(a->txt_tokens_dev, a->ph2word_dev, c.n_phone, B, T, T_w, wstart, wcnt, ph_pos, ustat, s));
    LAUNCH(ps_status_launch(ustat, B, 0, a->status_dev, s));
    // ---- phoneme encoder (TextEncoder, model.py:119-130): embedding * sqrt(C); the mask is the prefix mask of #(txt > 0)
    LAUNCH(embed_launch(a->txt_tokens_dev, h->ps_emb, sqrtf((float)C), x0, lens, B, T, C, c.n_phone, s));
    {   // ConvReluNorm: 3 x conv(x * mask) -> norm -> relu, then (x_org + proj(x)) * mask
        const float* in = x0;
        for (int i = 0; i < 3; ++i) {
            ConvParams p = base_params(in, C, B, T, T, tmp, C);
            p.in_lens = lens;
            LAUNCH(conv1d_launch(h->ps_pre[i], p, s));
            LAUNCH(ps_ln_relu_launch(tmp, hb, h->ps_pre_g[i], h->ps_pre_b[i], 1e-4f, (int)rows, C, s));
            in = hb;
        }
        ConvParams p = base_params(hb, C, B, T, T, x, C);
        set_res(p, 0, x0, C);
        p.out_lens = lens;
        p.zero_masked = 1;
        LAUNCH(conv1d_launch(h->ps_pre_proj, p, s));
    }
    for (const PsLayer& l : h->ps_layers) {   // Encoder.forward, post-LN (rel_transformer_encoder.py:55-79); x arrives masked
        ConvParams p = base_params(x, C, B, T, T, qkv, 3 * C);
        LAUNCH(conv1d_launch(l.qkv, p, s));
        LAUNCH(ps_rel_attn_launch(qkv, att, lens, l.ek, l.ev, h->ps_window, B, T, C, heads, s));
        p = base_params(att, C, B, T, T, tmp, C);
        set_res(p, 0, x, C);
        LAUNCH(conv1d_launch(l.o, p, s));
        // rows past the end are written as zeros here and below: they are the next layer's x * mask, and no live row reads them otherwise
        LAUNCH(layernorm_launch(tmp, x, l.g1, l.b1, 1e-4f, lens, 0, 1, B, T, C, s));
        p = base_params(x, C, B, T, T, ff, F);
        p.in_lens = lens;
        p.post_act = 1;
        LAUNCH(conv1d_launch(l.ffn1, p, s));
        p = base_params(ff, F, B, T, T, tmp, C);
        p.in_lens = lens;
        p.out_lens = lens;
        p.zero_masked = 1;
        set_res(p, 0, x, C);
        LAUNCH(conv1d_launch(l.ffn2, p, s));
        LAUNCH(layernorm_launch(tmp, x, l.g2, l.b2, 1e-4f, lens, 0, 1, B, T, C, s));
    }
    // ---- words: mean pooling, the word encoder (its padding from all-zero rows), durations per phoneme summed per word
    LAUNCH(ps_segment_mean_launch(x, wstart, wcnt, word_in, B, T, T_w, C, s));
    if (int rc = run_fft_stack(h, h->ps_word, word_in, nullptr, h->ps_pos_table, h->ps_n_pos, B, T_w, C, heads, h->weo, fw, s)) return rc;
    LAUNCH(rowcount_nonzero_launch(x, ilens_ph, B, T, C, s));
    if (int rc = run_dur_predictor(h, x, C, ilens_ph, d0, d1, dur_ph, B, T, s)) return rc;
    LAUNCH(ps_dur_sum_launch(dur_ph, wstart, wcnt, ilens_ph, h->dur, h->lens, B, T, T_w, s));
    // ---- the keys / values of the frame attention: Wk | Wv of enc_pos_proj([ph_encoder_out, enc_pos])
    LAUNCH(ps_cat_phonemes_launch(x, ph_pos, h->ps_freq, cat, (int)rows, C, s));
    {
        ConvParams p = base_params(cat, 2 * C, B, T, T, kvin, C);
        LAUNCH(conv1d_launch(h->ps_enc_pos, p, s));
        p = base_params(kvin, C, B, T, T, kv, 2 * C);
        LAUNCH(conv1d_launch(h->ps_kv, p, s));
    }
    // ---- durations -> mel2word
    int T_raw = 0;
    if (!a->mel2word_dev) {
        LAUNCH(durations_launch(h->dur, h->lens, starts, h->mel_lens, B, T_w, s));
        std::vector<int> tot(B);
        long long st[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(tot.data(), h->mel_lens, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(st, a->status_dev, sizeof st, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));   // the one host sync of the path: T_mel sizes every later buffer
        if (st[0])
            return fail(h, DTTS_E_INVAL, "%s: utterance %lld, position %lld, value %lld: %s", me, st[0] - 1, st[3], st[2], ps_code_name(st[1]));
        for (int b = 0; b < B; ++b) T_raw = std::max(T_raw, tot[b]);
    } else {
        T_raw = a->T_m2w;
    }
    if (int rc = lay_out_frames(h, a->mel2word_dev, a->T_m2w, T_raw, starts, h->lens, T_w, s, a->T_mel_host)) return rc;
    h->encoded = false;   // until the frames' half below is enqueued
    const int T_mel = h->T_mel;
    const size_t mrows = (size_t)B * T_mel;
    if (mrows * (size_t)(2 * C) > (size_t)INT_MAX || (a->want_attn && mrows * (size_t)T > (size_t)INT_MAX))
        return fail(h, DTTS_E_INVAL, "%s: B * T_mel = %zu frames (one call takes at most %d / (2 hidden_size); with want_attn %d / T_ph)", me, mrows, INT_MAX,
                    INT_MAX);
    // ---- frames: spans and positions, e = pad0(word_encoder_out)[mel2word], the two projections, the attention over the word's phonemes
    HIPCHK(h->a_psf.reserve((mrows * (size_t)(2 * C + 2 * C + C + C + C + (a->want_attn ? T : 0)) + spans * 2 + (size_t)B * 8) * sizeof(float) + 16 * 256, s));
    Arena& Af = h->a_psf;
    float* catf = Af.alloc<float>(mrows * 2 * C);
    float* qr = Af.alloc<float>(mrows * 2 * C);
    float* q = Af.alloc<float>(mrows * C);
    float* attf = Af.alloc<float>(mrows * C);
    float* g = Af.alloc<float>(mrows * C);
    float* attn = a->want_attn ? Af.alloc<float>(mrows * T) : nullptr;
    int* fstart = Af.alloc<int>(spans);
    int* fcnt = Af.alloc<int>(spans);
    long long* ustat_f = Af.alloc<long long>((size_t)B * 4);
    if (!catf || !qr || !q || !attf || !g || (a->want_attn && !attn) || !fstart || !fcnt || !ustat_f) return blk.workspace();
    LAUNCH(ps_scan_frames_launch(h->m2w, wcnt, B, T_mel, T_w, fstart, fcnt, ustat_f, s));
    LAUNCH(ps_status_launch(ustat_f, B, 1, a->status_dev, s));
    LAUNCH(ps_cat_frames_launch(h->weo, h->m2w, fstart, fcnt, h->ps_freq, catf, h->x_mask, B, T_mel, T_w, C, s));
    {
        ConvParams p = base_params(catf, 2 * C, B, T_mel, T_mel, qr, 2 * C);   // dec_query_proj | dec_res_proj
        LAUNCH(conv1d_launch(h->ps_dec_qr, p, s));
        p = base_params(qr, 2 * C, B, T_mel, T_mel, q, C);                    // q = Wq q_in * C^-0.5
        p.out_mul = (float)std::pow((double)C, -0.5);
        LAUNCH(conv1d_launch(h->ps_q, p, s));
    }
    LAUNCH(ps_frame_attn_launch(q, kv, h->m2w, wstart, wcnt, attf, attn, B, T_mel, T, T_w, C, s));
    {   // decoder_inp = (out_proj(attention) + x_res) * (mel2word > 0)
        ConvParams p = base_params(attf, C, B, T_mel, T_mel, g, C);
        set_res(p, 0, qr, 2 * C);
        p.seg[0].coff_res = C;
        p.row_mask = h->x_mask;
        LAUNCH(conv1d_launch(h->ps_out, p, s));
    }
    h->ps_g = g;
    h->ps_attn = attn;
    h->ps_encoded = true;
    h->encoded = true;
    return DTTS_OK;
}

} // namespace dtts
