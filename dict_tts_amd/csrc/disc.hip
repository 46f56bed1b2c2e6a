// libdicttts_hip.so — HifiGAN's discriminators on B waveform pairs (disc.h; dtts_text2mel_fetch(DTTS_OUT_DISC)).  Per discriminator:
// the row counts of every layer (device), the entry layer (C_in = 1: VALU), the dense layers on conv1d_launch (exact fp32 products, a fixed
// summation order per row), the grouped layers on gconv_launch, conv_post as one wave per row, then the fp64 sums per utterance.  With
// DTTS_DISC_FM every layer's output is followed by its feature sums: fixed tiles of DISC_FM_TILE floats, then the tiles in order.
#include "ctx.h"

namespace dtts {

typedef __attribute__((ext_vector_type(4))) float f32x4;

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * DISC_SLOPE; }

// ---- lengths: vlen[b] (0 for a refused pair) and status[b]
__global__ void disc_vlen_kernel(const int* lens, int B, int wav_ld, int* vlen, int* status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int L = lens ? lens[b] : wav_ld;
    const bool ok = L >= DTTS_DISC_MIN_LEN && L <= wav_ld;
    vlen[b] = ok ? L : 0;
    status[b] = ok ? 0 : DTTS_DISC_TOO_SHORT;
}

struct DiscChain {
    int n;              // layers
    int k[8], s[8], pad[8];
};

// tab[0][i] = input rows of sequence i (period: ceil(L / p) rows per column; scale: L pooled `pools` times), tab[l + 1][i] = rows after layer l
__global__ void disc_rows_kernel(const int* vlen, int B, int period, int pools, DiscChain c, int* tab, int nseq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseq) return;
    const int b = (i / period) % B;
    int r = vlen[b];
    if (period > 1) r = (r + period - 1) / period;
    for (int q = 0; q < pools; ++q) r = r / 2;   // AvgPool1d(4, 2, padding = 1): (r + 2 - 4) / 2 + 1
    tab[i] = r;
    for (int l = 0; l < c.n; ++l) {
        r = r > 0 ? (r + 2 * c.pad[l] - c.k[l]) / c.s[l] + 1 : 0;
        tab[(size_t)(l + 1) * nseq + i] = r;
    }
}

// ---- AvgPool1d(4, 2, padding = 1), count_include_pad: out[i] = (x[2i - 1] + x[2i] + x[2i + 1] + x[2i + 2]) / 4, zeros outside [0, in_len)
__global__ void disc_pool_kernel(const float* x0, const float* x1, int ld_in, const int* vlen, int B, int pools_in, float* out, int ld_out) {
    const int s = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    int n = vlen[s % B];
    for (int q = 0; q < pools_in; ++q) n = n / 2;
    if (i >= n / 2) return;
    const float* x = s < B ? x0 + (size_t)s * ld_in : x1 + (size_t)(s - B) * ld_in;
    float acc = 0.f;
#pragma unroll
    for (int k = -1; k <= 2; ++k) {
        const int j = 2 * i + k;
        acc += (j >= 0 && j < n) ? x[j] : 0.f;
    }
    out[(size_t)s * ld_out + i] = acc * 0.25f;
}

// ---- entry layer of a period discriminator: Conv2d(1 -> 32, (5, 1), stride (3, 1), pad (2, 0)) on the waveform folded to [rows][p], the
// reflect padding of the last row by index arithmetic
struct MpdEntryParams {
    const float *y, *yh;     // [B][wav_ld]
    const int* vlen;         // [B]
    const int* in_rows;      // [nseq]
    const int* out_lens;     // [nseq]
    const float *w, *bias;   // [32][5], [32]
    float* out;              // [nseq][T_out][32]
    int B, wav_ld, period, T_out;
};
__global__ __launch_bounds__(256) void disc_mpd_entry_kernel(const MpdEntryParams p) {
    const int seq = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    const int r1 = e >> 5, c = e & 31;
    if (r1 >= p.out_lens[seq]) return;
    const int s = seq / p.period, j = seq - s * p.period, b = s % p.B;
    const int L = p.vlen[b], R0 = p.in_rows[seq];
    const float* src = (s < p.B ? p.y : p.yh) + (size_t)b * p.wav_ld;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int r = r1 * 3 + k - 2;
        if (r < 0 || r >= R0) continue;
        int i = r * p.period + j;
        if (i >= L) i = 2 * L - 2 - i;   // F.pad(x, (0, n_pad), "reflect")
        acc = fmaf(p.w[c * 5 + k], src[i], acc);
    }
    p.out[((size_t)seq * p.T_out + r1) * 32 + c] = acc + p.bias[c];
}

// ---- entry layer of a scale discriminator: Conv1d(1 -> 128, k = 15, pad 7).  A thread owns one channel and MSD_ENTRY_ROWS consecutive
// outputs: its 15 weights and the 30-sample window stay in registers, a wave's stores are 256 contiguous bytes per row
constexpr int MSD_ENTRY_ROWS = 16;
struct MsdEntryParams {
    const float *x0, *x1;    // sequences s < B at x0 + s * ld, the rest at x1 + (s - B) * ld
    const int* lens;         // [2B] rows in = rows out
    const float *w, *bias;   // [15][128] (transposed at pack time), [128]
    float* out;              // [2B][T][128]
    int B, ld, T;
};
__global__ __launch_bounds__(256) void disc_msd_entry_kernel(const MsdEntryParams p) {
    const int s = blockIdx.y, c = threadIdx.x & 127;
    const int t0 = (blockIdx.x * 2 + (threadIdx.x >> 7)) * MSD_ENTRY_ROWS;
    const int n = p.lens[s];
    if (t0 >= n) return;
    const float* x = s < p.B ? p.x0 + (size_t)s * p.ld : p.x1 + (size_t)(s - p.B) * p.ld;
    float w[15], xv[MSD_ENTRY_ROWS + 14];
#pragma unroll
    for (int k = 0; k < 15; ++k) w[k] = p.w[k * 128 + c];
#pragma unroll
    for (int j = 0; j < MSD_ENTRY_ROWS + 14; ++j) {
        const int i = t0 + j - 7;
        xv[j] = (i >= 0 && i < n) ? x[i] : 0.f;
    }
    const float bias = p.bias[c];
    float* o = p.out + ((size_t)s * p.T + t0) * 128 + c;
#pragma unroll
    for (int u = 0; u < MSD_ENTRY_ROWS; ++u) {
        if (t0 + u >= n) break;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 15; ++k) acc = fmaf(w[k], xv[u + k], acc);
        o[(size_t)u * 128] = acc + bias;
    }
}

// ---- conv_post (1024 -> 1, k = 3, pad 1) on leaky_relu(x): one wave per output row, a fixed order within the lane and a fixed tree across
// the wave.  D goes to dws[s][r * period + j]: the reference's flattened order
struct PostParams {
    const float* x;          // [nseq][T][1024] pre-activation
    const int* lens;         // [nseq]
    const float* w;          // [3][1024]
    float bias;
    float* dws;              // [2B][dn_ld]
    int T, period, dn_ld;
};
__global__ __launch_bounds__(256) void disc_post_kernel(const PostParams p) {
    const int seq = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = p.lens[seq];
    if (t >= n) return;
    const float* xb = p.x + (size_t)seq * p.T * 1024;
    float acc = 0.f;
    for (int k = 0; k < 3; ++k) {
        const int r = t + k - 1;
        if (r < 0 || r >= n) continue;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int c = m * 256 + lane * 4;
            const f32x4 v = *(const f32x4*)(xb + (size_t)r * 1024 + c);
            const f32x4 wv = *(const f32x4*)(p.w + k * 1024 + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(wv[e], lrelu(v[e]), acc);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
        const int s = seq / p.period, j = seq - s * p.period;
        p.dws[(size_t)s * p.dn_ld + (size_t)t * p.period + j] = acc + p.bias;
    }
}

// fixed tree over the workgroup's 256 fp64 values per slot
template <int NS>
__device__ __forceinline__ void block_tree(double (&v)[NS], double* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NS; ++q) red[q * DISC_THREADS + tid] = v[q];
    __syncthreads();
    for (int w = DISC_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int q = 0; q < NS; ++q) red[q * DISC_THREADS + tid] += red[q * DISC_THREADS + tid + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) v[q] = red[q * DISC_THREADS];
}

// ---- the sums of one discriminator, a workgroup per utterance
struct ScoreParams {
    const float* dws;        // [2B][dn_ld]
    const int* lens;         // [nseq]: rows of conv_post per sequence (equal for the columns of one signal)
    double* sums;            // + b * 8 * 4: this discriminator's four sums
    long long* counts;       // + b * 8
    double* fm;              // + b * 8 * 8: the conv_post map's entry, or null
    long long* fm_counts;
    float *d_real, *d_gen;   // + b * d_ld, or null
    int B, period, dn_ld, d_ld;
};
__global__ __launch_bounds__(DISC_THREADS) void disc_score_kernel(const ScoreParams p) {
    __shared__ double red[5 * DISC_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = p.lens[(size_t)b * p.period] * p.period;
    const float* dr = p.dws + (size_t)b * p.dn_ld;
    const float* dg = p.dws + (size_t)(p.B + b) * p.dn_ld;
    double v[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < n; i += DISC_THREADS) {
        const double r = (double)dr[i], g = (double)dg[i];
        v[0] += (1.0 - r) * (1.0 - r);
        v[1] += r * r;
        v[2] += (1.0 - g) * (1.0 - g);
        v[3] += g * g;
        v[4] += fabs(r - g);
        if (p.d_real) {
            p.d_real[(size_t)b * p.d_ld + i] = dr[i];
            p.d_gen[(size_t)b * p.d_ld + i] = dg[i];
        }
    }
    block_tree<5>(v, red);
    if (tid == 0) {
        for (int q = 0; q < 4; ++q) p.sums[(size_t)b * 32 + q] = v[q];
        p.counts[(size_t)b * 8] = n;
        if (p.fm) {
            p.fm[(size_t)b * 64] = v[4];
            p.fm_counts[(size_t)b * 64] = n;
        }
    }
}

// ---- feature sums of one layer: sum |lrelu(a) - lrelu(b)| over the valid rows of a sequence pair, tile by tile, then the tiles in order
struct FmParams {
    const float* x;          // [nseq][T][C] pre-activation
    const int* lens;         // [nseq]
    double* part;            // [B * period][ntile]
    double* fm;              // + b * 64: this (discriminator, layer)'s entry
    long long* fm_counts;
    int B, period, T, C, ntile;
};
__global__ __launch_bounds__(DISC_THREADS) void disc_fm_kernel(const FmParams p) {
    __shared__ double red[DISC_THREADS];
    const int q = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;   // q = b * period + j
    const long long n = (long long)p.lens[q] * p.C;
    const long long e0 = (long long)tile * DISC_FM_TILE;
    if (e0 >= n) return;
    const float* a = p.x + (size_t)q * p.T * p.C;
    const float* g = p.x + (size_t)(p.B * p.period + q) * p.T * p.C;
    double v[1] = {0};
#pragma unroll
    for (int m = 0; m < DISC_FM_TILE / (4 * DISC_THREADS); ++m) {
        const long long e = e0 + (long long)(m * DISC_THREADS + tid) * 4;
        if (e >= n) continue;   // (C is a multiple of 4: a piece is valid as a whole)
        const f32x4 va = *(const f32x4*)(a + e), vg = *(const f32x4*)(g + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[0] += fabs((double)lrelu(va[k]) - (double)lrelu(vg[k]));
    }
    block_tree<1>(v, red);
    if (tid == 0) p.part[(size_t)q * p.ntile + tile] = v[0];
}
__global__ __launch_bounds__(DISC_THREADS) void disc_fm_reduce_kernel(const FmParams p) {
    __shared__ double red[DISC_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long n = (long long)p.lens[(size_t)b * p.period] * p.C;       // per column (the columns of one signal have equal rows)
    const int nt = (int)((n + DISC_FM_TILE - 1) / DISC_FM_TILE);
    double v[1] = {0};
    for (int i = tid; i < nt * p.period; i += DISC_THREADS) {
        const int j = i / nt, tile = i - j * nt;
        v[0] += p.part[(size_t)(b * p.period + j) * p.ntile + tile];
    }
    block_tree<1>(v, red);
    if (tid == 0) {
        p.fm[(size_t)b * 64] = v[0];
        p.fm_counts[(size_t)b * 64] = n * p.period;
    }
}

// =====================================================================================================================================
// weights
namespace {

bool shape_is(const HostTensor* t, std::initializer_list<int64_t> want) {
    // Conv2d weights carry a trailing 1; accept it or its absence
    std::vector<int64_t> s = t->shape;
    while (s.size() > want.size() && s.back() == 1) s.pop_back();
    return s == std::vector<int64_t>(want);
}

std::string shape_str(const HostTensor* t) {
    std::string s = "[";
    for (size_t i = 0; i < t->shape.size(); ++i) s += (i ? ", " : "") + std::to_string((long long)t->shape[i]);
    return s + "]";
}

// <base>.weight of shape [co][ci][k] (+ a trailing 1) and <base>.bias [co], or null after recording the failure in rc
const HostTensor* disc_tensor(dtts_ctx* h, Need& need, const std::string& base, int co, int ci, int k, const HostTensor** bias, int* rc) {
    const HostTensor* w = need.get(base + ".weight");
    const HostTensor* b = need.get(base + ".bias");
    if (!w || !b) return nullptr;
    if (!shape_is(w, {co, ci, k}) || b->numel() != co) {
        *rc = fail(h, DTTS_E_INVAL, "dtts_finalize_weights(DTTS_PART_DISC): %s.weight is %s with %lld bias entries; the reference's layer is [%d, %d, %d]",
                   base.c_str(), shape_str(w).c_str(), (long long)b->numel(), co, ci, k);
        return nullptr;
    }
    *bias = b;
    return w;
}

bool pack_dense(dtts_ctx* h, Need& need, PackedConv& L, const std::string& base, int co, int ci, int k, int stride, int* rc) {
    const HostTensor* b = nullptr;
    const HostTensor* w = disc_tensor(h, need, base, co, ci, k, &b, rc);
    if (!w) return false;
    const float* pw = w->f.data();
    if (!pack_conv(h, L, ENG_F32, co, ci, k, [=](int o, int i, int tap) { return pw[((size_t)o * ci + i) * k + tap]; }, b->f, 1, stride, k / 2)) {
        *rc = fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_DISC): packing %s", base.c_str());
        return false;
    }
    return true;
}

bool pack_grouped(dtts_ctx* h, Need& need, GroupedConv& G, const std::string& base, int co, int ci, int groups, int stride, int* rc) {
    const HostTensor* b = nullptr;
    const int cig = ci / groups, cog = co / groups;
    const HostTensor* w = disc_tensor(h, need, base, co, cig, GCONV_K, &b, rc);
    if (!w) return false;
    G.C_in = ci;
    G.C_out = co;
    G.groups = groups;
    G.stride = stride;
    G.cig = cig;
    G.cog = cog;
    G.ntg = (cog + 31) / 32;
    G.nq = GCONV_K * cig / 8;
    std::vector<float> pk((size_t)groups * G.ntg * G.nq * 64 * 4, 0.f);
    for (int g = 0; g < groups; ++g)
        for (int n = 0; n < G.ntg; ++n)
            for (int Q = 0; Q < G.nq; ++Q)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 4; ++e) {
                        const int c = n * 32 + (l & 31), kk = 8 * Q + 4 * (l >> 5) + e;
                        if (c >= cog) continue;
                        const int tap = kk / cig, i = kk % cig;
                        pk[((((size_t)g * G.ntg + n) * G.nq + Q) * 64 + l) * 4 + e] = w->f[((size_t)(g * cog + c) * cig + i) * GCONV_K + tap];
                    }
    G.w = upload(h, pk);
    G.bias = upload(h, b->f);
    G.hw = w->f;
    G.hb = b->f;
    if (!G.w || !G.bias) {
        *rc = fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_DISC): packing %s", base.c_str());
        return false;
    }
    return true;
}

// conv_post [1][1024][3] -> [3][1024]
bool pack_post(dtts_ctx* h, Need& need, float** wp, float* bp, const std::string& base, int* rc) {
    const HostTensor* b = nullptr;
    const HostTensor* w = disc_tensor(h, need, base, 1, 1024, 3, &b, rc);
    if (!w) return false;
    std::vector<float> t(3 * 1024);
    for (int c = 0; c < 1024; ++c)
        for (int k = 0; k < 3; ++k) t[(size_t)k * 1024 + c] = w->f[(size_t)c * 3 + k];
    *wp = upload(h, t);
    *bp = b->f[0];
    if (!*wp) {
        *rc = fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_DISC): packing %s", base.c_str());
        return false;
    }
    return true;
}

bool pack_entry(dtts_ctx* h, Need& need, float** wp, float** bp, const std::string& base, int co, int k, bool transposed, int* rc) {
    const HostTensor* b = nullptr;
    const HostTensor* w = disc_tensor(h, need, base, co, 1, k, &b, rc);
    if (!w) return false;
    std::vector<float> t(w->f);
    if (transposed)   // [co][k] -> [k][co]
        for (int c = 0; c < co; ++c)
            for (int q = 0; q < k; ++q) t[(size_t)q * co + c] = w->f[(size_t)c * k + q];
    *wp = upload(h, t);
    *bp = upload(h, b->f);
    if (!*wp || !*bp) {
        *rc = fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_DISC): packing %s", base.c_str());
        return false;
    }
    return true;
}

constexpr int MPD_CH[6] = {1, 32, 128, 512, 1024, 1024};
constexpr int MSD_CH[8] = {1, 128, 128, 256, 512, 1024, 1024, 1024};
constexpr int MSD_GROUPS[5] = {4, 16, 16, 16, 16};
constexpr int MSD_STRIDE[5] = {2, 2, 4, 4, 1};

} // namespace

int build_disc(dtts_ctx* h) {
    Need need{h};
    int rc = DTTS_OK;
    auto done = [&]() {
        if (rc != DTTS_OK) return rc;
        return fail(h, DTTS_E_NOENT, "dtts_finalize_weights(DTTS_PART_DISC): missing tensor %s", need.missing.c_str());
    };
    for (int i = 0; i < 5; ++i) {
        const std::string d = "disc.mpd." + std::to_string(i);
        DiscMpd& m = h->mpd[i];
        if (!pack_entry(h, need, &m.w0, &m.b0, d + ".convs.0", 32, 5, false, &rc)) return done();
        for (int j = 1; j < 5; ++j)
            if (!pack_dense(h, need, m.conv[j - 1], d + ".convs." + std::to_string(j), MPD_CH[j + 1], MPD_CH[j], 5, j < 4 ? 3 : 1, &rc)) return done();
        if (!pack_post(h, need, &m.wpost, &m.bpost, d + ".conv_post", &rc)) return done();
    }
    for (int i = 0; i < 3; ++i) {
        const std::string d = "disc.msd." + std::to_string(i);
        DiscMsd& m = h->msd[i];
        if (!pack_entry(h, need, &m.w0, &m.b0, d + ".convs.0", 128, 15, true, &rc)) return done();
        for (int j = 1; j < 6; ++j)
            if (!pack_grouped(h, need, m.g[j - 1], d + ".convs." + std::to_string(j), MSD_CH[j + 1], MSD_CH[j], MSD_GROUPS[j - 1], MSD_STRIDE[j - 1], &rc))
                return done();
        if (!pack_dense(h, need, m.c6, d + ".convs.6", 1024, 1024, 5, 1, &rc)) return done();
        if (!pack_post(h, need, &m.wpost, &m.bpost, d + ".conv_post", &rc)) return done();
    }
    h->disc_ready = true;
    return DTTS_OK;
}

// =====================================================================================================================================
// forward
namespace {

DiscChain mpd_chain() {
    DiscChain c{};
    c.n = DISC_MPD_LAYERS;
    for (int l = 0; l < 6; ++l) {
        c.k[l] = l < 5 ? 5 : 3;
        c.s[l] = l < 4 ? 3 : 1;
        c.pad[l] = l < 5 ? 2 : 1;
    }
    return c;
}
DiscChain msd_chain() {
    DiscChain c{};
    c.n = DISC_MSD_LAYERS;
    const int k[8] = {15, 41, 41, 41, 41, 41, 5, 3}, s[8] = {1, 2, 2, 4, 4, 1, 1, 1};
    for (int l = 0; l < 8; ++l) {
        c.k[l] = k[l];
        c.s[l] = s[l];
        c.pad[l] = k[l] / 2;
    }
    return c;
}

// the largest row counts a wav_ld-sample utterance gives: rows[0] = input rows, rows[l + 1] = after layer l (the chain is monotone in L)
void chain_rows(const DiscChain& c, int wav_ld, int period, int pools, int* rows) {
    int r = (wav_ld + period - 1) / period;
    for (int q = 0; q < pools; ++q) r = r / 2;
    rows[0] = r;
    for (int l = 0; l < c.n; ++l) rows[l + 1] = r = disc_conv_rows(r, c.k[l], c.s[l], c.pad[l]);
}

struct DiscPlan {
    size_t act[2] = {0, 0};   // floats of the two activation buffers per utterance pair (layers alternate between them)
    size_t part = 0;          // fp64 partial feature sums per utterance pair
    size_t dn = 0;            // D outputs per signal
    size_t pool1 = 0, pool2 = 0;
};

DiscPlan disc_plan(int wav_ld, int which) {
    DiscPlan pl;
    int rows[9];
    auto layer = [&](int l, int period, int C) {
        const size_t fl = (size_t)2 * period * rows[l + 1] * C;
        pl.act[l & 1] = std::max(pl.act[l & 1], fl);
        pl.part = std::max(pl.part, (size_t)period * (((size_t)rows[l + 1] * C + DISC_FM_TILE - 1) / DISC_FM_TILE));
    };
    if (which & DTTS_DISC_MPD)
        for (int i = 0; i < 5; ++i) {
            chain_rows(mpd_chain(), wav_ld, DISC_PERIODS[i], 0, rows);
            for (int l = 0; l < 5; ++l) layer(l, DISC_PERIODS[i], MPD_CH[l + 1]);
            pl.dn = std::max(pl.dn, (size_t)rows[6] * DISC_PERIODS[i]);
        }
    if (which & DTTS_DISC_MSD)
        for (int i = 0; i < 3; ++i) {
            chain_rows(msd_chain(), wav_ld, 1, i, rows);
            for (int l = 0; l < 7; ++l) layer(l, 1, MSD_CH[l + 1]);
            pl.dn = std::max(pl.dn, (size_t)rows[8]);
        }
    pl.pool1 = (size_t)2 * std::max(1, wav_ld / 2);
    pl.pool2 = (size_t)2 * std::max(1, wav_ld / 4);
    return pl;
}

size_t plan_bytes(const DiscPlan& pl, int Bc) {
    const size_t tab = (size_t)9 * 2 * Bc * DISC_MAX_P * sizeof(int) + (size_t)Bc * sizeof(int);
    return ((pl.act[0] + pl.act[1] + 2 * pl.dn + pl.pool1 + pl.pool2) * sizeof(float) + pl.part * sizeof(double)) * Bc + tab + 16 * 256;
}

} // namespace

// h may be null: the block is checked first, so that the refusals are reachable without a device
int disc_forward(dtts_ctx* h, const dtts_disc_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_DISC)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B < 1 || a->B > 65535) return fail(h, DTTS_E_INVAL, "%s: B = %d (supported: 1 .. 65535)", me, a->B);
    if (a->wav_ld < DTTS_DISC_MIN_LEN)
        return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples is below DTTS_DISC_MIN_LEN = %d, the shortest waveform the reference's discriminators accept", me,
                    a->wav_ld, DTTS_DISC_MIN_LEN);
    if (a->wav_ld > (1 << 24)) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: %d .. %d)", me, a->wav_ld, DTTS_DISC_MIN_LEN, 1 << 24);
    if (!(a->which & (DTTS_DISC_MPD | DTTS_DISC_MSD)) || (a->which & ~(DTTS_DISC_MPD | DTTS_DISC_MSD | DTTS_DISC_FM | DTTS_DISC_DENSE_GROUPED)))
        return fail(h, DTTS_E_INVAL, "%s: which = %d (DTTS_DISC_MPD = 1 and / or DTTS_DISC_MSD = 2, optionally DTTS_DISC_FM = 4, DTTS_DISC_DENSE_GROUPED = 8)", me,
                    a->which);
    if (a->reserved != 0) return fail(h, DTTS_E_INVAL, "%s: reserved = %d (must be 0)", me, a->reserved);
    if (!a->y_dev || !a->y_hat_dev || !a->sums_dev || !a->counts_dev || !a->status_dev)
        return fail(h, DTTS_E_INVAL, "%s: null y_dev / y_hat_dev / sums_dev / counts_dev / status_dev", me);
    const bool fm = (a->which & DTTS_DISC_FM) != 0;
    if (fm && (!a->fm_dev || !a->fm_counts_dev)) return fail(h, DTTS_E_INVAL, "%s: DTTS_DISC_FM without fm_dev / fm_counts_dev", me);
    const int d_need = (a->wav_ld + 63) / 64 + 16;
    if (a->d_dev && a->d_ld < d_need) return fail(h, DTTS_E_INVAL, "%s: d_ld = %d entries for wav_ld = %d (needs %d)", me, a->d_ld, a->wav_ld, d_need);
    if (int rc = blk.aligned(4, {{"y_dev", a->y_dev}, {"y_hat_dev", a->y_hat_dev}, {"lens_dev", a->lens_dev}, {"d_dev", a->d_dev}, {"status_dev", a->status_dev}}))
        return rc;
    if (int rc = blk.aligned(8, {{"sums_dev", a->sums_dev}, {"counts_dev", a->counts_dev}, {"fm_dev", a->fm_dev}, {"fm_counts_dev", a->fm_counts_dev}})) return rc;
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_DISC)) return rc;

    // measurement aid: the grouped layers as block-diagonal dense layers on conv1d_launch, packed here on first use (a host-side pack and
    // upload: this call synchronises)
    const bool dense_grouped = (a->which & DTTS_DISC_DENSE_GROUPED) && (a->which & DTTS_DISC_MSD);
    if (dense_grouped)
        for (int i = 0; i < 3; ++i) {
            DiscMsd& m = h->msd[i];
            if (m.gd_ready) continue;
            for (int l = 0; l < 5; ++l) {
                const GroupedConv& G = m.g[l];
                const float* pw = G.hw.data();
                const int cig = G.cig, cog = G.cog;
                if (!pack_conv(h, m.gd[l], ENG_F32, G.C_out, G.C_in, GCONV_K,
                               [=](int o, int c, int tap) { return c / cig == o / cog ? pw[((size_t)o * cig + c % cig) * GCONV_K + tap] : 0.f; }, G.hb, 1,
                               G.stride, GCONV_PAD))
                    return fail(h, DTTS_E_NOMEM, "%s: packing the dense form of msd.%d.convs.%d", me, i, l + 1);
            }
            m.gd_ready = true;
        }

    const int ld = a->wav_ld;
    const DiscPlan pl = disc_plan(ld, a->which);
    const int Bc = chunk_within(std::min(a->B, 65535 / (2 * DISC_MAX_P)), DTTS_DISC_WS_BYTES, [&](int n) { return plan_bytes(pl, n); });
    HIPCHK(h->a_disc.reserve(plan_bytes(pl, Bc), stream));

    for (int b0 = 0; b0 < a->B; b0 += Bc) {
        const int B = std::min(Bc, a->B - b0);
        Arena& ws = h->a_disc;
        ws.rewind();
        int* vlen = ws.alloc<int>((size_t)B);
        int* tab = ws.alloc<int>((size_t)9 * 2 * B * DISC_MAX_P);
        float* act[2] = {ws.alloc<float>(pl.act[0] * B), ws.alloc<float>(pl.act[1] * B)};
        float* dws = ws.alloc<float>(2 * pl.dn * B);
        double* part = fm ? ws.alloc<double>(pl.part * B) : nullptr;
        float* pool1 = (a->which & DTTS_DISC_MSD) ? ws.alloc<float>(pl.pool1 * B) : nullptr;
        float* pool2 = (a->which & DTTS_DISC_MSD) ? ws.alloc<float>(pl.pool2 * B) : nullptr;
        if (!vlen || !tab || !act[0] || !act[1] || !dws || (fm && !part) || ((a->which & DTTS_DISC_MSD) && (!pool1 || !pool2)))
            return blk.workspace();
        const float* y = a->y_dev + (size_t)b0 * ld;
        const float* yh = a->y_hat_dev + (size_t)b0 * ld;
        hipLaunchKernelGGL(disc_vlen_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, a->lens_dev ? a->lens_dev + b0 : nullptr, B, ld, vlen,
                           a->status_dev + b0);
        LAUNCH(hipGetLastError());

        // what follows every layer of discriminator d: its feature sums (layer l's output x [nseq][T][C])
        auto feature = [&](int d, int l, const float* x, const int* lens, int period, int T, int C) -> int {
            if (!fm) return DTTS_OK;
            FmParams f{};
            f.x = x;
            f.lens = lens;
            f.part = part;
            f.fm = a->fm_dev + ((size_t)b0 * 8 + d) * 8 + l;
            f.fm_counts = (long long*)a->fm_counts_dev + ((size_t)b0 * 8 + d) * 8 + l;
            f.B = B;
            f.period = period;
            f.T = T;
            f.C = C;
            f.ntile = (int)(((size_t)T * C + DISC_FM_TILE - 1) / DISC_FM_TILE);
            hipLaunchKernelGGL(disc_fm_kernel, dim3((unsigned)f.ntile, (unsigned)(B * period)), dim3(DISC_THREADS), 0, stream, f);
            LAUNCH(hipGetLastError());
            hipLaunchKernelGGL(disc_fm_reduce_kernel, dim3((unsigned)B), dim3(DISC_THREADS), 0, stream, f);
            LAUNCH(hipGetLastError());
            return DTTS_OK;
        };
        auto dense = [&](const PackedConv& L, const float* x, float* yo, int nseq, int T_in, int T_out, const int* in_lens, const int* out_lens) -> int {
            ConvParams p = base_params(x, L.C_in, nseq, T_in, T_out, yo, L.C_out);
            p.in_lens = in_lens;
            p.out_lens = out_lens;
            p.pre_act = 1;
            p.pre_slope = DISC_SLOPE;
            p.fixed_order = 1;
            LAUNCH(conv1d_launch(L, p, stream));
            return DTTS_OK;
        };
        // conv_post + the sums
        auto finish = [&](int d, const float* x, const int* lens, int period, int T, const float* wpost, float bpost, int n_maps) -> int {
            PostParams q{};
            q.x = x;
            q.lens = lens;
            q.w = wpost;
            q.bias = bpost;
            q.dws = dws;
            q.T = T;
            q.period = period;
            q.dn_ld = (int)pl.dn;
            hipLaunchKernelGGL(disc_post_kernel, dim3((unsigned)((T + 3) / 4), (unsigned)(2 * B * period)), dim3(256), 0, stream, q);
            LAUNCH(hipGetLastError());
            ScoreParams s{};
            s.dws = dws;
            s.lens = lens;
            s.sums = a->sums_dev + ((size_t)b0 * 8 + d) * 4;
            s.counts = (long long*)a->counts_dev + (size_t)b0 * 8 + d;
            s.fm = fm ? a->fm_dev + ((size_t)b0 * 8 + d) * 8 + (n_maps - 1) : nullptr;
            s.fm_counts = fm ? (long long*)a->fm_counts_dev + ((size_t)b0 * 8 + d) * 8 + (n_maps - 1) : nullptr;
            s.d_real = a->d_dev ? a->d_dev + (((size_t)d * 2 + 0) * a->B + b0) * a->d_ld : nullptr;
            s.d_gen = a->d_dev ? a->d_dev + (((size_t)d * 2 + 1) * a->B + b0) * a->d_ld : nullptr;
            s.B = B;
            s.period = period;
            s.dn_ld = (int)pl.dn;
            s.d_ld = a->d_ld;
            hipLaunchKernelGGL(disc_score_kernel, dim3((unsigned)B), dim3(DISC_THREADS), 0, stream, s);
            LAUNCH(hipGetLastError());
            return DTTS_OK;
        };

        int rows[9], rc;
        if (a->which & DTTS_DISC_MPD)
            for (int i = 0; i < 5; ++i) {
                const int P = DISC_PERIODS[i], nseq = 2 * B * P;
                const DiscMpd& m = h->mpd[i];
                const DiscChain ch = mpd_chain();
                chain_rows(ch, ld, P, 0, rows);
                hipLaunchKernelGGL(disc_rows_kernel, dim3((nseq + 255) / 256), dim3(256), 0, stream, vlen, B, P, 0, ch, tab, nseq);
                LAUNCH(hipGetLastError());
                auto lens = [&](int l) { return tab + (size_t)l * nseq; };
                MpdEntryParams e{};
                e.y = y;
                e.yh = yh;
                e.vlen = vlen;
                e.in_rows = lens(0);
                e.out_lens = lens(1);
                e.w = m.w0;
                e.bias = m.b0;
                e.out = act[0];
                e.B = B;
                e.wav_ld = ld;
                e.period = P;
                e.T_out = rows[1];
                hipLaunchKernelGGL(disc_mpd_entry_kernel, dim3((unsigned)(((size_t)rows[1] * 32 + 255) / 256), (unsigned)nseq), dim3(256), 0, stream, e);
                LAUNCH(hipGetLastError());
                if ((rc = feature(i, 0, act[0], lens(1), P, rows[1], 32)) != DTTS_OK) return rc;
                for (int l = 1; l < 5; ++l) {
                    if ((rc = dense(m.conv[l - 1], act[(l - 1) & 1], act[l & 1], nseq, rows[l], rows[l + 1], lens(l), lens(l + 1))) != DTTS_OK) return rc;
                    if ((rc = feature(i, l, act[l & 1], lens(l + 1), P, rows[l + 1], MPD_CH[l + 1])) != DTTS_OK) return rc;
                }
                if ((rc = finish(i, act[0], lens(5), P, rows[5], m.wpost, m.bpost, DISC_MPD_LAYERS)) != DTTS_OK) return rc;
            }
        if (a->which & DTTS_DISC_MSD) {
            const dim3 pg1((unsigned)((std::max(1, ld / 2) + 255) / 256), (unsigned)(2 * B)), pg2((unsigned)((std::max(1, ld / 4) + 255) / 256), (unsigned)(2 * B));
            const int ld1 = std::max(1, ld / 2), ld2 = std::max(1, ld / 4);
            hipLaunchKernelGGL(disc_pool_kernel, pg1, dim3(256), 0, stream, y, yh, ld, vlen, B, 0, pool1, ld1);
            LAUNCH(hipGetLastError());
            hipLaunchKernelGGL(disc_pool_kernel, pg2, dim3(256), 0, stream, (const float*)pool1, (const float*)(pool1 + (size_t)B * ld1), ld1, vlen, B, 1, pool2, ld2);
            LAUNCH(hipGetLastError());
            for (int i = 0; i < 3; ++i) {
                const int d = 5 + i, nseq = 2 * B;
                const DiscMsd& m = h->msd[i];
                const DiscChain ch = msd_chain();
                chain_rows(ch, ld, 1, i, rows);
                hipLaunchKernelGGL(disc_rows_kernel, dim3((nseq + 255) / 256), dim3(256), 0, stream, vlen, B, 1, i, ch, tab, nseq);
                LAUNCH(hipGetLastError());
                auto lens = [&](int l) { return tab + (size_t)l * nseq; };
                MsdEntryParams e{};
                e.x0 = i == 0 ? y : (i == 1 ? pool1 : pool2);
                e.x1 = i == 0 ? yh : (i == 1 ? pool1 + (size_t)B * ld1 : pool2 + (size_t)B * ld2);
                e.ld = i == 0 ? ld : (i == 1 ? ld1 : ld2);
                e.lens = lens(1);
                e.w = m.w0;
                e.bias = m.b0;
                e.out = act[0];
                e.B = B;
                e.T = rows[1];
                hipLaunchKernelGGL(disc_msd_entry_kernel, dim3((unsigned)((rows[1] + 2 * MSD_ENTRY_ROWS - 1) / (2 * MSD_ENTRY_ROWS)), (unsigned)nseq), dim3(256), 0, stream, e);
                LAUNCH(hipGetLastError());
                if ((rc = feature(d, 0, act[0], lens(1), 1, rows[1], 128)) != DTTS_OK) return rc;
                for (int l = 1; l < 6; ++l) {
                    const GroupedConv& G = m.g[l - 1];
                    if (dense_grouped) {
                        if ((rc = dense(m.gd[l - 1], act[(l - 1) & 1], act[l & 1], nseq, rows[l], rows[l + 1], lens(l), lens(l + 1))) != DTTS_OK) return rc;
                        if ((rc = feature(d, l, act[l & 1], lens(l + 1), 1, rows[l + 1], G.C_out)) != DTTS_OK) return rc;
                        continue;
                    }
                    GConvParams q{};
                    q.x = act[(l - 1) & 1];
                    q.y = act[l & 1];
                    q.w = G.w;
                    q.bias = G.bias;
                    q.in_lens = lens(l);
                    q.out_lens = lens(l + 1);
                    q.nseq = nseq;
                    q.T_in = rows[l];
                    q.T_out = rows[l + 1];
                    q.C_in = G.C_in;
                    q.C_out = G.C_out;
                    q.cig = G.cig;
                    q.cig_shift = __builtin_ctz((unsigned)G.cig);
                    q.cog = G.cog;
                    q.ntg = G.ntg;
                    q.nq = G.nq;
                    q.stride = G.stride;
                    q.slope = DISC_SLOPE;
                    LAUNCH(gconv_launch(q, stream));
                    if ((rc = feature(d, l, act[l & 1], lens(l + 1), 1, rows[l + 1], G.C_out)) != DTTS_OK) return rc;
                }
                if ((rc = dense(m.c6, act[1], act[0], nseq, rows[6], rows[7], lens(6), lens(7))) != DTTS_OK) return rc;
                if ((rc = feature(d, 6, act[0], lens(7), 1, rows[7], 1024)) != DTTS_OK) return rc;
                if ((rc = finish(d, act[0], lens(7), 1, rows[7], m.wpost, m.bpost, DISC_MSD_LAYERS)) != DTTS_OK) return rc;
            }
        }
    }
    return DTTS_OK;
}

} // namespace dtts
