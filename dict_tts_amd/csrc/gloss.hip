// libdicttts_hip.so — the gloss encoder (gloss.h; dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)): what the reference's binariser computes with
// pretrained/roformer-chinese-base for every dictionary gloss (data_gen/tts/binarizer_zh.py: get_encodings), on a ragged batch of glosses.
// Per call: the embedding stage, then per layer the fused q | k | v projection, the rotary attention, the output projection + residual,
// LayerNorm, the GELU feed-forward pair + residual and the LayerNorm that also keeps the running sum of the hidden states; the last one
// writes the mean.  Nothing but the offsets goes through the host (they are validated before the first launch).
#include "ctx.h"

namespace dtts {

typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

__device__ __forceinline__ float gl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// mean and 1 / sqrt(var + eps) of row xr as layernorm_kernel (ops.hip) computes them: lane-strided partial sums, the xor tree, two passes
__device__ __forceinline__ void gl_row_stats(const float* xr, int C, int lane, float eps, float* mean, float* inv) {
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += xr[c];
    const float m = gl_wave_sum(sum) / (float)C;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = xr[c] - m;
        sq += d * d;
    }
    *mean = m;
    *inv = 1.0f / sqrtf(gl_wave_sum(sq) / (float)C + eps);
}

// ---- the embedding stage: one wave per row
__global__ __launch_bounds__(256) void gloss_embed_kernel(const int64_t* ids, const float* table, int vocab, const float* tt0, const float* gamma,
                                                          const float* beta, float eps, float* x, float* acc, int64_t* status, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row < rows) {
        const long long id = ids[row];
        const bool ok = id >= 0 && id < vocab;
        const float* er = table + (ok ? id : 0) * (long long)C;
        float* xr = x + (long long)row * C;
        float* ar = acc + (long long)row * C;
        for (int c = lane; c < C; c += 64) {
            const float e = ok ? er[c] : 0.f;
            ar[c] = e;
            xr[c] = e + tt0[c];
        }
        float mean, inv;
        gl_row_stats(xr, C, lane, eps, &mean, &inv);
        for (int c = lane; c < C; c += 64) {
            const float y = (xr[c] - mean) * inv * gamma[c] + beta[c];
            xr[c] = y;
            ar[c] += y;
        }
    }
    if (blockIdx.x != 0) return;
    // workgroup 0 names the FIRST offending row: every thread's lowest, then a fixed tree (no atomics)
    __shared__ int first[256];
    int mine = INT_MAX;
    for (int r = threadIdx.x; r < rows; r += 256)
        if (ids[r] < 0 || ids[r] >= vocab) {
            mine = r;
            break;
        }
    first[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) first[threadIdx.x] = min(first[threadIdx.x], first[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int f = first[0];
        status[0] = f == INT_MAX ? 0 : (int64_t)f + 1;
        status[1] = f == INT_MAX ? 0 : ids[f];
    }
}

// ---- x = LN(x) in place, acc += x (or out = acc / div): one wave per row
__global__ __launch_bounds__(256) void gloss_ln_acc_kernel(float* x, const float* gamma, const float* beta, float eps, float* acc, float* out, float div,
                                                           int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* xr = x + (long long)row * C;
    float* ar = acc + (long long)row * C;
    float mean, inv;
    gl_row_stats(xr, C, lane, eps, &mean, &inv);
    for (int c = lane; c < C; c += 64) {
        const float y = (xr[c] - mean) * inv * gamma[c] + beta[c];
        xr[c] = y;
        const float sum = ar[c] + y;
        if (out) out[(long long)row * C + c] = sum / div;
        else ar[c] = sum;
    }
}

// ---- the rotary self-attention: one workgroup per gloss, its heads four at a time, one head per wave, one query row per lane.
// Every 1 KB a wave instruction moves is contiguous in a qkv (or ctx) row: piece (row, head of the group, 16 bytes of its 64 channels).
// Per group of heads: q' -> tile A (rotated while staged), each lane takes its own row into registers; k' -> A, v -> B; the lane walks the
// gloss's keys twice in key order (the maximum, then exp, the sum and P v; a key's row is one LDS broadcast); ctx / sum goes back through
// A so that the stores are the same contiguous pieces.  LDS: rot [L_ld][32] (sin, cos), then per wave A [L_ld][GLOSS_QLD], B [L_ld][64].
__device__ __forceinline__ float gl_dot64(const f32x4 (&q)[16], const float* kr) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;   // four chains over the channels 4 f + e, joined (a0 + a1) + (a2 + a3)
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        const f32x4 k = *(const f32x4*)(kr + 4 * f);
        a0 = fmaf(q[f][0], k[0], a0);
        a1 = fmaf(q[f][1], k[1], a1);
        a2 = fmaf(q[f][2], k[2], a2);
        a3 = fmaf(q[f][3], k[3], a3);
    }
    return ((a0 + a1) + (a2 + a3)) * 0.125f;   // / sqrt(64): exact
}

__global__ __launch_bounds__(256) void gloss_attn_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, const int* __restrict__ tok_off,
                                                         const float2* __restrict__ rot, int C, int L_ld) {
    extern __shared__ f32x4 gloss_lds[];
    float* lds = (float*)gloss_lds;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = tok_off[blockIdx.x];
    int L = tok_off[blockIdx.x + 1] - r0;
    L = L < 0 ? 0 : (L > L_ld ? L_ld : L);   // (the host has checked the offsets: this only keeps the tiles' bounds whatever they hold)
    float2* rt = (float2*)lds;
    float* tiles = lds + (size_t)L_ld * 64;
    const int wave_ld = L_ld * (GLOSS_QLD + 64);
    float* Aw = tiles + (size_t)w * wave_ld;
    float* Bw = Aw + (size_t)L_ld * GLOSS_QLD;
    const int heads = C / GLOSS_DK, C3 = 3 * C;
    for (int i = tid; i < L * 32; i += 256) rt[i] = rot[i];
    const float* src = qkv + (size_t)r0 * C3;
    float* dst = ctx + (size_t)r0 * C;

    for (int h0 = 0; h0 < heads; h0 += 4) {
        const int nh = min(4, heads - h0), per_row = nh * 16, pieces = L * per_row;
        const bool mine = w < nh && lane < L;
        __syncthreads();   // the table is staged / the previous group's ctx tile has been stored
        for (int idx = tid; idx < pieces; idx += 256) {
            const int row = idx / per_row, rem = idx - row * per_row, hw = rem >> 4, f = rem & 15;
            const f32x4 t = *(const f32x4*)(src + (size_t)row * C3 + (h0 + hw) * GLOSS_DK + 4 * f);
            const float2 s0 = rt[row * 32 + 2 * f], s1 = rt[row * 32 + 2 * f + 1];
            f32x4 r;   // t cos + rot(t) sin, each product rounded as the reference's elementwise form rounds it
            r[0] = __fadd_rn(__fmul_rn(t[0], s0.y), __fmul_rn(-t[1], s0.x));
            r[1] = __fadd_rn(__fmul_rn(t[1], s0.y), __fmul_rn(t[0], s0.x));
            r[2] = __fadd_rn(__fmul_rn(t[2], s1.y), __fmul_rn(-t[3], s1.x));
            r[3] = __fadd_rn(__fmul_rn(t[3], s1.y), __fmul_rn(t[2], s1.x));
            *(f32x4*)(tiles + (size_t)hw * wave_ld + row * GLOSS_QLD + 4 * f) = r;
        }
        __syncthreads();
        f32x4 q[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) q[f] = mine ? *(const f32x4*)(Aw + lane * GLOSS_QLD + 4 * f) : (f32x4){0.f, 0.f, 0.f, 0.f};
        __syncthreads();   // every lane holds its q' row: A takes k'
        for (int idx = tid; idx < pieces; idx += 256) {
            const int row = idx / per_row, rem = idx - row * per_row, hw = rem >> 4, f = rem & 15;
            const float* at = src + (size_t)row * C3 + (h0 + hw) * GLOSS_DK + 4 * f;
            const f32x4 t = *(const f32x4*)(at + C), v = *(const f32x4*)(at + 2 * C);
            const float2 s0 = rt[row * 32 + 2 * f], s1 = rt[row * 32 + 2 * f + 1];
            f32x4 r;
            r[0] = __fadd_rn(__fmul_rn(t[0], s0.y), __fmul_rn(-t[1], s0.x));
            r[1] = __fadd_rn(__fmul_rn(t[1], s0.y), __fmul_rn(t[0], s0.x));
            r[2] = __fadd_rn(__fmul_rn(t[2], s1.y), __fmul_rn(-t[3], s1.x));
            r[3] = __fadd_rn(__fmul_rn(t[3], s1.y), __fmul_rn(t[2], s1.x));
            float* tw = tiles + (size_t)hw * wave_ld;
            *(f32x4*)(tw + row * GLOSS_QLD + 4 * f) = r;
            *(f32x4*)(tw + (size_t)L_ld * GLOSS_QLD + row * 64 + 4 * f) = v;
        }
        __syncthreads();
        f32x4 o[16];
#pragma unroll
        for (int f = 0; f < 16; ++f) o[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float l = 1.f;
        if (mine) {
            float m = -INFINITY;
            for (int j = 0; j < L; ++j) m = fmaxf(m, gl_dot64(q, Aw + j * GLOSS_QLD));
            l = 0.f;
            for (int j = 0; j < L; ++j) {
                const float p = expf(gl_dot64(q, Aw + j * GLOSS_QLD) - m);
                l += p;
                const float* vr = Bw + j * 64;
#pragma unroll
                for (int f = 0; f < 16; ++f) {
                    const f32x4 v = *(const f32x4*)(vr + 4 * f);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[f][e] = fmaf(p, v[e], o[f][e]);
                }
            }
        }
        __syncthreads();   // every lane has read k': A takes ctx
        if (mine) {
#pragma unroll
            for (int f = 0; f < 16; ++f) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = o[f][e] / l;
                *(f32x4*)(Aw + lane * GLOSS_QLD + 4 * f) = r;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < pieces; idx += 256) {
            const int row = idx / per_row, rem = idx - row * per_row, hw = rem >> 4, f = rem & 15;
            *(f32x4*)(dst + (size_t)row * C + (h0 + hw) * GLOSS_DK + 4 * f) = *(const f32x4*)(tiles + (size_t)hw * wave_ld + row * GLOSS_QLD + 4 * f);
        }
    }
}

} // namespace

hipError_t gloss_embed_launch(const int64_t* ids, const float* table, int vocab, const float* tt0, const float* gamma, const float* beta, float eps,
                              float* x, float* acc, int64_t* status, int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(gloss_embed_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ids, table, vocab, tt0, gamma, beta, eps, x, acc, status,
                       rows, C);
    return hipGetLastError();
}

hipError_t gloss_ln_acc_launch(float* x, const float* gamma, const float* beta, float eps, float* acc, float* out, float div, int rows, int C,
                               hipStream_t s) {
    hipLaunchKernelGGL(gloss_ln_acc_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, gamma, beta, eps, acc, out, div, rows, C);
    return hipGetLastError();
}

size_t gloss_attn_lds(int L_ld) { return (size_t)L_ld * (64 + 4 * (GLOSS_QLD + 64)) * sizeof(float); }

hipError_t gloss_attn_launch(const float* qkv, float* ctx, const int* tok_off, const float2* rot, int n_gloss, int C, int L_ld, hipStream_t s) {
    if (L_ld < 1 || L_ld > GLOSS_MAX_L || C % GLOSS_DK || n_gloss < 1) return hipErrorInvalidValue;
    static bool configured_dev[64] = {};   // per device: hipFuncSetAttribute is per device (the tiles of L_ld = 64 take 148 KB)
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    if (!configured_dev[cur_dev & 63]) {
        hipError_t e = hipFuncSetAttribute((const void*)gloss_attn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gloss_attn_lds(GLOSS_MAX_L));
        if (e != hipSuccess) return e;
        configured_dev[cur_dev & 63] = true;
    }
    hipLaunchKernelGGL(gloss_attn_kernel, dim3((unsigned)n_gloss), dim3(256), gloss_attn_lds(L_ld), s, qkv, ctx, tok_off, rot, C, L_ld);
    return hipGetLastError();
}

// =====================================================================================================================================
// weights
namespace {

std::string gl_shape(const std::vector<int64_t>& sh) {
    std::string s = "[";
    for (size_t i = 0; i < sh.size(); ++i) s += (i ? ", " : "") + std::to_string((long long)sh[i]);
    return s + "]";
}

const char* GL_ME = "dtts_finalize_weights(DTTS_PART_GLOSS)";

// the tensor `name` of exactly `want`, or null after recording why not.  missing_code: what a tensor that was never loaded returns
const HostTensor* gl_tensor(dtts_ctx* h, const std::string& name, const std::vector<int64_t>& want, int missing_code, int* rc) {
    auto it = h->w.find(name);
    if (it == h->w.end()) {
        *rc = fail(h, missing_code, "%s: missing tensor %s", GL_ME, name.c_str());
        return nullptr;
    }
    const HostTensor* t = &it->second;
    if (t->shape != want || t->f.size() != (size_t)t->numel()) {
        *rc = fail(h, DTTS_E_INVAL, "%s: %s is %s; the encoder's is %s", GL_ME, name.c_str(), gl_shape(t->shape).c_str(), gl_shape(want).c_str());
        return nullptr;
    }
    return t;
}

} // namespace

int build_gloss(dtts_ctx* h) {
    int rc = DTTS_OK;
    // "gloss.config" [4]: num_attention_heads, layer_norm_eps, rotary_value (0 / 1), hidden_act (0 = the erf GELU, anything else = another)
    const HostTensor* cfg = gl_tensor(h, "gloss.config", {4}, DTTS_E_NOENT, &rc);
    if (!cfg) return rc;
    const int heads = (int)cfg->f[0];
    const float eps = cfg->f[1];
    auto we_it = h->w.find("gloss.embeddings.word_embeddings.weight");
    if (we_it == h->w.end()) return fail(h, DTTS_E_NOENT, "%s: missing tensor gloss.embeddings.word_embeddings.weight", GL_ME);
    const HostTensor* we = &we_it->second;
    auto eg_it = h->w.find("gloss.embeddings.LayerNorm.weight");
    if (eg_it == h->w.end()) return fail(h, DTTS_E_NOENT, "%s: missing tensor gloss.embeddings.LayerNorm.weight", GL_ME);
    if (we->shape.size() != 2 || we->shape[0] < 1 || we->shape[0] > INT_MAX || we->f.size() != (size_t)we->numel())
        return fail(h, DTTS_E_INVAL, "%s: gloss.embeddings.word_embeddings.weight is %s; the encoder's is [vocab, hidden]", GL_ME, gl_shape(we->shape).c_str());
    const int64_t C64 = eg_it->second.numel(), E = we->shape[1];
    if (C64 < 64 || C64 > 8192 || C64 % 64)
        return fail(h, DTTS_E_INVAL, "%s: hidden_size = %lld (supported: a multiple of 64 up to 8192)", GL_ME, (long long)C64);
    const int C = (int)C64;
    if (heads < 1 || C % heads || C / heads != GLOSS_DK)
        return fail(h, DTTS_E_INVAL, "%s: hidden_size / num_attention_heads = %d / %d (supported: heads of %d channels)", GL_ME, C, heads, GLOSS_DK);
    if (E != C)
        return fail(h, DTTS_E_INVAL, "%s: embedding_size = %lld differs from hidden_size = %d (the reference's feature buffer assumes they are equal)", GL_ME,
                    (long long)E, C);
    if (cfg->f[2] != 0.f) return fail(h, DTTS_E_INVAL, "%s: rotary_value = true is not supported (the reference's checkpoint rotates q and k only)", GL_ME);
    if (cfg->f[3] != 0.f) return fail(h, DTTS_E_INVAL, "%s: hidden_act is not the erf GELU (\"gelu\"), the only activation supported", GL_ME);
    if (!(eps > 0.f) || !std::isfinite(eps)) return fail(h, DTTS_E_INVAL, "%s: layer_norm_eps = %g (must be positive)", GL_ME, (double)eps);

    int n_layers = 0;
    const std::string lp = "gloss.encoder.layer.";
    for (const auto& kv : h->w)
        if (kv.first.rfind(lp, 0) == 0) n_layers = std::max(n_layers, atoi(kv.first.c_str() + lp.size()) + 1);
    if (n_layers < 1 || n_layers > 64) return fail(h, DTTS_E_INVAL, "%s: %d encoder layers loaded (supported: 1 .. 64)", GL_ME, n_layers);

    auto tt_it = h->w.find("gloss.embeddings.token_type_embeddings.weight");   // [type_vocab_size][hidden]: row 0 is the one a gloss uses
    if (tt_it == h->w.end()) return fail(h, DTTS_E_NOENT, "%s: missing tensor gloss.embeddings.token_type_embeddings.weight", GL_ME);
    const HostTensor* tt = &tt_it->second;
    if (tt->shape.size() != 2 || tt->shape[0] < 1 || tt->shape[1] != C || tt->f.size() != (size_t)tt->numel())
        return fail(h, DTTS_E_INVAL, "%s: gloss.embeddings.token_type_embeddings.weight is %s; the encoder's is [type_vocab_size >= 1, %d]", GL_ME,
                    gl_shape(tt->shape).c_str(), C);
    const HostTensor* eg = gl_tensor(h, "gloss.embeddings.LayerNorm.weight", {C}, DTTS_E_NOENT, &rc);
    if (!eg) return rc;
    const HostTensor* eb = gl_tensor(h, "gloss.embeddings.LayerNorm.bias", {C}, DTTS_E_NOENT, &rc);
    if (!eb) return rc;

    auto nomem = [&](const std::string& what) { return fail(h, DTTS_E_NOMEM, "%s: packing %s", GL_ME, what.c_str()); };
    int F = 0;
    h->gloss_layers.assign(n_layers, GlossLayer());
    for (int l = 0; l < n_layers; ++l) {   // a loaded layer is complete, or the call names what it lacks (DTTS_E_INVAL)
        const std::string p = lp + std::to_string(l) + ".";
        GlossLayer& L = h->gloss_layers[l];
        const HostTensor *w3[3], *b3[3];
        const char* names[3] = {"query", "key", "value"};
        for (int i = 0; i < 3; ++i) {
            if (!(w3[i] = gl_tensor(h, p + "attention.self." + names[i] + ".weight", {C, C}, DTTS_E_INVAL, &rc))) return rc;
            if (!(b3[i] = gl_tensor(h, p + "attention.self." + names[i] + ".bias", {C}, DTTS_E_INVAL, &rc))) return rc;
        }
        const HostTensor* wo = gl_tensor(h, p + "attention.output.dense.weight", {C, C}, DTTS_E_INVAL, &rc);
        if (!wo) return rc;
        const HostTensor* bo = gl_tensor(h, p + "attention.output.dense.bias", {C}, DTTS_E_INVAL, &rc);
        if (!bo) return rc;
        const HostTensor* g1 = gl_tensor(h, p + "attention.output.LayerNorm.weight", {C}, DTTS_E_INVAL, &rc);
        if (!g1) return rc;
        const HostTensor* b1 = gl_tensor(h, p + "attention.output.LayerNorm.bias", {C}, DTTS_E_INVAL, &rc);
        if (!b1) return rc;
        auto wi_it = h->w.find(p + "intermediate.dense.weight");
        if (wi_it == h->w.end()) return fail(h, DTTS_E_INVAL, "%s: missing tensor %sintermediate.dense.weight", GL_ME, p.c_str());
        const int64_t Fl = wi_it->second.shape.size() == 2 ? wi_it->second.shape[0] : 0;
        if (Fl < 1 || Fl > 65536 || (l > 0 && Fl != F))
            return fail(h, DTTS_E_INVAL, "%s: %sintermediate.dense.weight is %s; the encoder's is [intermediate_size <= 65536, %d], one size for all layers", GL_ME,
                        p.c_str(), gl_shape(wi_it->second.shape).c_str(), C);
        // output.dense stages its input rows, whose pitch is intermediate_size floats, in 16-byte pieces (conv1d.hip: `ci < C_in` guards the
        // piece's FIRST channel): a size that is no multiple of 4 would misalign every other row's loads and read past the last row
        if (Fl % 4)
            return fail(h, DTTS_E_INVAL, "%s: intermediate_size = %lld (supported: a multiple of 4 up to 65536; the feed-forward rows are read in 16-byte pieces)",
                        GL_ME, (long long)Fl);
        F = (int)Fl;
        const HostTensor* wi = gl_tensor(h, p + "intermediate.dense.weight", {F, C}, DTTS_E_INVAL, &rc);
        if (!wi) return rc;
        const HostTensor* bi = gl_tensor(h, p + "intermediate.dense.bias", {F}, DTTS_E_INVAL, &rc);
        if (!bi) return rc;
        const HostTensor* w2 = gl_tensor(h, p + "output.dense.weight", {C, F}, DTTS_E_INVAL, &rc);
        if (!w2) return rc;
        const HostTensor* b2 = gl_tensor(h, p + "output.dense.bias", {C}, DTTS_E_INVAL, &rc);
        if (!b2) return rc;
        const HostTensor* g2 = gl_tensor(h, p + "output.LayerNorm.weight", {C}, DTTS_E_INVAL, &rc);
        if (!g2) return rc;
        const HostTensor* be2 = gl_tensor(h, p + "output.LayerNorm.bias", {C}, DTTS_E_INVAL, &rc);
        if (!be2) return rc;

        const float *pq = w3[0]->f.data(), *pk = w3[1]->f.data(), *pv = w3[2]->f.data();
        std::vector<float> bias3((size_t)3 * C);
        for (int i = 0; i < 3; ++i) std::copy(b3[i]->f.begin(), b3[i]->f.end(), bias3.begin() + (size_t)i * C);
        if (!pack_conv(h, L.qkv, ENG_F32, 3 * C, C, 1,
                       [=](int o, int i, int) { return (o < C ? pq : o < 2 * C ? pk : pv)[(size_t)(o % C) * C + i]; }, bias3, 1, 1, 0))
            return nomem(p + "attention.self");
        const float *po = wo->f.data(), *pi = wi->f.data(), *p2 = w2->f.data();
        if (!pack_conv(h, L.o, ENG_F32, C, C, 1, [=](int o, int i, int) { return po[(size_t)o * C + i]; }, bo->f, 1, 1, 0)) return nomem(p + "attention.output.dense");
        if (!pack_conv(h, L.ffn1, ENG_F32, F, C, 1, [=](int o, int i, int) { return pi[(size_t)o * C + i]; }, bi->f, 1, 1, 0)) return nomem(p + "intermediate.dense");
        const int Fc = F;
        if (!pack_conv(h, L.ffn2, ENG_F32, C, F, 1, [=](int o, int i, int) { return p2[(size_t)o * Fc + i]; }, b2->f, 1, 1, 0)) return nomem(p + "output.dense");
        L.g1 = upload(h, g1->f);
        L.b1 = upload(h, b1->f);
        L.g2 = upload(h, g2->f);
        L.b2 = upload(h, be2->f);
        if (!L.g1 || !L.b1 || !L.g2 || !L.b2) return nomem(p + "LayerNorm");
    }
    // the rotary table as RoFormerSinusoidalPositionalEmbedding makes it: the angle and its sine / cosine in fp64, rounded once
    std::vector<float2> rot((size_t)GLOSS_MAX_L * 32);
    for (int pos = 0; pos < GLOSS_MAX_L; ++pos)
        for (int j = 0; j < 32; ++j) {
            const double ang = (double)pos / pow(10000.0, 2.0 * (double)j / (double)GLOSS_DK);
            rot[(size_t)pos * 32 + j] = make_float2((float)sin(ang), (float)cos(ang));
        }
    std::vector<float> tt0(tt->f.begin(), tt->f.begin() + C);
    h->gloss_word = upload(h, we->f);
    h->gloss_tt0 = upload(h, tt0);
    h->gloss_eg = upload(h, eg->f);
    h->gloss_eb = upload(h, eb->f);
    h->gloss_rot = upload(h, rot);
    if (!h->gloss_word || !h->gloss_tt0 || !h->gloss_eg || !h->gloss_eb || !h->gloss_rot) return nomem("embeddings");
    h->gloss_vocab = (int)we->shape[0];
    h->gloss_C = C;
    h->gloss_F = F;
    h->gloss_eps = eps;
    h->gloss_ready = true;
    return DTTS_OK;
}


// =====================================================================================================================================
// forward
int gloss_forward(dtts_ctx* h, const dtts_gloss_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)";
    const Block blk{h, me};
    // h may be null: the block is checked first, so that the refusals are reachable without a device
    if (!a) return fail(h, DTTS_E_INVAL, "%s: null argument block", me);
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->n_gloss < 1 || a->n_gloss > (1 << 24)) return fail(h, DTTS_E_INVAL, "%s: n_gloss = %d (supported: 1 .. %d)", me, a->n_gloss, 1 << 24);
    if (a->L_max < 1 || a->L_max > DTTS_GLOSS_MAX_L)
        return fail(h, DTTS_E_INVAL, "%s: L_max = %d tokens (supported: 1 .. %d)", me, a->L_max, DTTS_GLOSS_MAX_L);
    if (a->sum_L < a->n_gloss || (long long)a->sum_L > (long long)a->n_gloss * a->L_max)
        return fail(h, DTTS_E_INVAL, "%s: sum_L = %d rows for n_gloss = %d glosses of 1 .. L_max = %d tokens", me, a->sum_L, a->n_gloss, a->L_max);
    if (!a->ids_dev || !a->tok_off_dev || !a->out_dev || !a->status_dev) return fail(h, DTTS_E_INVAL, "%s: null ids_dev / tok_off_dev / out_dev / status_dev", me);
    if (int rc = blk.aligned(8, {{"ids_dev", a->ids_dev}, {"status_dev", a->status_dev}})) return rc;
    if (int rc = blk.aligned(4, {{"tok_off_dev", a->tok_off_dev}})) return rc;
    if (int rc = blk.aligned(16, {{"out_dev", a->out_dev}})) return rc;
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_GLOSS)) return rc;

    const int C = h->gloss_C, F = h->gloss_F, rows = a->sum_L, n_layers = (int)h->gloss_layers.size();
    const int W = std::max(4 * C, F);   // q | k | v and ctx, then the feed-forward's inner rows, share one buffer
    if ((long long)rows * W > INT_MAX)
        return fail(h, DTTS_E_INVAL, "%s: sum_L = %d rows (at hidden_size %d / intermediate_size %d one call takes at most %d)", me, rows, C, F, INT_MAX / W);
    // the offsets are the one thing the kernels index by: they are checked on the host before anything is launched
    std::vector<int> off((size_t)a->n_gloss + 1);
    HIPCHK(hipMemcpyAsync(off.data(), a->tok_off_dev, off.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (off[0] != 0) return fail(h, DTTS_E_INVAL, "%s: tok_off[0] = %d (must be 0)", me, off[0]);
    int longest = 0;
    for (int g = 0; g < a->n_gloss; ++g) {
        const long long L = (long long)off[g + 1] - off[g];
        if (L < 1 || L > DTTS_GLOSS_MAX_L)
            return fail(h, DTTS_E_INVAL, "%s: gloss %d has L = %lld tokens (supported: 1 .. %d)", me, g, L, DTTS_GLOSS_MAX_L);
        longest = std::max(longest, (int)L);
    }
    if (off[a->n_gloss] != rows) return fail(h, DTTS_E_INVAL, "%s: tok_off[n_gloss] = %d differs from sum_L = %d", me, off[a->n_gloss], rows);
    if (longest != a->L_max) return fail(h, DTTS_E_INVAL, "%s: L_max = %d, the longest gloss has %d tokens", me, a->L_max, longest);

    Arena& ws = h->a_gloss;
    HIPCHK(ws.reserve((size_t)rows * (3 * (size_t)C + W) * sizeof(float) + 4 * 256, stream));
    float* x = ws.alloc<float>((size_t)rows * C);
    float* at = ws.alloc<float>((size_t)rows * C);
    float* acc = ws.alloc<float>((size_t)rows * C);
    float* big = ws.alloc<float>((size_t)rows * W);
    if (!x || !at || !acc || !big) return blk.workspace();
    float* qkv = big;
    float* ctx = big + (size_t)rows * 3 * C;

    LAUNCH(gloss_embed_launch(a->ids_dev, h->gloss_word, h->gloss_vocab, h->gloss_tt0, h->gloss_eg, h->gloss_eb, h->gloss_eps, x, acc, a->status_dev, rows,
                              C, stream));
    for (int l = 0; l < n_layers; ++l) {
        const GlossLayer& L = h->gloss_layers[l];
        ConvParams p = base_params(x, C, 1, rows, rows, qkv, 3 * C);
        p.fixed_order = 1;
        LAUNCH(conv1d_launch(L.qkv, p, stream));
        LAUNCH(gloss_attn_launch(qkv, ctx, a->tok_off_dev, h->gloss_rot, a->n_gloss, C, a->L_max, stream));
        p = base_params(ctx, C, 1, rows, rows, at, C);
        set_res(p, 0, x, C);
        p.fixed_order = 1;
        LAUNCH(conv1d_launch(L.o, p, stream));
        LAUNCH(layernorm_launch(at, at, L.g1, L.b1, h->gloss_eps, nullptr, 0, 0, 1, rows, C, stream));
        p = base_params(at, C, 1, rows, rows, big, F);
        p.post_act = 3;
        p.fixed_order = 1;
        LAUNCH(conv1d_launch(L.ffn1, p, stream));
        p = base_params(big, F, 1, rows, rows, x, C);
        set_res(p, 0, at, C);
        p.fixed_order = 1;
        LAUNCH(conv1d_launch(L.ffn2, p, stream));
        LAUNCH(gloss_ln_acc_launch(x, L.g2, L.b2, h->gloss_eps, acc, l + 1 == n_layers ? a->out_dev : nullptr, (float)(n_layers + 2), rows, C, stream));
    }
    return DTTS_OK;
}

} // namespace dtts
