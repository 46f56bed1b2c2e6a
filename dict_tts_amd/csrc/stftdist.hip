// Multi-resolution STFT distance of a PAIR of waveform batches on the device: per resolution (n_fft, hop, window) and utterance the three sums
// behind the reference's spectral-convergence and log-magnitude figures (modules/hifigan/stft_loss.py: stft(), SpectralConvergengeLoss,
// LogSTFTMagnitudeLoss, as tasks/vocoder/hifigan.py:62-76 reports them at validation):
//   m = sqrt(max(re^2 + im^2, 1e-7)) of torch.stft(sig, n_fft, hop, win, hann_window(win))   (center=True, pad_mode='reflect')
//   sums[0] = sum (m_y - m_x)^2,  sums[1] = sum m_y^2,  sums[2] = sum |log m_y - log m_x|     over the T_b (n_fft / 2 + 1) values of the utterance.
//
// The STFT is the shared contraction of stft_core.h.  What this unit adds (section 3.7):
//   * the 32 frame columns of the MFMA hold the PAIR: columns 0 - 15 = frames f .. f + 15 of x, columns 16 - 31 = the same frames of y, read
//     from two slabs of one LDS tile.  A basis fragment fetched from L2 serves both signals, and m_x / m_y of one (bin, frame) sit in lanes l
//     and l ^ 16 of the same accumulator register: one exchange per register per bin block brings them together.
//   * staging mirrors instead of zero filling (g < 0 -> -g, g >= len -> 2 (len - 1) - g), through the same bounds-checked buffer loads.
//   * nothing but three numbers leaves a tile: lane-local fp32 over a bin block, fp64 per lane across bin blocks, a butterfly over the wave,
//     the waves in order, one fp64 triple per (utterance, tile); stft_reduce_kernel adds the tiles of an utterance in tile order.  No atomics:
//     the same inputs give the same bits, and the tile size does not depend on the batch, so an utterance alone = the same one in any batch.
#include "ctx.h"
#include "stftdist.h"

namespace dtts {

template <int WT>
__global__ __launch_bounds__(64 * WT) void stftdist_kernel(const StftParams p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fi = lane & 31, hf = lane >> 5, sig = fi >> 4, fr = fi & 15;
    const int b = blockIdx.x / p.g.ntile, tile = blockIdx.x % p.g.ntile;
    const int len = stft_len(p.lens, b, p.wav_ld);
    if (len <= p.g.n_fft / 2) return;   // torch.stft refuses it (the mirror would leave the signal): count 0, the reduction writes zeros
    const int T = 1 + len / p.g.hop;
    const int f0 = tile * p.g.tt;
    if (f0 >= T) return;                // (whole workgroup, before any barrier; the reduction reads only the tiles below T)
    const int nf = T - f0 < p.g.tt ? T - f0 : p.g.tt;   // frame pairs of this tile

    // ---- the tile's samples of both signals, mirrored at 0 and at len - 1.  len > n_fft / 2 keeps every mirrored index inside [0, len); the
    // buffer resource would return zero for one that is not
    const float* const xy[2] = {p.x + (size_t)b * p.wav_ld, p.y + (size_t)b * p.wav_ld};
    stft_stage<64 * WT>(slab, p.ybase, xy, len, f0, nf, p.g, tid, [len](int g) {
        g = g < 0 ? -g : g;
        return g >= len ? 2 * (len - 1) - g : g;
    });
    __syncthreads();

    double s_d2 = 0.0, s_py = 0.0, s_lg = 0.0;
    if (wv * 16 < nf) {   // (wave-uniform: the exchanges below see all 64 lanes)
        const int f = wv * 16 + fr;
        const bool live = f < nf;   // the same for lanes l and l ^ 16
        const int sbase = sig ? p.ybase : 0;
        const int abase = (live ? f : wv * 16) * p.g.hop + hf;   // a dead column recomputes the wave's first frame and contributes nothing
        const int nbins = p.g.n_fft / 2 + 1;
        float* mrow = p.mag && live ? p.mag + (((size_t)sig * p.B + b) * p.mag_cap + f0 + f) * nbins : nullptr;

        stft_contract(p.g.basis, p.g.n_fft / 32, p.g.sg_lo, p.g.sg_hi, 0, p.g.n_fft / 64, slab + sbase, abase, p.g.ps, lane, [&](int c, stft_f32x16 re, stft_f32x16 im) {
            // ---- clamped powers of this lane's signal; bin 0 is real and its im slot carried re[n_fft / 2], a bin of its own
            float pw[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) pw[r] = __builtin_fmaxf(__builtin_fmaf(re[r], re[r], __fmul_rn(im[r], im[r])), STFT_CLAMP);
            float pn = STFT_CLAMP;
            const bool edge = c == 0 && hf == 0;
            if (edge) {
                pw[0] = __builtin_fmaxf(__fmul_rn(re[0], re[0]), STFT_CLAMP);
                pn = __builtin_fmaxf(__fmul_rn(im[0], im[0]), STFT_CLAMP);
            }
            if (mrow) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mrow[32 * c + 8 * (r >> 2) + 4 * hf + (r & 3)] = __builtin_sqrtf(pw[r]);
                if (edge) mrow[p.g.n_fft / 2] = __builtin_sqrtf(pn);
            }
            // ---- the pair: lane l (x) takes p_y from lane l ^ 16.  One fp32 logarithm per bin: |log m_y - log m_x| = |log(p_y / p_x)| / 2
            float a_d2 = 0.f, a_py = 0.f, a_lg = 0.f;
            auto add = [&](float px, float py) {
                const float d = __builtin_sqrtf(py) - __builtin_sqrtf(px);
                a_d2 = __builtin_fmaf(d, d, a_d2);
                a_py += py;
                a_lg += 0.5f * __builtin_fabsf(logf(py / px));
            };
            const bool mine = live && sig == 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float po = __shfl_xor(pw[r], 16);
                if (mine) add(pw[r], po);
            }
            if (c == 0) {
                const float po = __shfl_xor(pn, 16);
                if (mine && hf == 0) add(pn, po);
            }
            s_d2 += (double)a_d2;
            s_py += (double)a_py;
            s_lg += (double)a_lg;
        });
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {   // a butterfly: every lane ends with the same sum, in an order that depends on nothing
            s_d2 += __shfl_xor(s_d2, o);
            s_py += __shfl_xor(s_py, o);
            s_lg += __shfl_xor(s_lg, o);
        }
    }
    // ---- the waves in order (a wave without frames adds its zeros), one triple per tile
    double* red = (double*)(slab + p.red);
    if (lane == 0) {
        red[3 * wv + 0] = s_d2;
        red[3 * wv + 1] = s_py;
        red[3 * wv + 2] = s_lg;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < WT; ++w) s += red[3 * w + tid];
        p.part[((size_t)b * p.g.ntile + tile) * 3 + tid] = s;
    }
}

// one thread per (resolution, utterance): the tiles below T_b in tile order
__global__ void stft_reduce_kernel(const StftReduceParams p) {
    const int i = blockIdx.x, b = blockIdx.y * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int len = stft_len(p.lens, b, p.wav_ld);
    double s[3] = {0.0, 0.0, 0.0};
    long long count = 0;
    if (len > p.n_fft[i] / 2) {
        const int T = 1 + len / p.hop[i], nt = (T + p.tt[i] - 1) / p.tt[i];
        const double* q = p.part[i] + (size_t)b * p.ntile[i] * 3;
        for (int t = 0; t < nt; ++t)
            for (int k = 0; k < 3; ++k) s[k] += q[3 * t + k];
        count = (long long)T * (p.n_fft[i] / 2 + 1);
    }
    for (int k = 0; k < 3; ++k) p.sums[((size_t)i * p.B + b) * 3 + k] = s[k];
    p.count[(size_t)i * p.B + b] = count;
}

int stft_conflict_degree(int hop, int ps, int ybase) {
    int worst = 1;
    for (int w = 0; w < STFT_WAVES; ++w)
        for (int k = 0; k < (1 << std::min(ps, 8)); ++k) {
            int on_bank[32] = {};   // hop >= 1 and ybase >= one slab: the 32 lanes of a half read 32 distinct addresses
            for (int t = 0; t < 32; ++t) {
                const int a = (16 * w + (t & 15)) * hop + k;
                worst = std::max(worst, ++on_bank[((t >> 4) * ybase + a + (a >> ps)) % 32]);
            }
        }
    return worst;
}

static size_t stft_lds_bytes(int tt, int hop, int n_fft, int ps, int ybase) {
    return (((size_t)ybase + melspec_slab_dwords(tt, hop, n_fft, ps) + 1) & ~(size_t)1) * 4 + (size_t)STFT_RED_DWORDS * 4;
}

StftLayout stft_layout(int hop, int n_fft) {
    StftLayout best{31, 1, 0, INT_MAX, 0};
    for (int ps : {31, 8, 7, 6, 5}) {
        int tt = 16 * STFT_WAVES;   // what fits with the largest offset of slab y, so that the offset does not change the tile
        while (tt > 1 && stft_lds_bytes(tt, hop, n_fft, ps, (int)melspec_slab_dwords(tt, hop, n_fft, ps) + 31) > (size_t)MELSPEC_LDS_BYTES) --tt;
        const int S = (int)melspec_slab_dwords(tt, hop, n_fft, ps);
        for (int o = 0; o < 32; ++o) {
            const int d = stft_conflict_degree(hop, ps, S + o);
            if (d < best.degree) best = StftLayout{ps, tt, S + o, d, stft_lds_bytes(tt, hop, n_fft, ps, S + o)};
        }
    }
    return best;
}

hipError_t stft_launch(StftParams p, hipStream_t stream) {
    const StftGeom& g = p.g;
    if (!stft_geom_ok(g, p.B, p.wav_ld)) return hipErrorInvalidValue;
    if (p.mag && p.mag_cap < 1 + p.wav_ld / g.hop) return hipErrorInvalidValue;
    const size_t S = melspec_slab_dwords(g.tt, g.hop, g.n_fft, g.ps);
    const size_t lds = stft_lds_bytes(g.tt, g.hop, g.n_fft, g.ps, p.ybase);
    if (g.tt < 1 || g.tt > 16 * STFT_WAVES || (size_t)p.ybase < S || lds > (size_t)MELSPEC_LDS_BYTES) return hipErrorInvalidValue;
    if (g.ntile != (1 + p.wav_ld / g.hop + g.tt - 1) / g.tt || (long long)g.ntile * p.B > INT_MAX) return hipErrorInvalidValue;
    p.red = (int)(((size_t)p.ybase + S + 1) & ~(size_t)1);
    if (hipError_t e = stft_lds_limit<stftdist_kernel<STFT_WAVES>>()) return e;
    hipLaunchKernelGGL(stftdist_kernel<STFT_WAVES>, dim3((unsigned)(g.ntile * p.B)), dim3(64 * STFT_WAVES), lds, stream, p);
    return hipGetLastError();
}

hipError_t stft_reduce_launch(const StftReduceParams& p, hipStream_t stream) {
    if (p.n_res < 1 || p.n_res > STFT_MAX_RES || p.B < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stft_reduce_kernel, dim3((unsigned)p.n_res, (unsigned)((p.B + 63) / 64)), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// ---- dtts_finalize_weights(DTTS_PART_STFT): "stft.<i>.window" [n_fft], i = 0 .. (at most STFT_MAX_RES - 1), each already zero padded and
// centred to n_fft as torch.stft does it -> one plan per window.  Finalising again replaces the plans (the old packs stay allocated until
// dtts_destroy: a launch in flight may still read them).
int build_stft(dtts_ctx* h) {
    const char* me = "dtts_finalize_weights(DTTS_PART_STFT)";
    std::vector<dtts_ctx::StftPlan> plans;
    for (int i = 0; i < STFT_MAX_RES; ++i) {
        auto it = h->w.find("stft." + std::to_string(i) + ".window");
        if (it == h->w.end()) break;
        const HostTensor& wn = it->second;
        if (wn.shape.size() != 1) return fail(h, DTTS_E_INVAL, "%s: stft.%d.window must be [n_fft] (got %d dimensions)", me, i, (int)wn.shape.size());
        const int n_fft = (int)std::min<int64_t>(wn.shape[0], INT_MAX);
        std::string why;
        if (!melspec_supported(n_fft, n_fft, n_fft, 1, &why)) return fail(h, DTTS_E_INVAL, "%s: stft.%d.window: unsupported %s", me, i, why.c_str());
        const SgRange sup = window_support(wn.f);
        if (!sup.hi) return fail(h, DTTS_E_INVAL, "%s: stft.%d.window is all zero", me, i);
        dtts_ctx::StftPlan pl;
        pl.core = StftBasisPlan{upload(h, melspec_pack_basis(n_fft, wn.f)), n_fft, sup.lo, sup.hi};
        if (!pl.core.basis) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
        plans.push_back(pl);
    }
    if (plans.empty()) return fail(h, DTTS_E_NOENT, "%s: missing weight stft.0.window", me);
    h->stft_plans = plans;
    return DTTS_OK;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE): one launch per resolution + the reduction, on the caller's stream, no host synchronisation
int stft_forward(dtts_ctx* h, const dtts_stft_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_STFT_DISTANCE)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (int rc = blk.finalized(DTTS_PART_STFT)) return rc;
    if (a->n_res < 1 || a->n_res > (int)h->stft_plans.size())
        return fail(h, DTTS_E_INVAL, "%s: n_res = %d (this context has %d plans)", me, a->n_res, (int)h->stft_plans.size());
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (int e = check_wav_ld(h, me, a->wav_ld, 2048)) return e;   // (the largest n_fft: one bound for every resolution)
    for (int i = 0; i < a->n_res; ++i) {
        const int n_fft = h->stft_plans[i].core.n_fft;
        if (a->hop[i] < 1 || a->hop[i] > n_fft)
            return fail(h, DTTS_E_INVAL, "%s: hop[%d] = %d (supported: 1 .. n_fft = %d)", me, i, a->hop[i], n_fft);
        if (a->mag_dev && a->mag_cap < 1 + a->wav_ld / a->hop[i])
            return fail(h, DTTS_E_INVAL, "%s: mag_cap = %d rows, wav_ld = %d samples at hop[%d] = %d give %d", me, a->mag_cap, a->wav_ld, i, a->hop[i],
                        1 + a->wav_ld / a->hop[i]);
    }
    if (((!a->x_dev || !a->y_dev) && a->wav_ld > 0) || !a->sums_dev || !a->count_dev) return fail(h, DTTS_E_INVAL, "%s: null x_dev / y_dev / sums_dev / count_dev", me);

    StftParams sp[STFT_MAX_RES];
    StftReduceParams rp{};
    size_t ws = 0, mag_off = 0;
    for (int i = 0; i < a->n_res; ++i) {
        dtts_ctx::StftPlan& pl = h->stft_plans[i];
        if (pl.layout_hop != a->hop[i]) {
            const StftLayout l = stft_layout(a->hop[i], pl.core.n_fft);
            pl.ps = l.ps;
            pl.tt = l.tt;
            pl.ybase = l.ybase;
            pl.layout_hop = a->hop[i];
        }
        StftParams& p = sp[i];
        p = StftParams{};
        p.x = a->x_dev;
        p.y = a->y_dev;
        p.lens = a->lens_dev;
        p.mag = a->mag_dev ? a->mag_dev + mag_off : nullptr;
        p.B = a->B;
        p.wav_ld = a->wav_ld;
        p.mag_cap = a->mag_cap;
        p.g = stft_geom(pl.core, a->hop[i], pl.ps);
        p.g.tt = pl.tt;
        p.g.ntile = (1 + a->wav_ld / a->hop[i] + pl.tt - 1) / pl.tt;
        p.ybase = pl.ybase;
        if ((long long)p.g.ntile * a->B > INT_MAX) return fail(h, DTTS_E_INVAL, "%s: B = %d utterances of %d tiles", me, a->B, p.g.ntile);
        mag_off += (size_t)2 * a->B * (a->mag_dev ? a->mag_cap : 0) * (p.g.n_fft / 2 + 1);
        ws += ((size_t)a->B * p.g.ntile * 3 * sizeof(double) + 255) & ~(size_t)255;
        rp.hop[i] = p.g.hop;
        rp.n_fft[i] = p.g.n_fft;
        rp.tt[i] = p.g.tt;
        rp.ntile[i] = p.g.ntile;
    }
    HIPCHK(h->a_stft.reserve(ws, stream));
    for (int i = 0; i < a->n_res; ++i) {
        sp[i].part = h->a_stft.alloc<double>((size_t)a->B * sp[i].g.ntile * 3);
        if (!sp[i].part) return blk.workspace();
        rp.part[i] = sp[i].part;
    }
    for (int i = 0; i < a->n_res; ++i) LAUNCH(stft_launch(sp[i], stream));
    rp.lens = a->lens_dev;
    rp.sums = a->sums_dev;
    rp.count = (long long*)a->count_dev;
    rp.n_res = a->n_res;
    rp.B = a->B;
    rp.wav_ld = a->wav_ld;
    LAUNCH(stft_reduce_launch(rp, stream));
    return DTTS_OK;
}

} // namespace dtts
