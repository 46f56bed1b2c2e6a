// Band-limited resampling (resample.h; dtts_text2mel_fetch(DTTS_OUT_RESAMPLE)).  All arithmetic is fp64.
//
// ONE kernel: workgroup (x, b) owns the RESAMPLE_TILE consecutive outputs t0 .. t0 + 255 of utterance b, lane t the output t0 + t.  The
// input samples those outputs read, n(t0) - wing .. n(t_last) + wing with wing = n_win / index_step >= the taps of one wing, are staged once
// in LDS as doubles (zeros outside 0 .. L - 1; never read there, since the wings are clipped to the utterance), at most 256 inc + 2 wing + 6
// of them: 2.3 k doubles for 48000 -> 8000 with kaiser_best, the longest span of the supported rates.  A lane then walks its left wing and
// its right wing in resampy's order with one accumulator.  The table is read through L2 as pairs (win[i], delta[i]): one 16-byte load per
// tap; neighbouring lanes read entries `off` apart, whatever the ratio makes of it (the two tables are 512 KiB for kaiser_best: no LDS
// holds them).  Outputs behind n_out are written as zeros by the workgroup that owns them, so the row needs no memset.
//
// Nothing here may be contracted: n and off are truncations of tr and f, and the weights are defined as separate roundings.  The file is
// compiled with contraction off; the one fused operation of the specification, the tap product, is written as fma().
#pragma clang fp contract(off)

#include "ctx.h"
#include "resample.h"

namespace dtts {

__global__ __launch_bounds__(RESAMPLE_TILE) void resample_kernel(ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) double resample_lds_x[];
    double* xs = resample_lds_x;
    const int b = blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * RESAMPLE_TILE, t = t0 + tid;
    const int L0 = p.lens ? p.lens[b] : p.wav_ld;
    bool ok = L0 >= 1 && L0 <= p.wav_ld;
    const int L = ok ? L0 : 0;
    const double lr = (double)L * p.ratio;
    const double lc = ceil(lr);
    ok = ok && lc <= (double)p.out_ld;
    const int n_out = ok ? (int)lr : 0;
    if (blockIdx.x == 0 && tid == 0) p.out_lens[b] = ok ? (int)lc : 0;
    float* out = p.out + (size_t)b * p.out_ld;
    double* out64 = p.out64 ? p.out64 + (size_t)b * p.out_ld : nullptr;
    if (t0 >= n_out) {                                  // (uniform) the whole tile lies behind the utterance's last output
        if (t < p.out_ld) {
            out[t] = 0.f;
            if (out64) out64[t] = 0.0;
        }
        return;
    }
    const int t_last = (t0 + RESAMPLE_TILE < n_out ? t0 + RESAMPLE_TILE : n_out) - 1;
    const int n_first = (int)((double)t0 * p.inc), n_last = (int)((double)t_last * p.inc);
    const int base = n_first - p.wing;
    int span = n_last + p.wing - base + 1;
    span = span < p.lds_n ? span : p.lds_n;             // (always: resample_lds bounds it)
    const float* x = p.wav + (size_t)b * p.wav_ld;
    for (int j = tid; j < span; j += RESAMPLE_TILE) {
        const int i = base + j;
        xs[j] = (i >= 0 && i < L) ? (double)x[i] : 0.0;
    }
    __syncthreads();
    if (t >= p.out_ld) return;
    double acc = 0.0;
    if (t < n_out) {
        const double tr = (double)t * p.inc;
        const int n = (int)tr;
        const double frac = p.scale * (tr - (double)n);
        const int c = n - base;                          // x[n] in the span
        {
            const double f = frac * p.num_table;
            const int off = (int)f;
            const double eta = f - (double)off;
            int imax = (p.n_win - off) / p.index_step;
            imax = imax < n + 1 ? imax : n + 1;
            imax = imax < c + 1 ? imax : c + 1;          // (always: the span starts wing samples before n_first)
            const double2* tb = p.tab + off;
            for (int i = 0; i < imax; ++i) {
                const double2 e = tb[(size_t)i * p.index_step];
                const double w = e.x * p.tscale + eta * (e.y * p.tscale);
                acc = fma(w, xs[c - i], acc);
            }
        }
        {
            const double f = (p.scale - frac) * p.num_table;
            const int off = (int)f;
            const double eta = f - (double)off;
            int kmax = (p.n_win - off) / p.index_step;
            kmax = kmax < L - n - 1 ? kmax : L - n - 1;
            kmax = kmax < span - c - 1 ? kmax : span - c - 1;   // (always)
            const double2* tb = p.tab + off;
            for (int k = 0; k < kmax; ++k) {
                const double2 e = tb[(size_t)k * p.index_step];
                const double w = e.x * p.tscale + eta * (e.y * p.tscale);
                acc = fma(w, xs[c + k + 1], acc);
            }
        }
    }
    out[t] = (float)acc;
    if (out64) out64[t] = acc;
}

hipError_t resample_launch(const ResampleParams& p, hipStream_t stream) {
    if (p.B < 1 || p.B > 65535 || p.out_ld < 1 || p.index_step < 1 || p.wing < 1 || p.lds_n < resample_lds(p.inc, p.wing) ||
        (size_t)p.lds_n * sizeof(double) > 64 * 1024 || !p.tab || !p.out || !p.out_lens)
        return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)((p.out_ld + RESAMPLE_TILE - 1) / RESAMPLE_TILE);
    hipLaunchKernelGGL(resample_kernel, dim3(tiles, (unsigned)p.B), dim3(RESAMPLE_TILE), (size_t)p.lds_n * sizeof(double), stream, p);
    return hipGetLastError();
}

// ---- dtts_finalize_weights(DTTS_PART_RESAMPLE): "resample.filter" [n_win] + "resample.num_table" [1], both fp64 -> the plan.  Finalising
// again replaces the plan; the old table stays allocated until dtts_destroy (a launch in flight may still read it).
int build_resample(dtts_ctx* h) {
    const char* me = "dtts_finalize_weights(DTTS_PART_RESAMPLE)";
    Need need{h};
    const HostTensor* fl = need.get("resample.filter");
    const HostTensor* nt = need.get("resample.num_table");
    if (!fl || !nt) return fail(h, DTTS_E_NOENT, "%s: missing weight %s", me, need.missing.c_str());
    if (fl->shape.size() != 1 || fl->d.size() != (size_t)fl->numel() || nt->d.size() != 1)
        return fail(h, DTTS_E_INVAL, "%s: resample.filter must be [n_win] and resample.num_table one value, both loaded as DTTS_F64", me);
    const double ntv = nt->d[0];
    const int num_table = ntv >= 1.0 && ntv <= (double)RESAMPLE_MAX_TABLE ? (int)ntv : 0;
    if ((double)num_table != ntv || (num_table & (num_table - 1)))
        return fail(h, DTTS_E_INVAL, "%s: resample.num_table = %g (supported: a power of two, 1 .. %d)", me, ntv, RESAMPLE_MAX_TABLE);
    const int64_t n_win = fl->shape[0];
    if (n_win < 2 || n_win > RESAMPLE_MAX_WIN || (n_win - 1) % num_table)
        return fail(h, DTTS_E_INVAL, "%s: resample.filter has n_win = %lld entries (supported: 2 .. %d with n_win - 1 a multiple of num_table = %d)", me,
                    (long long)n_win, RESAMPLE_MAX_WIN, num_table);
    std::vector<double2> tab((size_t)n_win);
    for (int64_t i = 0; i < n_win; ++i) {
        if (!std::isfinite(fl->d[i])) return fail(h, DTTS_E_INVAL, "%s: resample.filter[%lld] is not finite", me, (long long)i);
        tab[i].x = fl->d[i];
        tab[i].y = i + 1 < n_win ? fl->d[i + 1] - fl->d[i] : 0.0;   // interp_delta: one subtraction per entry
    }
    const double2* d = upload(h, tab);
    if (!d) return fail(h, DTTS_E_NOMEM, "%s: device allocation failed", me);
    h->rs_tab = d;
    h->rs_n_win = (int)n_win;
    h->rs_num_table = num_table;
    h->resample_ready = true;
    return DTTS_OK;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_RESAMPLE): one launch on the caller's stream, no host synchronisation.  h may be null: the block is
// checked first, so that the refusals are reachable without a device
int resample_forward(dtts_ctx* h, const dtts_resample_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_RESAMPLE)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (a->B <= 0 || a->B > 65535) return fail(h, DTTS_E_INVAL, "%s: B = %d (supported: 1 .. 65535)", me, a->B);
    if (a->wav_ld < 1 || a->wav_ld > RESAMPLE_MAX_WAV) return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 1 .. %d)", me, a->wav_ld, RESAMPLE_MAX_WAV);
    if (a->out_ld < 1) return fail(h, DTTS_E_INVAL, "%s: out_ld = %d samples (must be >= 1)", me, a->out_ld);
    if (a->sr_in < 8000 || a->sr_in > 48000) return fail(h, DTTS_E_INVAL, "%s: sr_in = %d (supported: 8000 .. 48000)", me, a->sr_in);
    if (a->sr_out < 8000 || a->sr_out > 48000) return fail(h, DTTS_E_INVAL, "%s: sr_out = %d (supported: 8000 .. 48000)", me, a->sr_out);
    if (a->sr_in == a->sr_out) return fail(h, DTTS_E_INVAL, "%s: sr_out = sr_in = %d: nothing to resample", me, a->sr_in);
    if (!a->wav_dev || !a->out_dev || !a->out_lens_dev) return fail(h, DTTS_E_INVAL, "%s: null wav_dev / out_dev / out_lens_dev", me);
    if (int rc = blk.aligned(4, {{"wav_dev", a->wav_dev}, {"lens_dev", a->lens_dev}, {"out_dev", a->out_dev}, {"out_lens_dev", a->out_lens_dev}})) return rc;
    if (int rc = blk.aligned(8, {{"out64_dev", a->out64_dev}})) return rc;
    if (int rc = blk.handle()) return rc;
    if (!h->resample_ready) return fail(h, DTTS_E_NOENT, "%s: no filter: load resample.filter and resample.num_table, then dtts_finalize_weights(DTTS_PART_RESAMPLE)", me);

    ResampleParams p{};
    p.ratio = (double)a->sr_out / (double)a->sr_in;
    p.inc = 1.0 / p.ratio;
    p.scale = p.ratio < 1.0 ? p.ratio : 1.0;
    p.tscale = p.scale;
    p.num_table = (double)h->rs_num_table;
    p.index_step = (int)(p.scale * p.num_table);
    if (p.index_step < 1)
        return fail(h, DTTS_E_INVAL, "%s: sr_in = %d -> sr_out = %d gives index_step = 0 with num_table = %d (must be >= 1)", me, a->sr_in, a->sr_out, h->rs_num_table);
    p.n_win = h->rs_n_win;
    if ((p.n_win - 1) / p.index_step > RESAMPLE_MAX_WING)
        return fail(h, DTTS_E_INVAL, "%s: sr_in = %d -> sr_out = %d gives %d taps per wing with this filter (supported: up to %d)", me, a->sr_in, a->sr_out,
                    (p.n_win - 1) / p.index_step, RESAMPLE_MAX_WING);
    p.wing = p.n_win / p.index_step;
    if (p.wing < 1) p.wing = 1;
    p.lds_n = resample_lds(p.inc, p.wing);
    p.wav = a->wav_dev;
    p.lens = a->lens_dev;
    p.tab = h->rs_tab;
    p.out = a->out_dev;
    p.out_lens = a->out_lens_dev;
    p.out64 = a->out64_dev;
    p.B = a->B;
    p.wav_ld = a->wav_ld;
    p.out_ld = a->out_ld;
    LAUNCH(resample_launch(p, stream));
    return DTTS_OK;
}

} // namespace dtts
