// Log-mel spectrogram on the device: the vocoder's wav2spec (vocoders/base_vocoder.py:36-53 -> process_utterance,
// data_gen/tts/data_gen_utils.py:122-134): zero padding of n_fft / 2 samples on both sides, frames of n_fft samples every hop, periodic Hann
// window of win_length centred in the frame, |rfft|, mel basis, log10(max(eps, .)).  One launch per batch.
//
// The time window is the contraction index: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 chains of MELSPEC_CHUNK steps joined in fp64),
//   D[bin 32][frame 32] += Wd[bin][k 2] * X[k 2][frame],   X[k][frame f] = slab[f * hop + k],
// a row-shifted window of ONE LDS tile: the samples of a tile of frames are staged once, (tt - 1) * hop + n_fft floats,
// by bounds-checked buffer loads — samples before 0 and past wav_lens[b] read as zero, which IS the reference's constant padding.
//   * Wd is the windowed DFT basis, computed in fp64 at finalisation, rounded once to fp32, stored in fragment order and streamed from L2.
//     Its real output columns number exactly n_fft: re[0 .. n_fft/2] and im[1 .. n_fft/2 - 1].  A wave holds re and im of the SAME 32 bins in
//     two accumulators with matching positions, so the magnitude needs no exchange; re[n_fft/2] rides in the (otherwise zero) im slot of bin 0.
//   * |X| stays in accumulator layout and is at once the B operand of the mel projection D2[mel 32][frame 32] += M[mel][bin 2] * |X|[bin 2][frame]:
//     register r of the two lane halves holds bins b and b + 4, which is the k pair of one MFMA; the mel pack is stored in that order.
//   * every frame is summed in the same order whatever tile it falls into (k in order, bin blocks in order): an utterance alone is
//     bit-identical to the same utterance inside any batch, at either tile size.
//   * a wave owns 32 frames of the tile; the slab is placed with a skew (sample a at dword a + (a >> ps)) so that the 32 rows of a fragment,
//     hop samples apart, fall into different banks (melspec_conflict_degree enumerates the read).
#include "ctx.h"

namespace dtts {

typedef __attribute__((ext_vector_type(16))) float f32x16m;

template <int WT>
__global__ __launch_bounds__(64 * WT) void melspec_kernel(const MelspecParams p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    constexpr int THREADS = 64 * WT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fi = lane & 31, hf = lane >> 5;
    const int b = blockIdx.x / p.ntile, tile = blockIdx.x % p.ntile;
    int len = p.wav_lens ? p.wav_lens[b] : p.wav_ld;
    len = len < 0 ? 0 : (len > p.wav_ld ? p.wav_ld : len);
    const int T = 1 + len / p.hop;
    if (tile == 0 && tid == 0 && p.mel_lens) p.mel_lens[b] = T;
    const int f0 = tile * p.tt;
    if (f0 >= T) return;
    const int nf = T - f0 < p.tt ? T - f0 : p.tt;   // frames of this tile
    const int ps = p.ps;

    // ---- the tile's samples: global sample g0 + q -> slab position q; outside [0, len) the buffer resource returns zero
    {
        const int P = (nf - 1) * p.hop + p.n_fft;
        const int g0 = f0 * p.hop - p.n_fft / 2;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.wav + (size_t)b * p.wav_ld), 0, len * 4, 0x00020000);
        for (int q = tid; q < P; q += THREADS) {
            const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(rs, (g0 + q) * 4, 0, 0);   // (a negative offset is a huge unsigned one)
            slab[q + (q >> ps)] = __builtin_bit_cast(float, v);
        }
    }
    __syncthreads();
    if (wv * 32 >= nf) return;   // (no barrier below)
    const int f = wv * 32 + fi;
    const bool live = f < nf;
    const int abase = (live ? f : wv * 32) * p.hop + hf;   // a dead lane recomputes the wave's first frame and stores nothing

    const int NB = p.n_fft / 64, SG = p.n_fft / 32, NM = (p.n_mels + 31) / 32;
    f32x16m macc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[mt][r] = 0.f;

    // one super-group = 16 MFMA steps = 32 samples: eight 16-byte fragments per lane (re of steps 0-3, .., 12-15, then im).  Two register
    // buffers take turns: while one is contracted (2048 MFMA cycles) the next super-group — of the next bin block behind this one's last — is on
    // its way from L2.  The launcher hands out a multiple of four super-groups per bin block (sg_lo a multiple of four too), so the turns need no copy.
    auto fetch = [&](float4 (&d)[8], int c, int sg) {
        const float4* s = p.basis + ((size_t)(c * SG + sg) * 8) * 64 + lane;
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = s[q * 64];
        __builtin_amdgcn_sched_barrier(0);   // the loads go out before the contraction they hide behind
    };
    float4 fa[8], fb[8];
    fetch(fa, 0, p.sg_lo);
#pragma unroll 1
    for (int c = 0; c < NB; ++c) {
        // Short fp32 chains joined in fp64: every MELSPEC_CHUNK MFMA steps (2 MELSPEC_CHUNK samples) start from zero and their sum goes into an
        // fp64 accumulator (exact next to fp32), rounded to fp32 once per bin block.  An fp32 chain rounds every step at the size of its
        // PARTIAL sum, which next to a strong harmonic or an offset is tens of times the final value; a chain of a few
        // samples never gets there.  The order stays fixed: chunks in k order.
        double dre[16], dim[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dre[r] = dim[r] = 0.0;
        auto contract = [&](const float4 (&w)[8], int sg) {
            const int a0 = abase + 32 * sg;
#pragma unroll
            for (int ch = 0; ch < 16 / MELSPEC_CHUNK; ++ch) {
                f32x16m re, im;
#pragma unroll
                for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
#pragma unroll
                for (int jj = 0; jj < MELSPEC_CHUNK; ++jj) {
                    const int j = ch * MELSPEC_CHUNK + jj, a = a0 + 2 * j;
                    const float x = slab[a + (a >> ps)];
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j >> 2][j & 3], x, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(w[4 + (j >> 2)][j & 3], x, im, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dre[r] += (double)re[r];
                    dim[r] += (double)im[r];
                }
            }
        };
#pragma unroll 1
        for (int sg = p.sg_lo; sg < p.sg_hi; sg += 4) {
            fetch(fb, c, sg + 1);
            contract(fa, sg);
            fetch(fa, c, sg + 2);
            contract(fb, sg + 1);
            fetch(fb, c, sg + 3);
            contract(fa, sg + 2);
            const bool wrap = sg + 4 == p.sg_hi;
            fetch(fa, wrap ? (c + 1 < NB ? c + 1 : c) : c, wrap ? p.sg_lo : sg + 4);
            contract(fb, sg + 3);
        }
        f32x16m re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            re[r] = (float)dre[r];
            im[r] = (float)dim[r];
        }
        // ---- magnitudes in place, then straight into the mel projection
        float mag[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) mag[r] = __builtin_sqrtf(__builtin_fmaf(re[r], re[r], __fmul_rn(im[r], im[r])));
        float nyq = 0.f;
        if (c == 0 && hf == 0) {   // bin 0 is real, and its im slot carried re[n_fft / 2]
            mag[0] = __builtin_fabsf(re[0]);
            nyq = __builtin_fabsf(im[0]);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt < NM) {
                const float4* mp = p.melpack + ((size_t)(c * NM + mt) * 4) * 64 + lane;
                float4 mq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) mq[q] = mp[q * 64];
#pragma unroll
                for (int r = 0; r < 16; ++r) macc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(mq[r >> 2][r & 3], mag[r], macc[mt], 0, 0, 0);
                if (c == 0) {
                    const float an = ((const float*)(p.melpack + (size_t)NB * NM * 4 * 64))[mt * 64 + lane];
                    macc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(an, nyq, macc[mt], 0, 0, 0);
                }
            }
        }
    }

    // ---- log10(max(eps, mel)) rows [T][n_mels]; the logarithm in fp64 (80 per frame against 2 n_fft^2 FLOP), rounded once
    if (live) {
        const size_t row = ((size_t)b * p.mel_cap + f0 + f) * p.n_mels;
        float* out = p.mel + row;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            if (mt < NM) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = 32 * mt + 8 * (r >> 2) + 4 * hf + (r & 3);
                    const float v = macc[mt][r];
                    if (m < p.n_mels) out[m] = (float)log10((double)(v > p.eps ? v : p.eps));
                    if (m < p.n_mels && p.lin) p.lin[row + m] = v;
                }
            }
        }
    }
}

bool melspec_supported(int n_fft, int hop, int win, int n_mels, std::string* why) {
    auto no = [&](const std::string& s) {
        if (why) *why = s;
        return false;
    };
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return no("n_fft = " + std::to_string(n_fft) + " (supported: 512, 1024, 2048)");
    if (win < 1 || win > n_fft) return no("win_length = " + std::to_string(win) + " (supported: 1 .. n_fft = " + std::to_string(n_fft) + ")");
    if (hop < 1 || hop > n_fft) return no("hop = " + std::to_string(hop) + " (supported: 1 .. n_fft = " + std::to_string(n_fft) + ")");
    if (n_mels < 1 || n_mels > MELSPEC_MAX_MELS) return no("n_mels = " + std::to_string(n_mels) + " (supported: 1 .. " + std::to_string(MELSPEC_MAX_MELS) + ")");
    return true;
}

int melspec_conflict_degree(int hop, int ps) {
    int worst = 1;
    for (int w = 0; w < 4; ++w)
        for (int k = 0; k < (1 << std::min(ps, 8)); ++k) {
            int on_bank[32] = {};   // hop >= 1: the 32 rows of a half read 32 distinct addresses
            for (int t = 0; t < 32; ++t) {
                const int a = (32 * w + t) * hop + k;
                worst = std::max(worst, ++on_bank[(a + (a >> ps)) % 32]);
            }
        }
    return worst;
}

int melspec_skew_shift(int hop) {
    int best = 31, deg = INT_MAX;   // 31: no skew (a >> 31 = 0), for the hops that need none
    for (int ps : {31, 8, 7, 6, 5}) {
        const int d = melspec_conflict_degree(hop, ps);
        if (d < deg) {
            deg = d;
            best = ps;
        }
    }
    return best;
}

int melspec_tile_frames(int waves, int hop, int n_fft, int ps) {
    int tt = 32 * waves;
    while (tt > 1 && melspec_slab_dwords(tt, hop, n_fft, ps) * 4 > (size_t)MELSPEC_LDS_BYTES) --tt;
    return tt;
}

// Wd[col][k] = w[k] cos(2 pi bin k / n_fft) (re) and -w[k] sin(..) (im), w the window centred in the frame.  The angle is reduced exactly
// (bin * k mod n_fft) and looked up in an fp64 table.  Order: [bin block c][super-group sg][part][lane][4], parts 0 .. 3 = re of MFMA steps
// 0-3 .. 12-15 of the super-group, 4 .. 7 = im; step j of super-group sg contracts samples k = 32 sg + 2 j + (lane >> 5); bin = 32 c + (lane & 31).
std::vector<float> melspec_pack_basis(int n_fft, const std::vector<float>& window) {
    const int N = n_fft, win = (int)window.size(), lpad = (N - win) / 2, NB = N / 64, SG = N / 32;
    std::vector<double> cs(N), sn(N), w(N, 0.0);
    for (int j = 0; j < N; ++j) {
        cs[j] = cos(2.0 * M_PI * j / N);
        sn[j] = sin(2.0 * M_PI * j / N);
    }
    for (int k = 0; k < win; ++k) w[lpad + k] = (double)window[k];
    std::vector<float> out((size_t)NB * SG * 8 * 64 * 4);
    for (int c = 0; c < NB; ++c)
        for (int sg = 0; sg < SG; ++sg)
            for (int part = 0; part < 8; ++part)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int j = 4 * (part & 3) + e, k = 32 * sg + 2 * j + (lane >> 5), bin = 32 * c + (lane & 31);
                        const int ang = (int)(((long long)bin * k) % N);
                        double v;
                        if (part < 4) v = w[k] * cs[ang];
                        else if (bin == 0) v = w[k] * ((k & 1) ? -1.0 : 1.0);   // re[n_fft / 2] in the im slot of bin 0
                        else v = -w[k] * sn[ang];
                        out[((((size_t)(c * SG + sg) * 8 + part) * 64) + lane) * 4 + e] = (float)v;
                    }
    return out;
}

// M[mel][bin] as the A operand of the projection: [bin block c][mel tile mt][q][lane][4], element e of q = accumulator register r = 4 q + e
// = bin 32 c + 8 (r >> 2) + (r & 3) + 4 (lane >> 5), mel = 32 mt + (lane & 31); behind them [mt][lane]: the Nyquist column (lanes < 32).
std::vector<float> melspec_pack_mel(int n_fft, int n_mels, const std::vector<float>& mel_basis) {
    const int NB = n_fft / 64, NM = (n_mels + 31) / 32, ld = n_fft / 2 + 1;
    std::vector<float> out((size_t)NB * NM * 4 * 64 * 4 + (size_t)NM * 64, 0.f);
    for (int c = 0; c < NB; ++c)
        for (int mt = 0; mt < NM; ++mt)
            for (int q = 0; q < 4; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * q + e, bin = 32 * c + 8 * (r >> 2) + (r & 3) + 4 * (lane >> 5), m = 32 * mt + (lane & 31);
                        if (m < n_mels) out[((((size_t)(c * NM + mt) * 4 + q) * 64) + lane) * 4 + e] = mel_basis[(size_t)m * ld + bin];
                    }
    for (int mt = 0; mt < NM; ++mt)
        for (int lane = 0; lane < 32; ++lane)
            if (32 * mt + lane < n_mels) out[(size_t)NB * NM * 4 * 64 * 4 + mt * 64 + lane] = mel_basis[(size_t)(32 * mt + lane) * ld + n_fft / 2];
    return out;
}

template <int WT>
static hipError_t melspec_launch_cfg(MelspecParams p, hipStream_t stream) {
    p.tt = melspec_tile_frames(WT, p.hop, p.n_fft, p.ps);
    const int t_cap = 1 + p.wav_ld / p.hop;
    p.ntile = (t_cap + p.tt - 1) / p.tt;
    const size_t lds = melspec_slab_dwords(p.tt, p.hop, p.n_fft, p.ps) * 4;
    if (lds > (size_t)MELSPEC_LDS_BYTES || (long long)p.ntile * p.B > INT_MAX) return hipErrorInvalidValue;
    auto kern = melspec_kernel<WT>;
    static bool configured_dev[64] = {};   // per device: hipFuncSetAttribute is per device
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    bool& configured = configured_dev[cur_dev & 63];
    if (!configured) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, MELSPEC_LDS_BYTES);
        if (e != hipSuccess) return e;
        configured = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.ntile * p.B)), dim3(64 * WT), lds, stream, p);
    return hipGetLastError();
}

// The tile rule: four waves x 32 frames; while those tiles would leave more than half of the CUs without one (B = 1), two waves x 32 frames
// (two workgroups share a CU).  Where the LDS holds fewer frames (long hops) a tile carries what fits.
hipError_t melspec_launch(const MelspecParams& p, int n_cu, hipStream_t stream) {
    if (!melspec_supported(p.n_fft, p.hop, p.n_fft, p.n_mels)) return hipErrorInvalidValue;
    if (p.B < 1 || p.wav_ld < 0 || p.sg_lo < 0 || p.sg_hi > p.n_fft / 32 || p.sg_lo >= p.sg_hi || (p.sg_lo & 3) || (p.sg_hi & 3) || p.ps < 1) return hipErrorInvalidValue;
    // 32-bit byte offsets inside an utterance's buffer resource: a tile reaches at most one slab past the utterance's end
    if (((long long)p.wav_ld + MELSPEC_LDS_BYTES / 4 + p.n_fft) * 4 >= (1LL << 31)) return hipErrorInvalidValue;
    if (p.mel_cap < 1 + p.wav_ld / p.hop) return hipErrorInvalidValue;
    const int tt4 = melspec_tile_frames(4, p.hop, p.n_fft, p.ps);
    const long long tiles4 = (long long)p.B * ((1 + p.wav_ld / p.hop + tt4 - 1) / tt4);
    return 2 * tiles4 <= n_cu ? melspec_launch_cfg<2>(p, stream) : melspec_launch_cfg<4>(p, stream);
}

// ---- dtts_finalize_weights(DTTS_PART_MELSPEC): "melspec.mel_basis" [n_mels][n_fft / 2 + 1] + "melspec.window" [win_length] -> the plan.
// Finalising again replaces the plan; the packs of the old one stay allocated until dtts_destroy (a launch in flight may still read them).
int build_melspec(dtts_ctx* h) {
    Need need{h};
    const HostTensor* mb = need.get("melspec.mel_basis");
    const HostTensor* wn = need.get("melspec.window");
    if (!mb || !wn) return fail(h, DTTS_E_NOENT, "dtts_finalize_weights(DTTS_PART_MELSPEC): missing weight %s", need.missing.c_str());
    if (mb->shape.size() != 2 || wn->shape.size() != 1 || mb->shape[1] < 2)
        return fail(h, DTTS_E_INVAL, "dtts_finalize_weights(DTTS_PART_MELSPEC): melspec.mel_basis must be [n_mels][n_fft / 2 + 1] and melspec.window [win_length] "
                    "(got %d and %d dimensions)", (int)mb->shape.size(), (int)wn->shape.size());
    const int n_mels = (int)std::min<int64_t>(mb->shape[0], INT_MAX), n_fft = (int)std::min<int64_t>(2 * (mb->shape[1] - 1), INT_MAX);
    const int win = (int)std::min<int64_t>(wn->shape[0], INT_MAX);
    std::string why;
    if (!melspec_supported(n_fft, n_fft, win, n_mels, &why))   // (the hop arrives with each call: any supported one stands in here)
        return fail(h, DTTS_E_INVAL, "dtts_finalize_weights(DTTS_PART_MELSPEC): unsupported %s", why.c_str());
    float* basis = upload(h, melspec_pack_basis(n_fft, wn->f));
    float* melpack = upload(h, melspec_pack_mel(n_fft, n_mels, mb->f));
    if (!basis || !melpack) return fail(h, DTTS_E_NOMEM, "dtts_finalize_weights(DTTS_PART_MELSPEC): device allocation failed");
    // the samples a zero of the centred window removes from the contraction (win_length < n_fft), in whole FOURS of 32-sample super-groups
    const int lpad = (n_fft - win) / 2;
    h->ms_basis = basis;
    h->ms_melpack = melpack;
    h->ms_n_fft = n_fft;
    h->ms_n_mels = n_mels;
    h->ms_win = win;
    h->ms_sg_lo = lpad / 128 * 4;
    h->ms_sg_hi = (lpad + win + 127) / 128 * 4;
    h->ms_skew_hop = 0;
    h->melspec_ready = true;
    return DTTS_OK;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_MELSPEC): one launch on the caller's stream, no host synchronisation
int melspec_forward(dtts_ctx* h, const dtts_melspec_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_MELSPEC)";
    if (a->size != (int32_t)sizeof(dtts_melspec_args))
        return fail(h, DTTS_E_INVAL, "%s: argument block of size = %d bytes, this library's is %d", me, a->size, (int)sizeof(dtts_melspec_args));
    if (!h->melspec_ready) return fail(h, DTTS_E_STATE, "%s before dtts_finalize_weights(DTTS_PART_MELSPEC)", me);
    std::string why;
    if (!melspec_supported(h->ms_n_fft, a->hop, h->ms_win, h->ms_n_mels, &why)) return fail(h, DTTS_E_INVAL, "%s: unsupported %s", me, why.c_str());
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (a->wav_ld < 0 || ((long long)a->wav_ld + MELSPEC_LDS_BYTES / 4 + h->ms_n_fft) * 4 >= (1LL << 31))
        return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 0 .. 2^29 - 2^16)", me, a->wav_ld);
    if (a->mel_cap < 1 + a->wav_ld / a->hop)
        return fail(h, DTTS_E_INVAL, "%s: mel_cap = %d rows, wav_ld = %d samples at hop %d give %d", me, a->mel_cap, a->wav_ld, a->hop, 1 + a->wav_ld / a->hop);
    if (!(a->eps > 0.f) || !(a->eps < 3.0e38f)) return fail(h, DTTS_E_INVAL, "%s: eps = %g (must be positive and finite)", me, (double)a->eps);
    if ((!a->wav_dev && a->wav_ld > 0) || !a->mel_dev) return fail(h, DTTS_E_INVAL, "%s: null wav_dev / mel_dev", me);
    if (h->ms_skew_hop != a->hop) {
        h->ms_skew = melspec_skew_shift(a->hop);
        h->ms_skew_hop = a->hop;
    }
    MelspecParams p{};
    p.wav = a->wav_dev;
    p.wav_lens = a->wav_lens_dev;
    p.mel = a->mel_dev;
    p.mel_lens = a->mel_lens_dev;
    p.lin = a->lin_dev;
    p.basis = (const float4*)h->ms_basis;
    p.melpack = (const float4*)h->ms_melpack;
    p.B = a->B;
    p.wav_ld = a->wav_ld;
    p.mel_cap = a->mel_cap;
    p.hop = a->hop;
    p.n_fft = h->ms_n_fft;
    p.n_mels = h->ms_n_mels;
    p.sg_lo = h->ms_sg_lo;
    p.sg_hi = h->ms_sg_hi;
    p.ps = h->ms_skew;
    p.eps = a->eps;
    LAUNCH(melspec_launch(p, h->n_cu, stream));
    return DTTS_OK;
}

} // namespace dtts
