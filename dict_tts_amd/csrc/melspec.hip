// Log-mel spectrogram on the device: the vocoder's wav2spec (vocoders/base_vocoder.py:36-53 -> process_utterance,
// data_gen/tts/data_gen_utils.py:122-134): zero padding of n_fft / 2 samples on both sides, frames of n_fft samples every hop, periodic Hann
// window of win_length centred in the frame, |rfft|, mel basis, log10(max(eps, .)).  One launch per batch.
//
// The STFT is the shared contraction of stft_core.h: the samples of a tile of frames staged once into one LDS slab —
// samples before 0 and past wav_lens[b] read as zero, which IS the reference's constant padding — and contracted against the windowed DFT
// basis on v_mfma_f32_32x32x2_f32.  What this unit adds:
//   * re and im of the same 32 bins sit in matching accumulator positions, so the magnitude needs no exchange.
//   * |X| stays in accumulator layout and is at once the B operand of the mel projection D2[mel 32][frame 32] += M[mel][bin 2] * |X|[bin 2][frame]:
//     register r of the two lane halves holds bins b and b + 4, which is the k pair of one MFMA; the mel pack is stored in that order.
//   * a wave owns 32 frames of the tile; bin blocks are projected in order, so an utterance alone is bit-identical to the same utterance
//     inside any batch, at either tile size.
#include "ctx.h"

namespace dtts {

template <int WT>
__global__ __launch_bounds__(64 * WT) void melspec_kernel(const MelspecParams p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, fi = lane & 31, hf = lane >> 5;
    const int b = blockIdx.x / p.g.ntile, tile = blockIdx.x % p.g.ntile;
    const int len = stft_len(p.wav_lens, b, p.wav_ld);
    const int T = 1 + len / p.g.hop;
    if (tile == 0 && tid == 0 && p.mel_lens) p.mel_lens[b] = T;
    const int f0 = tile * p.g.tt;
    if (f0 >= T) return;
    const int nf = T - f0 < p.g.tt ? T - f0 : p.g.tt;   // frames of this tile
    const float* const sig[1] = {p.wav + (size_t)b * p.wav_ld};
    stft_stage<64 * WT>(slab, 0, sig, len, f0, nf, p.g, tid, [](int g) { return g; });
    __syncthreads();
    if (wv * 32 >= nf) return;   // (no barrier below)
    const int f = wv * 32 + fi;
    const bool live = f < nf;
    const int abase = (live ? f : wv * 32) * p.g.hop + hf;   // a dead lane recomputes the wave's first frame and stores nothing

    const int NB = p.g.n_fft / 64, NM = (p.n_mels + 31) / 32;
    stft_f32x16 macc[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[mt][r] = 0.f;

    stft_contract(p.g.basis, p.g.n_fft / 32, p.g.sg_lo, p.g.sg_hi, 0, NB, slab, abase, p.g.ps, lane, [&](int c, stft_f32x16 re, stft_f32x16 im) {
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
    });

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

SgRange window_support(const std::vector<float>& window) {
    int lo = (int)window.size(), hi = -1;
    for (int k = 0; k < (int)window.size(); ++k)
        if (window[k] != 0.f) {
            lo = std::min(lo, k);
            hi = k;
        }
    return SgRange{lo / 128 * 4, (hi + 128) / 128 * 4};
}

int check_wav_ld(dtts_ctx* h, const char* me, int wav_ld, int n_fft) {
    if (stft_wav_ld_ok(wav_ld, n_fft)) return DTTS_OK;
    return fail(h, DTTS_E_INVAL, "%s: wav_ld = %d samples (supported: 0 .. 2^29 - 2^16)", me, wav_ld);
}

template <int WT>
static hipError_t melspec_launch_cfg(MelspecParams p, hipStream_t stream) {
    const size_t lds = stft_set_tile(p.g, WT, p.wav_ld);
    if (lds > (size_t)MELSPEC_LDS_BYTES || (long long)p.g.ntile * p.B > INT_MAX) return hipErrorInvalidValue;
    if (hipError_t e = stft_lds_limit<melspec_kernel<WT>>()) return e;
    hipLaunchKernelGGL(melspec_kernel<WT>, dim3((unsigned)(p.g.ntile * p.B)), dim3(64 * WT), lds, stream, p);
    return hipGetLastError();
}

hipError_t melspec_launch(const MelspecParams& p, int n_cu, hipStream_t stream) {
    if (!stft_geom_ok(p.g, p.B, p.wav_ld) || p.n_mels < 1 || p.n_mels > MELSPEC_MAX_MELS) return hipErrorInvalidValue;
    if (p.mel_cap < 1 + p.wav_ld / p.g.hop) return hipErrorInvalidValue;
    return stft_tile_waves(p.B, p.wav_ld, p.g.hop, p.g.n_fft, p.g.ps, n_cu) == 2 ? melspec_launch_cfg<2>(p, stream) : melspec_launch_cfg<4>(p, stream);
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
    h->ms = StftBasisPlan{basis, n_fft, lpad / 128 * 4, (lpad + win + 127) / 128 * 4};
    h->ms_melpack = melpack;
    h->ms_n_mels = n_mels;
    h->ms_win = win;
    h->ms_skew_hop = 0;
    h->melspec_ready = true;
    return DTTS_OK;
}

// ---- dtts_text2mel_fetch(DTTS_OUT_MELSPEC): one launch on the caller's stream, no host synchronisation
int melspec_forward(dtts_ctx* h, const dtts_melspec_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_OUT_MELSPEC)";
    const Block blk{h, me};
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    if (int rc = blk.finalized(DTTS_PART_MELSPEC)) return rc;
    std::string why;
    if (!melspec_supported(h->ms.n_fft, a->hop, h->ms_win, h->ms_n_mels, &why)) return fail(h, DTTS_E_INVAL, "%s: unsupported %s", me, why.c_str());
    if (a->B <= 0) return fail(h, DTTS_E_INVAL, "%s: B = %d", me, a->B);
    if (int e = check_wav_ld(h, me, a->wav_ld, h->ms.n_fft)) return e;
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
    p.melpack = (const float4*)h->ms_melpack;
    p.g = stft_geom(h->ms, a->hop, h->ms_skew);
    p.B = a->B;
    p.wav_ld = a->wav_ld;
    p.mel_cap = a->mel_cap;
    p.n_mels = h->ms_n_mels;
    p.eps = a->eps;
    LAUNCH(melspec_launch(p, h->n_cu, stream));
    return DTTS_OK;
}

} // namespace dtts
