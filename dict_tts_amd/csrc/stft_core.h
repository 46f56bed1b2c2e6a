// The STFT contraction that melspec.hip (log-mel), stftdist.hip (STFT distance of a pair) and istft.hip (forward half of the spectral filter)
// share, with the host-side rules around it.  The time window is the contraction index of v_mfma_f32_32x32x2_f32
// (exact fp32 products, fp32 chains of MELSPEC_CHUNK steps joined in fp64),
//   D[bin 32][frame 32] += Wd[bin][k 2] * X[k 2][frame],   X[k][frame f] = slab[f * hop + k],
// a row-shifted window of ONE LDS tile: the samples of a tile of frames are staged once, (tt - 1) * hop + n_fft floats, by bounds-checked
// buffer loads (stft_stage), and every wave contracts its 32 frame columns against the streamed basis (stft_contract).
//   * Wd is the windowed DFT basis (melspec_pack_basis), computed in fp64 at finalisation, rounded once to fp32, stored in fragment order and
//     streamed from L2.  Its real output columns number exactly n_fft: re[0 .. n_fft/2] and im[1 .. n_fft/2 - 1].  A wave holds re and im of
//     the SAME 32 bins in two accumulators with matching positions; re[n_fft/2] rides in the (otherwise zero) im slot of bin 0.
//   * every frame is summed in the same order whatever tile it falls into (k in order, bin blocks in order): an utterance alone is
//     bit-identical to the same utterance inside any batch, at any tile size.  That order is written here and nowhere else.
//   * the slab is placed with a skew (sample a at dword a + (a >> ps)) so that the 32 rows of a fragment, hop samples apart, fall into
//     different banks (melspec_conflict_degree enumerates the read).
// The names keep the MELSPEC_ / melspec_ prefix of the unit that came first: tests, tools/lds_conflicts_*.py and the notes refer to them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <vector>

namespace dtts {

constexpr int MELSPEC_LDS_BYTES = 160 * 1024;
constexpr int MELSPEC_CHUNK = 4;   // MFMA steps (of two samples) per fp32 chain of the contraction; the chains are joined in fp64.  Divides 16.

typedef __attribute__((ext_vector_type(16))) float stft_f32x16;   // one 32 x 32 accumulator

// what a finaliser keeps of a window (dtts_ctx: the melspec plan, every StftPlan, the istft plan) ...
struct StftBasisPlan {
    float* basis = nullptr;         // melspec_pack_basis of the window, on the device
    int n_fft = 0;
    int sg_lo = 0, sg_hi = 0;       // the 32-sample super-groups of the contraction that the window does not zero (both multiples of four)
};

// ... and what a launch adds to it: embedded in MelspecParams, StftParams and SpecFwdParams
struct StftGeom {
    const float4* basis;
    int hop, n_fft;
    int sg_lo, sg_hi;        // as StftBasisPlan
    int tt;                  // frames (stftdist: frame pairs) per tile: what fits the LDS at this hop
    int ntile;               // tiles per utterance at wav_ld samples
    int ps;                  // slab skew: sample a of the tile lives at LDS dword a + (a >> ps)
};

inline StftGeom stft_geom(const StftBasisPlan& pl, int hop, int ps) {   // (tt and ntile are the launcher's, or stft_layout's)
    return StftGeom{(const float4*)pl.basis, hop, pl.n_fft, pl.sg_lo, pl.sg_hi, 0, 0, ps};
}

// The one predicate of the supported set (finalisers and launchers): n_fft in {512, 1024, 2048}, 1 <= win <= n_fft, 1 <= hop <= n_fft,
// 1 <= n_mels <= 128 (a unit without mel rows passes 1).  *why names the offending value.
bool melspec_supported(int n_fft, int hop, int win, int n_mels, std::string* why = nullptr);

// worst conflict degree of the contraction's slab read (ds_read_b32: 32 banks, the two 32-lane halves are separate groups) at this hop
// and skew, over every phase of the contraction index; tools/lds_conflicts_melspec.py restates it
int melspec_conflict_degree(int hop, int ps);
int melspec_skew_shift(int hop);   // the skew the launcher takes: the smallest degree, ties to the smaller pad

// LDS dwords of a tile of tt frames
inline size_t melspec_slab_dwords(int tt, int hop, int n_fft, int ps) {
    const size_t P = (size_t)(tt - 1) * hop + n_fft;
    return P + (P >> ps) + 1;
}
int melspec_tile_frames(int waves, int hop, int n_fft, int ps);

// fp64 on the host, rounded once to fp32, in the order stft_contract walks it
std::vector<float> melspec_pack_basis(int n_fft, const std::vector<float>& window);

// The non-zero support of a window already zero padded and centred to n_fft, in whole FOURS of 32-sample super-groups, as the contraction
// walks them.  hi = 0: the window is all zero.  (build_melspec is given the un-centred window and derives its range from win_length.)
struct SgRange { int lo, hi; };
SgRange window_support(const std::vector<float>& window);

// 32-bit byte offsets inside an utterance's buffer resource: a tile reaches at most one slab past the utterance's end
inline bool stft_wav_ld_ok(int wav_ld, int n_fft) { return wav_ld >= 0 && ((long long)wav_ld + MELSPEC_LDS_BYTES / 4 + n_fft) * 4 < (1LL << 31); }

// what every launcher refuses before its own conditions; tt and ntile are not looked at (a launcher sets or checks them itself)
inline bool stft_geom_ok(const StftGeom& g, int B, int wav_ld) {
    return melspec_supported(g.n_fft, g.hop, g.n_fft, 1) && B >= 1 && g.sg_lo >= 0 && g.sg_hi <= g.n_fft / 32 && g.sg_lo < g.sg_hi && !(g.sg_lo & 3) &&
           !(g.sg_hi & 3) && g.ps >= 1 && stft_wav_ld_ok(wav_ld, g.n_fft);
}

// The tile rule of the launchers that may choose (melspec, spectral forward): four waves x 32 frames; while those tiles would leave more than
// half of the CUs without one (B = 1), two waves x 32 frames (two workgroups share a CU).  Where the LDS holds fewer frames (long hops) a
// tile carries what fits.
inline int stft_tile_waves(int B, int wav_ld, int hop, int n_fft, int ps, int n_cu) {
    const int tt4 = melspec_tile_frames(4, hop, n_fft, ps);
    const long long tiles4 = (long long)B * ((1 + wav_ld / hop + tt4 - 1) / tt4);
    return 2 * tiles4 <= n_cu ? 2 : 4;
}

// tt and ntile of a tile of `waves` waves x 32 frames; returns the slab's LDS bytes
inline size_t stft_set_tile(StftGeom& g, int waves, int wav_ld) {
    g.tt = melspec_tile_frames(waves, g.hop, g.n_fft, g.ps);
    g.ntile = (1 + wav_ld / g.hop + g.tt - 1) / g.tt;
    return melspec_slab_dwords(g.tt, g.hop, g.n_fft, g.ps) * 4;
}

// raises the dynamic-LDS limit of kernel Kern to MELSPEC_LDS_BYTES, once per device (hipFuncSetAttribute is per device)
template <auto Kern>
hipError_t stft_lds_limit() {
    static bool configured_dev[64] = {};
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    bool& configured = configured_dev[cur_dev & 63];
    if (!configured) {
        hipError_t e = hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, MELSPEC_LDS_BYTES);
        if (e != hipSuccess) return e;
        configured = true;
    }
    return hipSuccess;
}

// samples of utterance b: lens[b] (or wav_ld without lens) clamped to 0 .. wav_ld
__device__ __forceinline__ int stft_len(const int* lens, int b, int wav_ld) {
    const int len = lens ? lens[b] : wav_ld;
    return len < 0 ? 0 : (len > wav_ld ? wav_ld : len);
}

// The samples of a tile of nf frames from frame f0 on, of NS signals in one pass: global sample map(g0 + q) of signal s -> slab position q of
// slab s (which starts at dword s * ybase).  Outside [0, len) the buffer resource returns zero (a negative offset is a huge unsigned one):
// with the identity map that IS constant padding.  The caller's barrier follows.
template <int THREADS, int NS, class Map>
__device__ __forceinline__ void stft_stage(float* slab, int ybase, const float* const (&sig)[NS], int len, int f0, int nf, const StftGeom& g, int tid, Map map) {
    const int P = (nf - 1) * g.hop + g.n_fft;
    const int g0 = f0 * g.hop - g.n_fft / 2;
    __amdgpu_buffer_rsrc_t rs[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) rs[s] = __builtin_amdgcn_make_buffer_rsrc((void*)sig[s], 0, len * 4, 0x00020000);
    for (int q = tid; q < P; q += THREADS) {
        const int gi = map(g0 + q);
        unsigned v[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) v[s] = __builtin_amdgcn_raw_buffer_load_b32(rs[s], gi * 4, 0, 0);
        const int d = q + (q >> g.ps);
#pragma unroll
        for (int s = 0; s < NS; ++s) slab[s * ybase + d] = __builtin_bit_cast(float, v[s]);
    }
}

// One wave's contraction of its 32 frame columns over the bin blocks c_lo .. c_hi - 1 (32 bins each): epi(c, re, im) receives, once per
// bin block, the fp64 sums of re and of im rounded once to fp32, in accumulator layout (register r = bin 32 c + 8 (r >> 2) + 4 (lane >> 5)
// + (r & 3), frame column lane & 31).  `x` is the slab this lane reads (stftdist: the slab of its signal), abase = column's frame * hop +
// (lane >> 5).  (The epilogue takes the rounded vectors BY VALUE, not dre / dim: with the fp64 arrays in its reach the compiler pairs re
// and im of an epilogue's interleaved stores back through the fp64 adds and moves them behind the next fetch: LABNOTES.md, 2026-10-19.)
//
// One super-group = 16 MFMA steps = 32 samples: eight 16-byte fragments per lane (re of steps 0-3, .., 12-15, then im).  Two register
// buffers take turns: while one is contracted (2048 MFMA cycles) the next super-group — of the next bin block behind this one's last — is on
// its way from L2.  The launcher hands out a multiple of four super-groups per bin block (sg_lo a multiple of four too), so the turns need no copy.
template <class Epi>
__device__ __forceinline__ void stft_contract(const float4* basis, int SG, int sg_lo, int sg_hi, int c_lo, int c_hi, const float* x, int abase, int ps, int lane, Epi&& epi) {
    auto fetch = [&](float4 (&d)[8], int c, int sg) {
        const float4* s = basis + ((size_t)(c * SG + sg) * 8) * 64 + lane;
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = s[q * 64];
        __builtin_amdgcn_sched_barrier(0);   // the loads go out before the contraction they hide behind
    };
    float4 fa[8], fb[8];
    fetch(fa, c_lo, sg_lo);
#pragma unroll 1
    for (int c = c_lo; c < c_hi; ++c) {
        // Short fp32 chains joined in fp64: every MELSPEC_CHUNK MFMA steps (2 MELSPEC_CHUNK samples) start from zero and their sum goes into an
        // fp64 accumulator (exact next to fp32), rounded to fp32 once per bin block by the epilogue.  An fp32 chain rounds every step at the
        // size of its PARTIAL sum, which next to a strong harmonic or an offset is tens of times the final value; a
        // chain of a few samples never gets there.  The order stays fixed: chunks in k order.
        double dre[16], dim[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) dre[r] = dim[r] = 0.0;
        auto contract = [&](const float4 (&w)[8], int sg) {
            const int a0 = abase + 32 * sg;
#pragma unroll
            for (int ch = 0; ch < 16 / MELSPEC_CHUNK; ++ch) {
                stft_f32x16 re, im;
#pragma unroll
                for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
#pragma unroll
                for (int jj = 0; jj < MELSPEC_CHUNK; ++jj) {
                    const int j = ch * MELSPEC_CHUNK + jj, a = a0 + 2 * j;
                    const float v = x[a + (a >> ps)];
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j >> 2][j & 3], v, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(w[4 + (j >> 2)][j & 3], v, im, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    dre[r] += (double)re[r];
                    dim[r] += (double)im[r];
                }
            }
        };
#pragma unroll 1
        for (int sg = sg_lo; sg < sg_hi; sg += 4) {
            fetch(fb, c, sg + 1);
            contract(fa, sg);
            fetch(fa, c, sg + 2);
            contract(fb, sg + 1);
            fetch(fb, c, sg + 3);
            contract(fa, sg + 2);
            const bool wrap = sg + 4 == sg_hi;
            fetch(fa, wrap ? (c + 1 < c_hi ? c + 1 : c) : c, wrap ? sg_lo : sg + 4);
            contract(fb, sg + 3);
        }
        stft_f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            re[r] = (float)dre[r];
            im[r] = (float)dim[r];
        }
        epi(c, re, im);
    }
}

} // namespace dtts
