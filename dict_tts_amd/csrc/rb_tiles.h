// What the fused vocoder kernels (rblock.hip, rb2x.hip, rbn.hip, vpair.hip) share around their contractions: the persistent workgroups' tile
// table, what a finished row does with the stage sum, the fused conv_post + tanh with the always-on non-finite detector, and the launchers'
// per-device plumbing.  The parameter structs stay per kernel (their field order reaches the scalar argument loads): the helpers take plain arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "rb_common.h"

namespace dtts {

// ---- the tile table.  The valid tiles of a batch (ceil(len_b / TTo) per utterance, TTo = the rows a tile steps by) are numbered through; workgroup w
// takes tiles w, w + G, ... or — dynamic claiming — its first tile w and then whatever a device counter hands out.  In LDS at `pre`:
//   [0, B]: prefix sums of the tile counts | [B + 1, 2 B]: the counts | [2 B + 1, 3 B]: the lengths (no global load between two tiles) | [3 B + 1]: the claimed tile
struct RbTiles {
    int* pre;
    int B;
    __device__ __forceinline__ void build(const int* lens, int T, int TTo, int tid, int THREADS) const {
        for (int i = tid; i < B; i += THREADS) {
            const int l = lens ? lens[i] : T;
            pre[B + 1 + i] = (l + TTo - 1) / TTo;
            pre[2 * B + 1 + i] = l;
        }
        __syncthreads();
        for (int i = tid; i <= B; i += THREADS) {
            int a = 0;
            for (int u = 0; u < i; ++u) a += pre[B + 1 + u];
            pre[i] = a;
        }
        __syncthreads();
    }
    __device__ __forceinline__ int total() const { return pre[B]; }
    // tile j -> its utterance: the index only ever moves forward
    __device__ __forceinline__ void locate(int j, int& b) const {
        while (pre[b + 1] <= j) ++b;
        b = __builtin_amdgcn_readfirstlane(b);
    }
    // (readfirstlane: a length in a VGPR would put every buffer resource made from it in VGPRs: a waterfall loop around each buffer access)
    __device__ __forceinline__ int len_of(int b) const { return __builtin_amdgcn_readfirstlane(pre[2 * B + 1 + b]); }
    __device__ __forceinline__ int first_row(int j, int b, int TTo) const { return (j - pre[b]) * TTo; }
    // dynamic claiming: tiles 0 .. G - 1 are the workgroups' first tiles, the counter hands out G, G + 1, ...  One lane publishes its claim, everyone
    // reads it behind a workgroup barrier
    __device__ __forceinline__ void publish_claim(int G, unsigned claim) const { pre[3 * B + 1] = G + (int)claim; }
    __device__ __forceinline__ int claimed() const { return __builtin_amdgcn_readfirstlane(pre[3 * B + 1]); }
};

// ---- a finished row's four channels xs (the stage sum with this ResBlock added: xs += resblock(x), hifigan.py:133-135) leave: / div in mode 2, the
// fp32 store unless the stage's consumers read only the bf16 copy (drop_S), and that copy — leaky_relu, at half the byte offset.  `off` is a byte
// offset into rs_s or 0x80000000 (out of range: dropped).  cached: the sum is re-read by this workgroup's next ResBlock (rblock's fused-stage
// launches): write-back cached; everything else streams out.
template <class RS>
__device__ __forceinline__ void rb_stage_row(f32x4 o, RS rs_s, RS rs_a, int off, int mode, float div, float slope, bool drop_S, bool has_Sa, bool cached) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    if (mode == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] / div;
    }
    if (!(mode == 2 && has_Sa && drop_S)) {
        if (cached) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_s, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs_s, off, 0, VP_ST_AUX);
    }
    if (mode == 2 && has_Sa) {
        const u32x2 pk = {pack2bf(lrelu(o[0], slope), lrelu(o[1], slope)), pack2bf(lrelu(o[2], slope), lrelu(o[3], slope))};
        __builtin_amdgcn_raw_buffer_store_b64(pk, rs_a, off == (int)0x80000000 ? off : off >> 1, 0, VP_ST_AUX);
    }
}

// ---- wav[t] = tanh(b + sum_{tap, c} w[c][tap] * otile[t + tap - 3][c])   (conv_post + tanh, hifigan.py:139-141) in exact fp32, over the fp32 stage
// output a tile left in LDS: otile[TTo + 6 rows][C], output o of the tile = global sample t0 + 3 + o.  The caller's barrier orders the tile's writes.
// C / 4 lanes per output sample (4 channels each, 7 taps), partial sums joined by xor-shuffles.  Each group of lanes slides over PR consecutive
// outputs (PR + 6 row reads instead of 7 PR; PR odd: neighbouring groups start 128 B apart modulo the 256 B of the LDS banks at C = 32); every output
// is summed tap by tap in the order of the one-output form, in explicit operations: the same rounding sequence for every sample, whatever its place
// in a group or a tile, and whatever PR.  (rbn.hip keeps a local one-output copy of this function: see there.)
template <int C, int THREADS, int PR>
__device__ __forceinline__ void rb_conv_post_tanh(const char* otile, const float* post_w, const float* post_b, float* wav_row, int t0, int TTo, int len,
                                                  unsigned* bad, int tid) {
    constexpr int PK = 7, PH = (PK - 1) / 2, LPO = C / 4, OP = C * 4;
    static_assert(LPO == 8 || LPO == 4 || LPO == 2, "the lanes of a sample are joined inside a wave");
    const int q = tid % LPO, rr = tid / LPO;                       // channel quad, group within a pass of THREADS / LPO groups
    f32x4 wq[PK];
#pragma unroll
    for (int k = 0; k < PK; ++k) wq[k] = *(const f32x4*)(post_w + k * C + q * 4);
    const float pb = post_b[0];
    for (int o0 = 0; o0 < TTo; o0 += (THREADS / LPO) * PR) {
        const int ob = o0 + rr * PR;                               // first output of this group: otile rows ob .. ob + PR + PK - 2
        float a[PR];
#pragma unroll
        for (int i = 0; i < PR; ++i) a[i] = 0.f;
        if (ob < TTo) {
#pragma unroll
            for (int j = 0; j < PR + PK - 1; ++j) {
                const int row = ob + j < TTo + PK - 1 ? ob + j : TTo + PK - 2;   // (rows past the tile feed discarded outputs only)
                const f32x4 v = *(const f32x4*)(otile + (size_t)row * OP + q * 16);
#pragma unroll
                for (int i = 0; i < PR; ++i) {
                    const int k = j - i;
                    if (k >= 0 && k < PK) {
                        const float d = __builtin_fmaf(v[3], wq[k][3], __builtin_fmaf(v[2], wq[k][2], __builtin_fmaf(v[1], wq[k][1], __fmul_rn(v[0], wq[k][0]))));
                        a[i] = __fadd_rn(a[i], d);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PR; ++i) {
            a[i] += __shfl_xor(a[i], 1, 64);
            if constexpr (LPO >= 4) a[i] += __shfl_xor(a[i], 2, 64);
            if constexpr (LPO >= 8) a[i] += __shfl_xor(a[i], 4, 64);
        }
        // ALWAYS-ON overflow detector (every instantiation, every call): an fp16 operand that overflowed anywhere upstream is +-inf, every
        // sum it enters is inf / NaN from there on (the fp32 residual stream never recovers), so it arrives HERE as a non-finite
        // pre-tanh value.  tanh would turn +-inf into a plausible +-1: the sample is poisoned with NaN instead and counted.
        // tanh(x) = 1 - 2 / (e^{2x} + 1) on the hardware exp2 / rcp, evaluated by every lane (libm's tanhf ran its ~45 instructions for
        // the one live lane of a group): absolute error <= 3e-7 (1 / 100 of an int16 step), saturates correctly at +-1.
        float pre[PR], th[PR];
        int nf = 0;   // non-finite SAMPLES of this group (the same unit as vconv.hip's post_tanh detector: dtts_vocoder_nonfinite counts samples)
#pragma unroll
        for (int i = 0; i < PR; ++i) {
            pre[i] = a[i] + pb;
            th[i] = __builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(__fadd_rn(__builtin_amdgcn_exp2f(pre[i] * 2.885390081777927f), 1.f)), 1.f);   // (2 log2 e)
        }
        if (q == 0) {
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int o = ob + i, t = t0 + PH + o;
                const bool nonfin = !(__builtin_fabsf(pre[i]) <= 3.0e38f);
                if (o < TTo && t < len) {
                    wav_row[t] = nonfin ? __builtin_nanf("") : th[i];
                    nf += nonfin ? 1 : 0;
                }
            }
            if (nf && bad) atomicAdd(bad, (unsigned)nf);   // (never on a healthy call)
        }
    }
}

// ---- host side: what every launcher of these kernels does per device
inline size_t rb_table_bytes(int B) { return (size_t)(3 * B + 2) * sizeof(int); }   // RbTiles' layout: the only place that knows its size

// compute units of the current device (cached per device), or 0 when the device cannot be queried
inline int rb_device_cus() {
    static int cus_dev[64] = {};
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    int& cus = cus_dev[cur_dev & 63];
    if (!cus) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cur_dev) != hipSuccess) return 0;
        cus = prop.multiProcessorCount;
    }
    return cus;
}

// lets KERN take up to 160 KB of dynamic LDS: once per kernel and device (hipFuncSetAttribute is per device; a process may hold contexts on several GPUs)
template <auto KERN>
inline hipError_t rb_allow_full_lds() {
    static bool configured_dev[64] = {};
    int cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    bool& configured = configured_dev[cur_dev & 63];
    if (!configured) {
        const hipError_t e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        configured = true;
    }
    return hipSuccess;
}

// persistent workgroups: as many as are RESIDENT at once — by LDS, by threads and by the kernel's register bound (by_regs workgroups per CU) — never
// more than there can be tiles.  A surplus workgroup would start only when another one ends, and set itself up for a tile or two.
inline int rb_resident_grid(int cus, size_t lds, int threads, int by_regs, long long max_tiles) {
    const int per_cu = std::max(1, std::min({(int)(160 * 1024 / lds), 2048 / threads, by_regs}));
    return (int)std::min<long long>((long long)cus * per_cu, max_tiles);
}

// a configuration that does not fit (hipErrorOutOfMemory: its LDS cannot hold the tile table of this many utterances, or the halo eats its tile)
// falls through to the next one down
#define RB_TRY(call)                                   \
    do {                                               \
        const hipError_t e_ = (call);                  \
        if (e_ != hipErrorOutOfMemory) return e_;      \
    } while (0)

} // namespace dtts
