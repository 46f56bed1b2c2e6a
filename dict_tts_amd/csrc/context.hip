// libdicttts_hip.so — the context's life cycle: configuration, creation, weight loading and finalisation, error text, timers, and the
// red-zone check of the memory-safety mode.  C ABI declared in include/dicttts_hip.h; the subsystems are in vocoder.hip, text2mel.hip,
// text2mel_build.hip, fft_blocks.hip and pack.hip, the types they share in ctx.h.
#include "ctx.h"

using namespace dtts;

// dtts_config.tune_flags (include/dicttts_hip.h).  The library honours only the bits that have a parity / bit-identity test behind them
// (tests/test_gpu_parity.py): 8 prior flow launch by launch on the exact-fp32 kernels, 9 all ResBlocks of a C <= 64 stage in one launch,
// 12 the first two ResBlocks of the C = 32 stage in one launch, 13 two-product fp16 ups.1, 14 512-row tiles for every k at C = 64, 15 the fp32
// inter-iteration stream of the per-iteration ResBlock kernels (round 5's form; default since round 6: fp16).  dtts_create REJECTS every
// other bit (DTTS_E_INVAL) instead of ignoring it.
constexpr int TUNE_RELEASE_MASK = (1 << 8) | (1 << 9) | (1 << 12) | (1 << 13) | (1 << 14) | (1 << 15);

static std::string g_create_err;

// every workspace arena of a context, in the order dtts_debug_check names its zones: creation (the debug flag), destruction and the
// red-zone mode walk this list and nothing else, so an arena that is in it cannot leak or escape the check
static const struct { const char* name; Arena dtts_ctx::*a; } ARENAS[] = {
    {"encode workspace", &dtts_ctx::a_enc},          {"decode workspace", &dtts_ctx::a_dec},
    {"vocoder workspace", &dtts_ctx::a_voc},         {"fft workspace", &dtts_ctx::a_fft},
    {"speaker workspace", &dtts_ctx::a_spk},         {"posterior workspace", &dtts_ctx::a_post},
    {"stft workspace", &dtts_ctx::a_stft},           {"spectral workspace", &dtts_ctx::a_spec},
    {"loss workspace", &dtts_ctx::a_loss},           {"dtw workspace", &dtts_ctx::a_dtw},
    {"pitch workspace", &dtts_ctx::a_pitch},         {"loudness workspace", &dtts_ctx::a_loud},
    {"discriminator workspace", &dtts_ctx::a_disc},  {"speaker encoder workspace", &dtts_ctx::a_spkenc},
    {"mel discriminator workspace", &dtts_ctx::a_meldisc}, {"gloss workspace", &dtts_ctx::a_gloss},
    {"portaspeech workspace", &dtts_ctx::a_ps},      {"portaspeech frame workspace", &dtts_ctx::a_psf}};
constexpr int ARENA_VOC = 2;   // dtts_debug_poke looks at this one first

namespace dtts {

template <class A, int (*F)(dtts_ctx*, const A*, hipStream_t)>
static int as_block(dtts_ctx* h, const void* a, hipStream_t s) {
    return F(h, (const A*)a, s);
}
#define PART(X) DTTS_PART_##X, "DTTS_PART_" #X
#define NO_PART 0, nullptr, nullptr, nullptr, false, nullptr
#define ITEM(X, A, F) DTTS_OUT_##X, as_block<A, F>
#define NO_ITEM 0, nullptr, false

// The parts come in build order; nothing else depends on where a row stands
static const Unit UNITS[] = {
    {PART(ACOUSTIC), "model.", build_acoustic, true, [](const dtts_ctx* h) { return h->acoustic_ready; }, NO_ITEM},
    {PART(VOCODER), "vocoder.", build_vocoder, true, [](const dtts_ctx* h) { return h->vocoder_ready; }, NO_ITEM},
    {PART(FFT), "fft.", build_fft, true, [](const dtts_ctx* h) { return h->fft_ready; }, NO_ITEM},
    {PART(MELSPEC), "melspec.", build_melspec, false, [](const dtts_ctx* h) { return h->melspec_ready; },
     ITEM(MELSPEC, dtts_melspec_args, melspec_forward), false},
    {PART(STFT), "stft.", build_stft, false, [](const dtts_ctx* h) { return !h->stft_plans.empty(); },
     ITEM(STFT_DISTANCE, dtts_stft_args, stft_forward), false},
    {PART(ISTFT), "istft.", build_istft, false, [](const dtts_ctx* h) { return h->istft_ready; },
     ITEM(SPECTRAL, dtts_spectral_args, spectral_forward), false},
    {NO_PART, ITEM(GRIFFIN_LIM, dtts_griffinlim_args, griffin_lim), false},   // runs on the ISTFT part's plan
    {NO_PART, ITEM(LOSSES, dtts_loss_args, losses_forward), false},
    {NO_PART, ITEM(DTW, dtts_dtw_args, dtw_forward), true},
    {NO_PART, ITEM(PITCH, dtts_pitch_args, pitch_forward), true},
    {PART(RESAMPLE), "resample.", build_resample, false, [](const dtts_ctx* h) { return h->resample_ready; },
     ITEM(RESAMPLE, dtts_resample_args, resample_forward), true},
    {NO_PART, ITEM(LOUDNESS, dtts_loudness_args, loudness_forward), true},
    {PART(DISC), "disc.", build_disc, true, [](const dtts_ctx* h) { return h->disc_ready; }, ITEM(DISC, dtts_disc_args, disc_forward), true},
    {PART(SPKENC), "spkenc.", build_spkenc, true, [](const dtts_ctx* h) { return h->spkenc_ready; },
     ITEM(SPKENC, dtts_spkenc_args, spkenc_forward), true},
    {PART(MELDISC), "meldisc.", build_meldisc, true, [](const dtts_ctx* h) { return h->meldisc_ready; },
     ITEM(MELDISC, dtts_meldisc_args, meldisc_forward), true},
    {PART(GLOSS), "gloss.", build_gloss, true, [](const dtts_ctx* h) { return h->gloss_ready; },
     DTTS_GLOSS_ENCODE, as_block<dtts_gloss_args, gloss_forward>, true},   // (an item outside the DTTS_OUT_* numbering: it is no output of an encode)
    {PART(PORTASPEECH), "ps.", build_ps, true, [](const dtts_ctx* h) { return h->ps_ready; },
     DTTS_PS_ENCODE, as_block<dtts_ps_args, ps_forward>, true},             // (the same: it is the baseline's encode itself)
    {NO_PART, DTTS_DICT_EDIT, as_block<dtts_dict_edit_args, dict_edit_forward>, true},      // (the same: they change / read the id path's INPUT,
    {NO_PART, DTTS_DICT_ENTRY, as_block<dtts_dict_entry_args, dict_entry_forward>, true},   //  the resident table; dict_edit.hip)
};
#undef PART
#undef NO_PART
#undef ITEM
#undef NO_ITEM

const Unit* find_item(int what) {
    for (const Unit& u : UNITS)
        if (u.forward && u.out == what) return &u;
    return nullptr;
}

int Block::finalized(int part) const {
    for (const Unit& u : UNITS)
        if (u.part == part) return u.ready(h) ? 0 : fail(h, DTTS_E_STATE, "%s before dtts_finalize_weights(%s)", me, u.part_name);
    return fail(h, DTTS_E_INVAL, "%s: no part 0x%x", me, (unsigned)part);
}

int fail(dtts_ctx* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    else g_create_err = buf;
    return code;
}

} // namespace dtts

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" {

int dtts_config_sizeof(void) { return (int)sizeof(dtts_config); }

void dtts_default_config(dtts_config* c) {
    memset(c, 0, sizeof *c);
    c->hidden_size = 192;
    c->num_heads = 2;
    c->enc_ffn_kernel_size = 5;
    c->enc_layers = 4;
    c->gloss_dim = 768;
    c->word_size = 8000;
    c->value_embedding_size = 185;
    c->n_phone = 6;
    c->audio_num_mel_bins = 80;
    c->latent_size = 16;
    c->fvae_enc_dec_hidden = 192;
    c->fvae_kernel_size = 5;
    c->fvae_dec_n_layers = 4;
    c->fvae_enc_n_layers = 8;
    c->prior_glow_hidden = 64;
    c->glow_kernel_size = 3;
    c->prior_glow_n_blocks = 4;
    c->prior_glow_n_layers = 4;
    c->dur_predictor_layers = 3;
    c->dur_predictor_kernel = 5;
    c->dur_chans = 128;
    c->frames_multiple = 4;
    c->language_zh = 1;
    c->upsample_initial_channel = 512;
    c->n_upsamples = 4;
    const int ur[4] = {8, 8, 2, 2}, uk[4] = {16, 16, 4, 4}, rk[3] = {3, 7, 11};
    for (int i = 0; i < 4; ++i) {
        c->upsample_rates[i] = ur[i];
        c->upsample_kernel_sizes[i] = uk[i];
    }
    c->n_resblock_kernels = 3;
    for (int i = 0; i < 3; ++i) {
        c->resblock_kernel_sizes[i] = rk[i];
        c->resblock_dilation_sizes[i][0] = 1;
        c->resblock_dilation_sizes[i][1] = 3;
        c->resblock_dilation_sizes[i][2] = 5;
    }
    c->vocoder_precision = DTTS_VOC_F16;
    c->fft_layers = 4;
    c->fft_kernel_size = 9;
    c->fft_use_pos_embed = 1;
    c->fft_use_last_norm = 1;
}

int dtts_create(const dtts_config* cfg, dtts_handle* out) {
    if (!cfg || !out) return fail(nullptr, DTTS_E_INVAL, "dtts_create: null argument");
    if (cfg->tune_flags & ~TUNE_RELEASE_MASK)   // (a bit without a test behind it is refused, never silently ignored)
        return fail(nullptr, DTTS_E_INVAL, "dtts_create: tune_flags 0x%x carries bits this library does not honour (supported mask 0x%x)",
                    (unsigned)cfg->tune_flags, (unsigned)TUNE_RELEASE_MASK);
    // the block type of the generator is encoded in the dilation rows (include/dicttts_hip.h): a third entry of 0 = a two-dilation
    // (ResBlock2) row.  All used rows are of one kind
    if (cfg->n_resblock_kernels >= 0 && cfg->n_resblock_kernels <= 4) {
        int two = 0;
        for (int j = 0; j < cfg->n_resblock_kernels; ++j) {
            const int32_t* d = cfg->resblock_dilation_sizes[j];
            if (d[0] < 1 || d[1] < 1 || d[2] < 0)
                return fail(nullptr, DTTS_E_INVAL, "dtts_create: resblock_dilation_sizes[%d] = (%d, %d, %d): the first two dilations must be >= 1, the third >= 1 (ResBlock1) or 0 (ResBlock2)",
                            j, (int)d[0], (int)d[1], (int)d[2]);
            two += d[2] == 0 ? 1 : 0;
        }
        if (two != 0 && two != cfg->n_resblock_kernels)
            return fail(nullptr, DTTS_E_INVAL, "dtts_create: resblock_dilation_sizes mixes two-dilation (ResBlock2, third entry 0) and three-dilation (ResBlock1) rows: "
                        "%d of %d rows have a third entry of 0", two, (int)cfg->n_resblock_kernels);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, DTTS_E_HIP, "dtts_create: no HIP device visible (the HIP path has no CPU fallback)");
    if (cfg->hidden_size % 64 || cfg->hidden_size / cfg->num_heads > 96 || cfg->gloss_dim > 768 || cfg->gloss_dim % 4 ||
        cfg->n_upsamples > 8 || cfg->n_resblock_kernels > 4 || cfg->latent_size % 8 || cfg->prior_glow_hidden % 32 ||
        cfg->fvae_enc_dec_hidden % 32)
        return fail(nullptr, DTTS_E_INVAL, "dtts_create: unsupported configuration");
    dtts_ctx* h = new dtts_ctx();
    h->cfg = *cfg;
    // dtts_config.tune_flags (0 = the measured defaults; bits documented in include/dicttts_hip.h).  The library never reads the environment.
    h->tune = cfg->tune_flags;
    {   // prior-sample seed: different per context, process, device and start time (data-parallel ranks and restarts must not draw the
        // same z_p sequence); dtts_set_noise_seed makes it reproducible
        static unsigned long long instance = 0;
        int dev = 0;
        (void)hipGetDevice(&dev);
        unsigned long long z = (unsigned long long)time(nullptr) * 0x9E3779B97F4A7C15ull ^ ((unsigned long long)getpid() << 32) ^
                               ((unsigned long long)dev << 20) ^ ++instance;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        h->noise_seed = z ^ (z >> 31);
    }
    h->guard_on = cfg->vocoder_range_guard != 0;
    h->resblock2 = cfg->n_resblock_kernels > 0 && cfg->resblock_dilation_sizes[0][2] == 0;
    (void)hipGetDevice(&h->device);
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || h->n_cu <= 0) h->n_cu = 256;
    h->debug_rz = cfg->debug_redzone != 0;
    h->debug_misorder = cfg->debug_redzone == 2;
    for (const auto& a : ARENAS) (h->*a.a).debug = h->debug_rz;
    *out = h;
    return DTTS_OK;
}

void dtts_destroy(dtts_handle h) {
    if (h && h->bad_host) {
        (void)hipDeviceSynchronize();
        (void)hipHostFree((void*)h->bad_host);
        h->bad_host = nullptr;
    }
    if (!h) return;
    (void)hipDeviceSynchronize();
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->amax_bits) (void)hipFree(h->amax_bits);
    for (const auto& a : ARENAS) (h->*a.a).release();
    for (auto& t : h->timers)
        for (auto e : t.pool) (void)hipEventDestroy(e);
    delete h;
}

const char* dtts_last_error(dtts_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int dtts_load_weight(dtts_handle h, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
    if (!h || !name || !host_ptr || ndim < 0 || ndim > 8) return fail(h, DTTS_E_INVAL, "dtts_load_weight: bad argument");
    const bool f64 = dtype == DTTS_F64 && std::string(name).rfind("resample.", 0) == 0;   // the resampler's table keeps its precision
    if (dtype != DTTS_F32 && !f64) return fail(h, DTTS_E_INVAL, "dtts_load_weight(%s): only fp32 tensors are accepted", name);
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    const int64_t n = t.numel();
    if (f64)
        t.d.assign((const double*)host_ptr, (const double*)host_ptr + n);
    else
        t.f.assign((const float*)host_ptr, (const float*)host_ptr + n);
    h->w[name] = std::move(t);
    return DTTS_OK;
}

int dtts_finalize_weights(dtts_handle h, int parts) {
    if (!h) return DTTS_E_INVAL;
    h->err.clear();
    int rc = DTTS_OK, built = 0;   // built: the parts this call (re)built
    for (const Unit& u : UNITS)
        if (rc == DTTS_OK && (parts & u.part) && !(u.once && u.ready(h))) {
            rc = u.build(h);
            built |= u.part;
        }
    if (rc == DTTS_OK)   // host copies are no longer needed for finished parts: those built once, and what this call rebuilt
        for (auto it = h->w.begin(); it != h->w.end();) {
            bool done = false;
            for (const Unit& u : UNITS)
                if (u.part && it->first.rfind(u.prefix, 0) == 0) done = u.once ? u.ready(h) : (built & u.part) != 0;
            it = done ? h->w.erase(it) : std::next(it);
        }
    return rc;
}

// ---- the single-call forms and names of SURVEY.md 8(b)
int dtts_load_weights(dtts_handle h, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
    return dtts_load_weight(h, name, host_ptr, shape, ndim, dtype);
}

int dtts_timer_enable(dtts_handle h, int which) {
    if (!h || which < 1 || which >= DTTS_TIMER_COUNT) return DTTS_E_INVAL;
    h->timers[which].enabled = true;
    return DTTS_OK;
}

static void timer_collect(TimerSlot& t) {
    for (size_t i = 0; i + 1 < t.used; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.pool[i], t.pool[i + 1]) == hipSuccess) t.ms_done += ms;
    }
    t.used = 0;
}

int dtts_timer_read(dtts_handle h, int which, double* ms_total, int64_t* launches) {
    if (!h || which < 1 || which >= DTTS_TIMER_COUNT) return DTTS_E_INVAL;
    HIPCHK(hipDeviceSynchronize());
    TimerSlot& t = h->timers[which];
    timer_collect(t);
    if (ms_total) *ms_total = t.ms_done;
    if (launches) *launches = t.launches;
    return DTTS_OK;
}

int dtts_timer_reset(dtts_handle h) {
    if (!h) return DTTS_E_INVAL;
    HIPCHK(hipDeviceSynchronize());
    for (auto& t : h->timers) {
        t.used = 0;
        t.ms_done = 0;
        t.launches = 0;
    }
    return DTTS_OK;
}

// ---- memory-safety mode (dtts_config.debug_redzone): verify every red zone of the workspaces and the weight packs
namespace {
struct RzZone { const unsigned char* p; unsigned n; unsigned id; };
__global__ void redzone_check_kernel(const RzZone* z, int nz, unsigned long long* out) {   // out[0] = damaged bytes, out[1] = lowest damaged zone id
    const RzZone q = z[blockIdx.x];
    unsigned bad = 0;
    for (unsigned i = threadIdx.x; i < q.n; i += blockDim.x) bad += q.p[i] != 0xFF ? 1u : 0u;
    if (bad) {
        atomicAdd(out, (unsigned long long)bad);
        atomicMin(out + 1, (unsigned long long)q.id);
    }
}
} // namespace

// harness self-test: damage ONE red-zone byte (the first byte after the first buffer of the first workspace in use, or after the first
// weight pack) the way an off-by-one store of a kernel would, so that a test can show dtts_debug_check notices
int dtts_debug_poke(dtts_handle h, dtts_stream stream) {
    if (!h) return DTTS_E_INVAL;
    if (!h->debug_rz) return fail(h, DTTS_E_STATE, "dtts_debug_poke: the context was not created with dtts_config.debug_redzone = 1");
    char* target = nullptr;
    for (int i = -1; i < (int)(sizeof ARENAS / sizeof ARENAS[0]); ++i) {   // the vocoder's first, then in the list's order
        const Arena& a = h->*ARENAS[i < 0 ? ARENA_VOC : i].a;
        if (!target && a.base && !a.bufs.empty()) target = a.base + a.bufs[0].start + a.bufs[0].bytes;
    }
    if (!target && !h->rz_static.empty()) target = h->rz_static[0].p + h->rz_static[0].bytes;
    if (!target) return fail(h, DTTS_E_STATE, "dtts_debug_poke: nothing allocated yet");
    HIPCHK(hipMemsetAsync(target, 0, 1, (hipStream_t)stream));
    return DTTS_OK;
}

int dtts_debug_check(dtts_handle h, int64_t* damaged_bytes, dtts_stream stream) {
    if (!h || !damaged_bytes) return DTTS_E_INVAL;
    *damaged_bytes = -1;
    if (!h->debug_rz) return fail(h, DTTS_E_STATE, "dtts_debug_check: the context was not created with dtts_config.debug_redzone = 1");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(s));
    std::vector<RzZone> zones;
    std::vector<std::string> names;
    auto zone = [&](const char* p0, size_t n, const std::string& name) {
        if (!n) return;
        zones.push_back({(const unsigned char*)p0, (unsigned)n, (unsigned)names.size()});
        names.push_back(name);
    };
    for (const auto& a : ARENAS) {
        const Arena& arena = h->*a.a;
        const auto& bufs = arena.bufs;
        const char* base = arena.base;
        for (size_t i = 0; i < bufs.size(); ++i) {   // layout: [RZ][buffer 0][slack to 256 B][RZ][buffer 1]...[RZ .. up to the arena's end]
            const std::string me = std::string(a.name) + " buffer #" + std::to_string(i) + " (" + std::to_string(bufs[i].bytes) + " B)";
            const size_t end = bufs[i].start + bufs[i].bytes, padded_end = bufs[i].start + ((bufs[i].bytes + 255) & ~(size_t)255);
            zone(base + bufs[i].start - RZ, RZ, i ? "AFTER " + std::string(a.name) + " buffer #" + std::to_string(i - 1) + " / BEFORE " + me : "BEFORE " + me);
            zone(base + end, padded_end - end, "AFTER " + me + " (alignment slack)");
            if (i + 1 == bufs.size()) zone(base + padded_end, std::min(RZ, arena.cap - padded_end), "AFTER " + me);
        }
    }
    for (size_t i = 0; i < h->rz_static.size(); ++i) {
        const auto& b = h->rz_static[i];
        const size_t padded = (b.bytes + 255) & ~(size_t)255;
        const std::string me = "weight pack / table #" + std::to_string(i) + " (" + std::to_string(b.bytes) + " B)";
        zone(b.p - RZ, RZ, "BEFORE " + me);
        zone(b.p + b.bytes, padded + RZ - b.bytes, "AFTER " + me);
    }
    if (zones.empty()) {
        *damaged_bytes = 0;
        return DTTS_OK;
    }
    RzZone* dz = nullptr;
    unsigned long long* dout = nullptr;
    unsigned long long hout[2] = {0ull, ~0ull};
    HIPCHK(hipMalloc((void**)&dz, zones.size() * sizeof(RzZone)));
    hipError_t e = hipMalloc((void**)&dout, sizeof hout);
    if (e == hipSuccess) e = hipMemcpy(dz, zones.data(), zones.size() * sizeof(RzZone), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dout, hout, sizeof hout, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(redzone_check_kernel, dim3((unsigned)zones.size()), dim3(256), 0, s, dz, (int)zones.size(), dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(hout, dout, sizeof hout, hipMemcpyDeviceToHost);
    (void)hipFree(dz);
    if (dout) (void)hipFree(dout);
    if (e != hipSuccess) return fail(h, DTTS_E_HIP, "dtts_debug_check: %s", hipGetErrorString(e));
    *damaged_bytes = (int64_t)hout[0];
    if (hout[0]) h->err = "red zone damaged: " + std::to_string(hout[0]) + " bytes in " + std::to_string(zones.size()) + " zones; first: " +
                          (hout[1] < names.size() ? names[hout[1]] : std::string("?"));
    return DTTS_OK;
}

} // extern "C"
