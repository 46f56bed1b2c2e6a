// libdicttts_hip.so — editing the resident dictionary table in place (dict_edit.h): the segment-copy kernel, DTTS_DICT_EDIT (replace and
// append entries: project only the new rows, move everything else on the device) and DTTS_DICT_ENTRY (read an entry back).  The table itself
// and its upload are in text2mel.hip; the S2PA kernels that read it (ops.hip) are untouched: the CSR layout t_off[e] .. t_off[e + 1] stays.
#include "ctx.h"

using namespace dtts;

namespace {

// A pure streaming kernel: a workgroup owns DICT_SEG_TILE consecutive elements of the NEW array, lane after lane (coalesced, 16 B per lane in
// the K / V instantiation), finds the segment of its first element once (uniform) and walks the list forward from there: within a tile the
// elements ascend, so does their segment.  All loads of a lane are issued before its stores; no LDS.  The host built the list so that every
// source index lies inside its source array (dict_edit_forward: segments()).
template <class T>
__global__ __launch_bounds__(256) void dict_seg_copy_kernel(const T* __restrict__ old, const T* __restrict__ staging, T* __restrict__ out,
                                                            const DictSeg* __restrict__ segs, int n_seg, int width, long long total) {
    const long long tile0 = (long long)blockIdx.x * DICT_SEG_TILE;
    int lo = 0, hi = n_seg - 1;   // the last segment that starts at or before tile0 (segs[0].dst == 0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)segs[mid].dst * width <= tile0) lo = mid;
        else hi = mid - 1;
    }
    int s = lo;
    auto locate = [&](long long i) -> const T* {   // where element i of the new array comes from (null past the end)
        if (i >= total) return nullptr;
        while (s + 1 < n_seg && (long long)segs[s + 1].dst * width <= i) ++s;
        const DictSeg q = segs[s];
        return (q.staged ? staging : old) + ((long long)q.src * width + (i - (long long)q.dst * width));
    };
    static_assert(DICT_SEG_UNROLL == 4, "four named values: an indexed array of them would be placed in LDS");
    const long long i0 = tile0 + threadIdx.x, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
    // the (cached) list reads of all four elements first: the four streaming loads are then in flight together
    const T *p0 = locate(i0), *p1 = locate(i1), *p2 = locate(i2), *p3 = locate(i3);
    T v0, v1, v2, v3;
    if (p0) v0 = *p0;
    if (p1) v1 = *p1;
    if (p2) v2 = *p2;
    if (p3) v3 = *p3;
    if (i0 < total) out[i0] = v0;
    if (i1 < total) out[i1] = v1;
    if (i2 < total) out[i2] = v2;
    if (i3 < total) out[i3] = v3;
}

template <class T>
hipError_t seg_copy(const void* old, const void* staging, void* out, const DictSeg* segs, int n_seg, int width, long long total, hipStream_t s) {
    const long long blocks = (total + DICT_SEG_TILE - 1) / DICT_SEG_TILE;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dict_seg_copy_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, (const T*)old, (const T*)staging, (T*)out, segs, n_seg, width,
                       total);
    return hipGetLastError();
}

} // namespace

namespace dtts {

hipError_t dict_seg_copy_launch(int elem_bytes, const void* old, const void* staging, void* new_, const DictSeg* segs_dev, int n_seg, int width,
                                long long total_rows, hipStream_t stream) {
    if (total_rows <= 0 || n_seg <= 0) return hipSuccess;
    const long long total = total_rows * width;
    switch (elem_bytes) {
        case 16: return seg_copy<uint4>(old, staging, new_, segs_dev, n_seg, width, total, stream);
        case 8: return seg_copy<unsigned long long>(old, staging, new_, segs_dev, n_seg, width, total, stream);
        case 4: return seg_copy<unsigned>(old, staging, new_, segs_dev, n_seg, width, total, stream);
        default: return hipErrorInvalidValue;
    }
}

int dict_edit_forward(dtts_ctx* h, const dtts_dict_edit_args* a, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_DICT_EDIT)";
    const Block blk{h, me};
    // h may be null: the block is checked first, so that the refusals are reachable without a device
    if (!a) return fail(h, DTTS_E_INVAL, "%s: null argument block", me);
    if (int rc = blk.size(a->size, sizeof *a)) return rc;
    const int n = a->n_edit;
    if (n < 0) return fail(h, DTTS_E_INVAL, "%s: n_edit = %d", me, n);
    if (a->rows_on_device != 0 && a->rows_on_device != 1) return fail(h, DTTS_E_INVAL, "%s: rows_on_device = %d (0 = host rows, 1 = device rows)", me, a->rows_on_device);
    const int32_t *id = a->entry_id_host, *eo = a->tok_off_host, *ep = a->pin_off_host;
    std::vector<int> epm((size_t)n, 0);   // the largest pinyin_map value per edited entry (t_pmmax)
    if (n > 0) {
        if (!id || !eo || !ep) return fail(h, DTTS_E_INVAL, "%s: null entry_id_host / tok_off_host / pin_off_host", me);
        for (int i = 0; i < n; ++i)
            if (id[i] < 0 || (i && id[i] <= id[i - 1]))
                return fail(h, DTTS_E_INVAL, "%s: entry ids must be non-negative and strictly ascending (entry_id[%d] = %d%s)", me, i, id[i],
                            i ? (" after " + std::to_string(id[i - 1])).c_str() : "");
        if (eo[0] != 0 || ep[0] != 0) return fail(h, DTTS_E_INVAL, "%s: tok_off[0] = %d, pin_off[0] = %d (must be 0)", me, eo[0], ep[0]);
        for (int i = 0; i < n; ++i)
            if (eo[i + 1] < eo[i] || ep[i + 1] < ep[i]) return fail(h, DTTS_E_INVAL, "%s: offsets must be non-decreasing (edit %d, entry %d)", me, i, id[i]);
        if (eo[n] > INT_MAX / 2 || ep[n] > INT_MAX / 2) return fail(h, DTTS_E_INVAL, "%s: %d gloss rows, %d pinyin slots (at most %d)", me, eo[n], ep[n], INT_MAX / 2);
        if ((eo[n] && (!a->keys || !a->key_map_host)) || (ep[n] && (!a->pinyin_host || !a->pinyin_map_host)))
            return fail(h, DTTS_E_INVAL, "%s: null keys / key_map_host / pinyin_host / pinyin_map_host", me);
        for (int i = 0; i < n; ++i) {
            for (int p = ep[i]; p < ep[i + 1]; ++p) epm[i] = std::max(epm[i], (int)a->pinyin_map_host[p]);
            float km = 0.f;
            for (int l = eo[i]; l < eo[i + 1]; ++l) km = std::max(km, a->key_map_host[l]);
            if (epm[i] > DTTS_MAX_SENSES || km > (float)DTTS_MAX_SENSES)
                return fail(h, DTTS_E_INVAL, "%s: entry %d has sense index %d; at most %d senses per word are supported", me, id[i],
                            std::max(epm[i], (int)km), DTTS_MAX_SENSES);
        }
        if (a->rows_on_device)
            if (int rc = blk.aligned(16, {{"keys", a->keys}, {"values", a->values}})) return rc;
    }
    if (int rc = blk.handle()) return rc;
    if (int rc = blk.finalized(DTTS_PART_ACOUSTIC)) return rc;
    if (!h->t_entries) return fail(h, DTTS_E_STATE, "%s before dtts_dict_table_upload: no table is resident", me);
    if (n == 0) return DTTS_OK;

    // ---- the plan, on the host: which entry comes from where, the new offsets, the segments
    const int n_old = h->t_entries;
    int n_rep = 0;
    while (n_rep < n && id[n_rep] < n_old) ++n_rep;
    for (int i = n_rep; i < n; ++i)
        if (id[i] != n_old + (i - n_rep))
            return fail(h, DTTS_E_INVAL, "%s: entry_id[%d] = %d leaves a gap: the table holds %d entries, so appended ids continue at %d", me, i, id[i],
                        n_old, n_old + (i - n_rep));
    const int n_new = n_old + (n - n_rep);
    const std::vector<int>&oo = h->m_off, &op = h->m_poff;
    std::vector<int> which((size_t)n_new, -1), no((size_t)n_new + 1), np((size_t)n_new + 1), nm((size_t)n_new);
    for (int i = 0; i < n; ++i) which[id[i]] = i;
    long long r = 0, q = 0;
    for (int e = 0; e < n_new; ++e) {
        const int i = which[e];
        no[e] = (int)r;
        np[e] = (int)q;
        r += i >= 0 ? eo[i + 1] - eo[i] : oo[e + 1] - oo[e];
        q += i >= 0 ? ep[i + 1] - ep[i] : op[e + 1] - op[e];
        nm[e] = i >= 0 ? epm[i] : h->m_pmmax[e];
        if (r > INT_MAX / 2 || q > INT_MAX / 2)
            return fail(h, DTTS_E_INVAL, "%s: the edited table would hold more than %d gloss rows or pinyin slots", me, INT_MAX / 2);
    }
    no[n_new] = (int)r;
    np[n_new] = (int)q;
    // old entries between two edited ones are one run; neighbouring edited entries are neighbours in the staging array too
    auto segments = [&](const std::vector<int>& o, const int32_t* s, const std::vector<int>& d) {
        std::vector<DictSeg> out;
        for (int e = 0; e < n_new;) {
            if (which[e] < 0) {
                int e1 = e;
                while (e1 < n_new && which[e1] < 0) ++e1;   // (appended entries all have an edit: e1 <= n_old)
                if (o[e1] > o[e]) out.push_back({d[e], o[e], o[e1] - o[e], 0});
                e = e1;
            } else {
                const int i = which[e], rows = s[i + 1] - s[i];
                if (rows && !out.empty() && out.back().staged && out.back().src + out.back().rows == s[i]) out.back().rows += rows;
                else if (rows) out.push_back({d[e], s[i], rows, 1});
                ++e;
            }
        }
        return out;
    };
    const std::vector<DictSeg> rs = segments(oo, eo, no), ps = segments(op, ep, np);
    // the kernel indexes by these lists alone: a list must tile the new array exactly and stay inside both sources, or nothing is launched
    auto tiles = [](const std::vector<DictSeg>& segs, int n_old_rows, int n_staged_rows, int n_new_rows) {
        long long at = 0;
        for (const DictSeg& g : segs) {
            if (g.dst != at || g.rows <= 0 || g.src < 0 || (long long)g.src + g.rows > (g.staged ? n_staged_rows : n_old_rows)) return false;
            at += g.rows;
        }
        return at == n_new_rows;
    };
    if (!tiles(rs, oo[n_old], eo[n], no[n_new]) || !tiles(ps, op[n_old], ep[n], np[n_new]))
        return fail(h, DTTS_E_STATE, "%s: internal error: the segment lists do not tile the edited table; the previous table stays in use", me);

    // ---- build the NEW table beside the one in use; a failure below releases it again and leaves the previous table working
    int dev_cur = -1;
    (void)hipGetDevice(&dev_cur);
    if (dev_cur != h->device) return fail(h, DTTS_E_STATE, "%s: the current HIP device is %d, the context was created on device %d", me, dev_cur, h->device);
    const int C = h->cfg.hidden_size, D = h->cfg.gloss_dim;
    const size_t sL = (size_t)eo[n], sP = (size_t)ep[n], nL = (size_t)no[n_new], nP = (size_t)np[n_new];
    std::vector<void*> fresh, temps;   // the new table's arrays (context-owned); what only this call needs
    const char* what = nullptr;
    hipError_t herr = hipSuccess;
    auto table = [&](size_t bytes) -> void* {
        void* d = what ? nullptr : dev_alloc(h, bytes);
        if (d) fresh.push_back(d);
        else if (!what) what = "device allocation";
        return d;
    };
    auto temp = [&](size_t bytes) -> void* {
        void* d = nullptr;
        if (what || !bytes) return nullptr;
        if ((herr = hipMalloc(&d, bytes)) != hipSuccess) {
            what = "staging buffer allocation";
            return nullptr;
        }
        temps.push_back(d);
        return d;
    };
    auto put = [&](void* dst, const void* src, size_t bytes) {   // host -> device on the call's stream (the host arrays outlive the call's last sync)
        if (!what && dst && bytes && (herr = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) what = "host-to-device copy";
    };
    int* n_off = (int*)table(sizeof(int) * ((size_t)n_new + 1));
    int* n_poff = (int*)table(sizeof(int) * ((size_t)n_new + 1));
    int* n_pmmax = (int*)table(sizeof(int) * (size_t)n_new);
    float* n_keys = (float*)table(nL * C * sizeof(float));
    float* n_values = (float*)table(nL * C * sizeof(float));
    float* n_key_map = (float*)table(nL * sizeof(float));
    int64_t* n_pinyin = (int64_t*)table(nP * sizeof(int64_t));
    int64_t* n_pinyin_map = (int64_t*)table(nP * sizeof(int64_t));
    float* raw = a->rows_on_device ? nullptr : (float*)temp(sL * D * sizeof(float));
    float* pk = (float*)temp(sL * C * sizeof(float));
    float* pv = (float*)temp(sL * C * sizeof(float));
    float* s_km = (float*)temp(sL * sizeof(float));
    int64_t* s_py = (int64_t*)temp(sP * sizeof(int64_t));
    int64_t* s_pm = (int64_t*)temp(sP * sizeof(int64_t));
    DictSeg* d_rs = (DictSeg*)temp(rs.size() * sizeof(DictSeg));
    DictSeg* d_ps = (DictSeg*)temp(ps.size() * sizeof(DictSeg));
    put(n_off, no.data(), sizeof(int) * ((size_t)n_new + 1));
    put(n_poff, np.data(), sizeof(int) * ((size_t)n_new + 1));
    put(n_pmmax, nm.data(), sizeof(int) * (size_t)n_new);
    put(s_km, a->key_map_host, sL * sizeof(float));
    put(s_py, a->pinyin_host, sP * sizeof(int64_t));
    put(s_pm, a->pinyin_map_host, sP * sizeof(int64_t));
    put(d_rs, rs.data(), rs.size() * sizeof(DictSeg));
    put(d_ps, ps.data(), ps.size() * sizeof(DictSeg));
    // only the new rows are projected, by the upload's two launches (text2mel.hip): a conv1d row depends neither on its position nor on the row
    // count (these 1x1 layers always run on the three-piece short kernel, whose summation order is fixed by the layer: conv1d.hip)
    auto project = [&](const float* src, const PackedConv& L, float* out) {
        if (what || !sL) return;
        ConvParams p = base_params(src, D, 1, (int)sL, (int)sL, out, C);
        if ((herr = conv1d_launch(L, p, stream)) != hipSuccess) what = "projection kernel launch";
    };
    const float* src_k = a->rows_on_device ? a->keys : raw;
    put(raw, a->keys, sL * D * sizeof(float));
    project(src_k, h->s2_k, pk);
    const float* src_v = src_k;   // values == NULL: the keys, as in the upload
    if (a->values && a->rows_on_device) src_v = a->values;
    else if (a->values) put(raw, a->values, sL * D * sizeof(float));   // (stream order: behind the K projection that read raw)
    project(src_v, h->s2_v, pv);
    auto move = [&](int elem_bytes, const void* old, const void* stg, void* out, const std::vector<DictSeg>& segs, const DictSeg* dsegs, int width, size_t total) {
        if (!what && (herr = dict_seg_copy_launch(elem_bytes, old, stg, out, dsegs, (int)segs.size(), width, (long long)total, stream)) != hipSuccess)
            what = "segment-copy kernel launch";
    };
    {
        Timed tm(h, DTTS_TIMER_DICT_SEG_COPY, stream);
        move(16, h->t_keys, pk, n_keys, rs, d_rs, C / 4, nL);
    }
    move(16, h->t_values, pv, n_values, rs, d_rs, C / 4, nL);
    move(4, h->t_key_map, s_km, n_key_map, rs, d_rs, 1, nL);
    move(8, h->t_pinyin, s_py, n_pinyin, ps, d_ps, 1, nP);
    move(8, h->t_pinyin_map, s_pm, n_pinyin_map, ps, d_ps, 1, nP);
    // the one device synchronisation: the new arrays are complete, and nothing may still be using the previous ones when they are released
    const hipError_t serr = hipDeviceSynchronize();
    if (!what && serr != hipSuccess) {
        herr = serr;
        what = "hipDeviceSynchronize";
    }
    for (void* t : temps) (void)hipFree(t);
    if (what) {
        for (void* f : fresh) dev_free(h, f);
        return fail(h, strstr(what, "allocation") ? DTTS_E_NOMEM : DTTS_E_HIP, "%s: %s failed (%s); the previous table stays in use", me, what,
                    hipGetErrorString(herr));
    }
    void* old[] = {h->t_off, h->t_poff, h->t_pmmax, h->t_keys, h->t_values != h->t_keys ? h->t_values : nullptr, h->t_key_map, h->t_pinyin, h->t_pinyin_map};
    for (void* o : old) dev_free(h, o);
    h->t_off = n_off;
    h->t_poff = n_poff;
    h->t_pmmax = n_pmmax;
    h->t_keys = n_keys;
    h->t_values = n_values;
    h->t_key_map = n_key_map;
    h->t_pinyin = n_pinyin;
    h->t_pinyin_map = n_pinyin_map;
    h->t_entries = n_new;
    h->m_off = std::move(no);
    h->m_poff = std::move(np);
    h->m_pmmax = std::move(nm);
    return DTTS_OK;
}

int dict_entry_forward(dtts_ctx* h, const dtts_dict_entry_args* ca, hipStream_t stream) {
    const char* me = "dtts_text2mel_fetch(DTTS_DICT_ENTRY)";
    const Block blk{h, me};
    if (!ca) return fail(h, DTTS_E_INVAL, "%s: null argument block", me);
    if (int rc = blk.size(ca->size, sizeof *ca)) return rc;
    if (ca->entry < -1) return fail(h, DTTS_E_INVAL, "%s: entry = %d (an entry id, or -1 for the count alone)", me, ca->entry);
    if (int rc = blk.aligned(4, {{"k_dev", ca->k_dev}, {"v_dev", ca->v_dev}, {"key_map_dev", ca->key_map_dev}})) return rc;
    if (int rc = blk.aligned(8, {{"pinyin_dev", ca->pinyin_dev}, {"pinyin_map_dev", ca->pinyin_map_dev}})) return rc;
    if (int rc = blk.handle()) return rc;
    dtts_dict_entry_args* a = const_cast<dtts_dict_entry_args*>(ca);   // (the dispatcher hands every block over as const; this one has out fields)
    a->n_entries = h->t_entries;
    a->L_e = a->P_e = 0;
    const int e = a->entry;
    if (e < 0) return DTTS_OK;
    if (!h->t_entries) return fail(h, DTTS_E_STATE, "%s before dtts_dict_table_upload: no table is resident", me);
    if (e >= h->t_entries) return fail(h, DTTS_E_INVAL, "%s: entry = %d, the table holds %d entries", me, e, h->t_entries);
    const size_t C = (size_t)h->cfg.hidden_size, l0 = (size_t)h->m_off[e], p0 = (size_t)h->m_poff[e];
    const size_t L = (size_t)h->m_off[e + 1] - l0, P = (size_t)h->m_poff[e + 1] - p0;
    a->L_e = (int32_t)L;
    a->P_e = (int32_t)P;
    if (a->k_dev && L) HIPCHK(hipMemcpyAsync(a->k_dev, h->t_keys + l0 * C, L * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (a->v_dev && L) HIPCHK(hipMemcpyAsync(a->v_dev, h->t_values + l0 * C, L * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (a->key_map_dev && L) HIPCHK(hipMemcpyAsync(a->key_map_dev, h->t_key_map + l0, L * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (a->pinyin_dev && P) HIPCHK(hipMemcpyAsync(a->pinyin_dev, h->t_pinyin + p0, P * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
    if (a->pinyin_map_dev && P) HIPCHK(hipMemcpyAsync(a->pinyin_map_dev, h->t_pinyin_map + p0, P * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
    return DTTS_OK;
}

} // namespace dtts
