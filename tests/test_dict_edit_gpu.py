"""Editing the resident dictionary in place (PortaSpeech_dict.edit_dict_table, csrc/dict_edit.hip) on the GPU.

The yardstick of every case is a FRESH context that uploads the edited dictionary with ``upload_dict_table`` (the path the parity tests pin
to the reference); equality is exact — bit patterns, so that a NaN or a signed zero cannot hide — in
  (i)  ``dict_entry(e)`` of every entry (K, V, key_map, pinyin, pinyin_map, L, P) and ``dict_entries()``,
  (ii) ``forward_ids`` (dur, pron_attn, dict_attn, word_encoder_out, mel_out) on a batch that uses EVERY entry of the edited table, with a
       teacher-forced mel2word and a fixed z_p.
Every case builds its own models on the 24-entry dictionary of tests/dict_edit_shapes.py (hidden 192, gloss_dim 768): an edit changes the
context it is applied to."""
import numpy as np
import pytest
import torch

import dict_edit_shapes as S
from dict_tts_amd import abi, dict_embed, synth
from dict_tts_amd import model as M

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
OUT_KEYS = ("dur", "pron_attn", "dict_attn", "word_encoder_out", "mel_out")
ENTRY_KEYS = ("K", "V", "key_map", "pinyin", "pinyin_map")
_STATE = {}


def make_model(**hp):
    if not _STATE:
        _STATE.update({k: T(v) for k, v in synth.dict_tts_state_dict(S.SEED).items()})
    m = M.PortaSpeech_dict(hparams=hp)
    m.load_state_dict(_STATE)
    return m


def uploaded(items, **hp):
    m = make_model(**hp)
    m.upload_dict_table(S.table_of(items))
    return m


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def snapshot(m):
    return [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in m.dict_entry(e).items()} for e in range(m.dict_entries())]


def assert_entries(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for e, (a, b) in enumerate(zip(got, want)):
        assert (a["L"], a["P"]) == (b["L"], b["P"]), (what, e, a["L"], a["P"], b["L"], b["P"])
        for k in ENTRY_KEYS:
            assert same(a[k], b[k]), (what, "entry", e, k)


def run(m, items):
    """forward_ids on the three sentences that use every entry of ``items``"""
    ib = synth.make_id_batch(S.sentences(len(items)), S.table_of(items), pron_every=3)
    m2w = T(synth.teacher_mel2word(ib["word_tokens"], 4, 2))
    z = T(synth.noise(S.SEED, m2w.shape[0], m2w.shape[1] // 4, "edit.z"))
    r = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], mel2word=m2w, z_p=z)
    return {k: r[k] for k in OUT_KEYS}


def assert_outputs(got, want, what):
    for k in OUT_KEYS:
        assert same(got[k], want[k]), (what, k, float((got[k].double() - want[k].double()).abs().max()))


def on_device(items):
    dev = lambda a: None if a is None else T(a).cuda()
    return [{**it, "key": dev(it["key"]), **({"value": dev(it["value"])} if "value" in it else {})} for it in items]


def edit(m, rep, app, device=False):
    if device:
        rep, app = dict(zip(rep, on_device(list(rep.values())))), on_device(app)
    return m.edit_dict_table(replace=rep, append=app)


def check(m, items, what):
    """(i) and (ii) against a fresh context that uploads ``items``"""
    fresh = uploaded(items)
    assert m.dict_entries() == fresh.dict_entries() == len(items)
    assert_entries(snapshot(m), snapshot(fresh), what)
    assert_outputs(run(m, items), run(fresh, items), what)


@pytest.mark.parametrize("name", list(S.edits()))
def test_an_edit_equals_a_fresh_upload(name):
    rep, app = S.edits()[name]
    base = S.base_items()
    m = uploaded(base)
    new_ids = edit(m, rep, app)
    assert new_ids == list(range(S.N_BASE, S.N_BASE + len(app)))
    check(m, S.apply(base, rep, app), name)


def test_host_rows_and_device_rows_with_and_without_values_agree():
    """one edit four ways: host / device rows x values left out / given as arrays of their own that equal the keys -> four identical tables,
    all the fresh upload's; then values that DIFFER from the keys, from host and from device rows"""
    base = S.base_items()
    rep, app = S.mixed()
    with_values = lambda its: [{**it, "value": it["key"].copy()} for it in its]
    rep_v, app_v = dict(zip(rep, with_values(list(rep.values())))), with_values(app)
    want = uploaded(S.apply(base, rep, app))
    w_entries, w_out = snapshot(want), run(want, S.apply(base, rep, app))
    for device in (False, True):
        for r, a, tag in ((rep, app, "values=None"), (rep_v, app_v, "values given")):
            m = uploaded(base)
            edit(m, r, a, device)
            assert_entries(snapshot(m), w_entries, (device, tag))
            assert_outputs(run(m, S.apply(base, rep, app)), w_out, (device, tag))
    rep, app = S.mixed(own_value=True)
    new = S.apply(base, rep, app)
    assert S.table_of(new)["values"] is not None
    want = uploaded(new)
    w_entries, w_out = snapshot(want), run(want, new)
    assert not same(w_entries[S.FIRST]["K"], w_entries[S.FIRST]["V"])
    for device in (False, True):
        m = uploaded(base)
        edit(m, rep, app, device)
        assert_entries(snapshot(m), w_entries, (device, "own values"))
        assert_outputs(run(m, new), w_out, (device, "own values"))


def test_two_edits_in_a_row():
    """the second edit replaces an entry the first one appended (and appends again): one fresh upload of the final dictionary"""
    base = S.base_items()
    m = uploaded(base)
    rep1, app1 = {3: S.item("two.a", 21, senses=2)}, [S.item("two.b", 8), S.item("two.c", 2)]
    assert edit(m, rep1, app1) == [S.N_BASE, S.N_BASE + 1]
    mid = S.apply(base, rep1, app1)
    rep2, app2 = {3: S.item("two.d", 1), S.N_BASE: S.item("two.e", 30, senses=3)}, [S.item("two.f", 5)]
    assert edit(m, rep2, app2, device=True) == [S.N_BASE + 2]
    check(m, S.apply(mid, rep2, app2), "two edits")


def test_the_tensor_path_anchors_the_edited_table():
    """outside the id path: the edited dictionary's collated tensors through forward(dict_msg=...) against forward_ids after the edit, to
    the tolerances tests/test_gpu_parity.py keeps between those two paths (test_resident_dictionary_ids_equal_collated_tensors)"""
    base = S.base_items()
    rep, app = S.mixed(own_value=True)
    m = uploaded(base)
    edit(m, rep, app, device=True)
    new = S.apply(base, rep, app)
    ib, tb = S.collate(S.table_of(new), S.sentences(len(new)))
    m2w = T(synth.teacher_mel2word(ib["word_tokens"], 4, 2))
    z = T(synth.noise(S.SEED, m2w.shape[0], m2w.shape[1] // 4, "edit.z"))
    by_id = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], mel2word=m2w, z_p=z)
    by_tensor = m((T(ib["word_tokens"]), None), T(ib["pron_modified"]), (None,) * 3, None, None,
                  (T(tb["keys"]), T(tb["values"]), T(tb["key_map"]), T(tb["pinyin"]), T(tb["pinyin_map"])), infer=True, z_p=z, mel2word=m2w)
    assert torch.equal(by_id["mel2word"], by_tensor["mel2word"])
    for k, tol in (("dur", 1e-5), ("pron_attn", 1e-5), ("dict_attn", 1e-5), ("word_encoder_out", 1e-4), ("mel_out", 1e-3)):
        d = float((by_id[k] - by_tensor[k]).abs().max())
        print(f"DICTEDIT anchor: {k} table - tensor {d:.3g}")
        assert by_id[k].shape == by_tensor[k].shape and torch.isfinite(by_id[k]).all() and d <= tol, (k, d)


def test_order_on_a_stream():
    """encode, edit, encode with no synchronisation by the caller: what the first encode's fetches were handed is what the OLD table gives,
    the second encode sees the NEW table"""
    base = S.base_items()
    rep, app = S.mixed()
    new = S.apply(base, rep, app)
    m = uploaded(base)
    first = run(m, base)
    edit(m, rep, app, device=True)
    second = run(m, new)
    assert_outputs(first, run(uploaded(base), base), "before the edit")
    assert_outputs(second, run(uploaded(new), new), "after the edit")
    assert not same(first["pron_attn"], second["pron_attn"])


def test_a_refused_edit_leaves_the_table_intact():
    base = S.base_items()
    m = uploaded(base)
    before, out = snapshot(m), run(m, base)
    stream = torch.cuda.current_stream().cuda_stream
    bad = S.item("bad.sense", 6)
    bad["pinyin_map"] = np.array([1, 16], np.int64)
    with pytest.raises(abi.DttsError, match=r"\(-22\).*entry 3 has sense index 16; at most 15"):
        m.edit_dict_table(replace={2: S.item("bad.ok", 4), 3: bad})
    p = dict_embed.pack_items([S.item("bad.a", 4), S.item("bad.b", 5)])
    call = lambda ids: m.ctx.dict_table_edit(ids, p["tok_off"], p["pin_off"], p["key_map"], p["pinyin"], p["pinyin_map"], np.concatenate(p["keys"]),
                                             None, stream)
    with pytest.raises(abi.DttsError, match=r"\(-22\).*strictly ascending \(entry_id\[1\] = 1 after 3\)"):
        call([3, 1])
    with pytest.raises(abi.DttsError, match=rf"\(-22\).*entry_id\[1\] = {S.N_BASE + 1} leaves a gap: the table holds {S.N_BASE} entries"):
        call([3, S.N_BASE + 1])
    assert m.dict_entries() == S.N_BASE
    assert_entries(snapshot(m), before, "after three refusals")
    assert_outputs(run(m, base), out, "after three refusals")
    with pytest.raises(abi.DttsError, match=rf"\(-22\).*entry = {S.N_BASE}, the table holds {S.N_BASE} entries"):
        m.dict_entry(S.N_BASE)
    # the refusals that need the context: weights not finalised, no table resident
    raw = M.PortaSpeech_dict(hparams={})
    call = lambda c: c.dict_table_edit([0, 1], p["tok_off"], p["pin_off"], p["key_map"], p["pinyin"], p["pinyin_map"], np.concatenate(p["keys"]), None, stream)
    with pytest.raises(abi.DttsError, match=r"\(-1\).*DTTS_DICT_EDIT\) before dtts_finalize_weights\(DTTS_PART_ACOUSTIC\)"):
        call(raw.ctx)
    empty = make_model()
    assert empty.dict_entries() == 0
    with pytest.raises(abi.DttsError, match=r"\(-1\).*no table is resident"):
        call(empty.ctx)
    with pytest.raises(abi.DttsError, match=r"\(-1\).*no table is resident"):
        empty.dict_entry(0)


def test_memory_safety_mode():
    """debug_redzone = 1: the new arrays of an edit sit between red zones like the upload's; a mixed replace-and-append edit and the encode
    behind it damage none, and give the release context's bits"""
    base = S.base_items()
    rep, app = S.mixed(own_value=True)
    new = S.apply(base, rep, app)
    for device in (False, True):
        m = uploaded(base, dtts_debug_redzone=1)
        edit(m, rep, app, device)
        got = run(m, new)
        assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()
        assert all(torch.isfinite(v).all() for v in got.values())
        check(m, new, f"red zones, device rows = {device}")
        assert m.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, m.ctx.last_error()


def test_gloss_ids_to_the_resident_table_without_the_host():
    """seeded gloss encoder -> build_items(device=True) -> edit_dict_table(append=...): the table of a fresh upload of
    build_items(device=False)'s items"""
    import gloss_shapes as GS
    from dict_tts_amd import gloss_encoder as G
    cfg, n_hidden = GS.CFGS["h768x1"]
    enc = G.GlossEncoder.from_pretrained(GS.seeded_state(cfg), cfg, n_hidden=n_hidden)
    g = GS.id_sets((5, 3, 5, 32, 7, 4), seed=GS.SEED + 4)
    entries = {0: [(("zh", "ong1"), g[0])], 1: [(("h", "ang2"), g[1]), (("x", "ing2"), g[2]), (("h", "ang4"), g[3])], 3: [(("d", "e5"), g[4])],
               5: [(("l", "e5"), g[5])]}
    host, dev = enc.build_items(entries, 6), enc.build_items(entries, 6, device=True)
    assert all(it["key"].is_cuda and it["value"].is_cuda for it in dev) and not any(it["key"].is_cuda for it in host)
    penc = ["<UNK>"] + sorted({p for it in host for p in it["pinyin"]} - {"<UNK>"})
    m = make_model()
    m.upload_dict_table(dict_embed.table_from_items(host[:3], penc))
    assert m.edit_dict_table(append=dev[3:], pinyin_encoder=penc) == [3, 4, 5]
    fresh = make_model()
    fresh.upload_dict_table(dict_embed.table_from_items(host, penc))
    got = snapshot(m)
    assert_entries(got, snapshot(fresh), "gloss path")
    assert [e["L"] for e in got] == [5, 40, 3, 7, 3, 4] and float(got[3]["K"].abs().max()) > 0
