"""S2PA (ops.hip: s2pa_kernel, four instantiations) word by word against the float64 restatement, along its own axes: gloss rows per entry,
live rows and their pattern, row order, senses and pinyin slots, forced pronunciations, dead words, row width -- the case table of
tests/s2pa_shapes.py, each case named after the branch it forces (run with `-m gpu` on an MI355X; tests/test_s2pa_cpu.py shows on the
CPU that every planted partition defect is caught by one of these cases at these bounds).

Every case runs in the forms it has: the resident table + ids (the benchmark's input: the speculative stream s2pa_kernel<1, 3|4, true>;
<3, 4, false> with `entry` set at hidden 384), the collated tensors with `values` a separate tensor, and with `values` THE SAME tensor
as `keys` (the alias branch `r.kb == r.vb`: two chunks in flight).  The .vfull cases carry separate full-scale `values` (uploaded with
the table too) and have no alias form.  A short teacher-forced mel2word (2 frames per word) keeps the float64 reference small.
dict_attn, pron_attn, context and word_encoder_out are compared with acoustic_ref.BOUNDS, unchanged, on every case; one ``S2PAMEAS {json}``
line per comparison (run with -s).

Before this file no test and no caller passed one tensor for keys and values: synth.make_batch returns values = keys.copy(), and every
test, smoke() and bench.py hand the two arrays over separately, so the alias branch of the shipped kernel had never run.

Also: each word bit-identical to itself alone (B = 1) in both forms, whatever the batch's L_k; alias == separate-but-equal bit for bit
(the claim of the comment beside `alias`); the refusals, each naming the value (L_k = S2PA_LMAX + 1, P = 65, sense 16 in pinyin_map, an
entry longer than L_k / P through forward_ids, the last three at the predicted-duration call's one host synchronisation); one case per
instantiation under debug_redzone.  Not reachable, so not run: s2pa_kernel<1, S2PA_RU_P, false> (collated rows <= 256 wide) needs
gloss_dim <= 256, and no hparam sets gloss_dim (the model and the synthetic weights are 768 wide).

Measured on MI355X, worst over every case and form of this file (GPU - float64, max / 8-word window RMS / RMS; the bounds are
acoustic_ref.BOUNDS).  The .peaked family (the synthetic gloss scale, batches dense in long all-live entries) apart, since torch's fp32
oracle itself uses up to 0.76 / 1.0 of the context / word_encoder_out bounds there (tests/test_s2pa_cpu.py):
  every other case   dict_attn 1.6e-7 / 1.4e-8 / 1.3e-8   pron_attn 2.4e-7 / 1.8e-7 / 1.8e-7   context 8.6e-7 / 1.5e-7 / 1.3e-7
                     word_encoder_out 3.6e-6 / 5.1e-7 / 5.1e-7   (largest share of a bound: pron_attn RMS 0.41, order_descending)
  .peaked            dict_attn 2.6e-6 / 1.5e-7 / 1.4e-7   pron_attn 1.7e-6 / 3.8e-7 / 3.2e-7   context 1.1e-5 / 1.3e-6 / 1.3e-6
                     word_encoder_out 7.3e-6 / 1.4e-6 / 1.3e-6   (largest share: pron_attn RMS 0.73, patterns_66.peaked, table form)
No case exceeds a bound and no bound is widened.  The alias form is bit-identical to the separate-but-equal form on every case (the
kernel's comment is right), and every word is bit-identical to itself alone.  No kernel defect was found.
"""
import json

import numpy as np
import pytest
import torch

import acoustic_ref as ar
import s2pa_shapes as sp
import test_text2mel_kernels_gpu as tk
from dict_tts_amd import abi, synth

pytestmark = pytest.mark.gpu
T = tk.T
OUT = ("dict_attn", "pron_attn", "context", "word_encoder_out")
_M, _CASES = {}, {}


@pytest.fixture(autouse=True, scope="module")
def _module():
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(n)
    _M.clear()
    _CASES.clear()


def model(hp_name, **extra):
    key = (hp_name, tuple(sorted(extra.items())))
    if key not in _M:
        _M[key] = tk.make_model(tk.shape_hp(hp_name), **extra)
    return _M[key]


def cases():
    if not _CASES:
        _CASES.update(sp.cases())
        base = sp.order_base()
        pre = sp.s2pa_inputs(ar.state(tk.sd_np({}), torch.float64), {}, base.batch())
        _CASES.update(sp.order_cases({i: pre["logits"][0, i + 1, :len(e[1])].numpy() for i, e in enumerate(base.entries)}))
    return _CASES


CASE_NAMES = sorted(sp.cases()) + list(sp.ORDER_NAMES)   # (names only: a case builds its entries on first use)


def forward(m, batch, m2w, z, alias=False):
    """the tensor API; alias: ONE device tensor for keys and values (model.forward keeps a float32 contiguous device tensor as it is)"""
    b = {k: T(v) for k, v in batch.items()}
    keys = b["keys"].cuda()
    values = keys if alias else b["values"].cuda()
    assert (keys.data_ptr() == values.data_ptr()) == alias
    r = m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
          (keys, values, b["key_map"], b["pinyin"], b["pinyin_map"]), infer=True, z_p=z, mel2word=None if m2w is None else T(m2w))
    return tk.with_context(m, r, *batch["word_tokens"].shape)


def forward_ids(m, ib, m2w, z, L_k=None, P=None):
    r = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"] if L_k is None else L_k,
                      ib["P"] if P is None else P, z_p=z, mel2word=None if m2w is None else T(m2w))
    return tk.with_context(m, r, *ib["word_tokens"].shape)


def measure(case, form, got, want, batch, fails):
    word_mask = torch.from_numpy(batch["word_tokens"] > 0).double()
    for k in OUT:
        v = ar.rowcmp(tk.as_rows(k, got[k], word_mask), tk.as_rows(k, want[k], word_mask))
        print("S2PAMEAS " + json.dumps({"case": case, "form": form, "what": k, **v}), flush=True)
        b = ar.BOUNDS[k]
        fails += [f"{case} [{form}]: {k} {s} {v[s]:.3g} > {b[s]:.3g} (max at word {v['at']}, worst window at {v['win_at']})"
                  for s in ("max", "win", "rms") if v[s] > b[s]]


def teacher(c, batch, hp):
    frames = c.frames()
    m2w = ar.spread_mel2word(batch["word_tokens"], frames)
    T4 = -(-max(frames) // 4)
    return m2w, tk.noise(f"s2pa.{c.name}.z", batch["word_tokens"].shape[0], T4, synth.acoustic_shape(hp)["latent_size"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_s2pa_case_against_float64(name):
    c = cases()[name]
    hp = tk.shape_hp(c.hp)
    m = model(c.hp)
    batch = c.batch()
    m2w, z = teacher(c, batch, hp)
    want = tk.reference(hp, sp.for_reference(batch), m2w, z)
    fails = []
    tab = sp.table(c.entries)
    m.upload_dict_table(tab)
    got = {"table": forward_ids(m, c.ids(tab), m2w, z), "tensor": forward(m, batch, m2w, z)}
    if "values" not in tab:
        got["alias"] = forward(m, batch, m2w, z, alias=True)
    for form, g in got.items():
        assert torch.equal(g["mel2word"].cpu(), want["mel2word"])
        measure(name, form, g, want, batch, fails)
    if "alias" in got:   # the comment beside `alias` in s2pa_kernel: both input forms give bit-identical results
        for k in OUT + ("mel_out",):
            if not torch.equal(got["alias"][k], got["tensor"][k]):
                fails.append(f"{name}: {k} of the alias form differs from the separate-but-equal form in bits "
                             f"(max {float((got['alias'][k] - got['tensor'][k]).abs().max()):.3g})")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------- each word against itself
ALONE = ("rows_148-257_mixed_with_1.flat", "rows_1-17.peaked", "patterns_66.flat")


@pytest.mark.parametrize("name", ALONE)
def test_each_word_equals_itself_alone(name):
    """a batch of single-word sentences (one per entry, L_k / P the batch maxima) against each sentence alone at B = 1 (L_k / P its own):
    dict_attn over the word's own rows, pron_attn over its own slots and context are bit-identical, the padding rows' weights are what the
    word alone says they are (exactly 0 where it has a live row), in the table form and the tensor form"""
    c0 = cases()[name]
    m = model("default")
    ent = c0.entries
    tab = sp.table(ent)
    m.upload_dict_table(tab)
    sents = [[3 + i] for i in range(len(ent))]
    big = sp.Case(name + ".batch", ent, sents)
    fails = []
    bb = big.batch()
    m2w_b, z_b = ar.spread_mel2word(bb["word_tokens"], [8] * len(sents)), tk.noise("alone.z", len(sents), 2)
    both = {"table": forward_ids(m, big.ids(tab), m2w_b, z_b), "tensor": forward(m, bb, m2w_b, z_b)}
    for i in range(len(ent)):
        one = sp.Case(f"{name}.alone{i}", ent, [sents[i]])
        b1 = one.batch()
        m2w, z = ar.spread_mel2word(b1["word_tokens"], [8]), z_b[i:i + 1]
        alone = {"table": forward_ids(m, one.ids(tab), m2w, z), "tensor": forward(m, b1, m2w, z)}
        L, P = len(ent[i][1]), len(ent[i][2])
        for form in ("table", "tensor"):
            a, g = alone[form], both[form]
            same = (torch.equal(a["dict_attn"][0, 0, :L, 1], g["dict_attn"][i, 0, :L, 1]) and
                    torch.equal(a["pron_attn"][0, 1, :P], g["pron_attn"][i, 1, :P]) and torch.equal(a["context"][0, 1], g["context"][i, 1]))
            pad = g["dict_attn"][i, 0, L:, 1]
            if not same:
                fails.append(f"{name} entry {i} ({L} rows) [{form}]: differs from the word alone, dict_attn max "
                             f"{float((a['dict_attn'][0, 0, :L, 1] - g['dict_attn'][i, 0, :L, 1]).abs().max()):.3g}, context max "
                             f"{float((a['context'][0, 1] - g['context'][i, 1]).abs().max()):.3g}")
            if ent[i][1].any() and pad.numel() and float(pad.abs().max()) != 0.0:
                fails.append(f"{name} entry {i} [{form}]: a padding row has weight {float(pad.abs().max()):.3g}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------- refusals
def small():
    c = sp.Case("refusals", sp.rows_entries((5, 9), sp.FLAT, "refuse") + sp.p_entries(7, sp.FLAT))
    return c, sp.table(c.entries)


def test_refusals_name_the_value():
    c, tab = small()
    m = model("default")
    m.upload_dict_table(tab)
    ib, batch = c.ids(tab), c.batch()
    with pytest.raises(abi.DttsError, match=f"L_k={sp.LMAX + 1}"):
        forward_ids(m, ib, None, None, L_k=sp.LMAX + 1)
    with pytest.raises(abi.DttsError, match="P=65"):
        forward_ids(m, ib, None, None, P=65)
    wide = dict(batch)
    wide["pinyin"] = np.zeros(batch["pinyin"].shape[:2] + (65,), np.int64)
    wide["pinyin_map"] = np.zeros(batch["pinyin"].shape[:2] + (65,), np.int64)
    with pytest.raises(abi.DttsError, match="P=65"):
        forward(m, wide, None, None)
    # sense 16 in pinyin_map, tensor API, predicted durations: refused at the call's one host synchronisation
    bad = dict(batch)
    bad["pinyin_map"] = batch["pinyin_map"].copy()
    bad["pinyin_map"][0, 2, 0] = sp.MAX_SENSES + 1
    with pytest.raises(abi.DttsError, match=f"sense index {sp.MAX_SENSES + 1}; at most {sp.MAX_SENSES} senses"):
        forward(m, bad, None, None)
    # forward_ids with L_k / P below an entry of the batch (the kernel would clamp and drop the rest silently): the longest entry has 60
    # gloss rows and 7 pinyin slots
    assert ib["L_k"] == 60 and ib["P"] == 7
    with pytest.raises(abi.DttsError, match="entry of 60 gloss rows and one of 7 pinyin slots; L_k=59 P=7"):
        forward_ids(m, ib, None, None, L_k=59)
    with pytest.raises(abi.DttsError, match="entry of 60 gloss rows and one of 7 pinyin slots; L_k=60 P=6"):
        forward_ids(m, ib, None, None, P=6)
    # the context still works, and larger L_k / P than the maxima are fine
    m2w, z = teacher(c, batch, {})
    want = tk.reference({}, batch, m2w, z)
    fails = []
    measure("refusals.after", "table", forward_ids(m, ib, m2w, z), want, batch, fails)
    g = forward_ids(m, ib, None, None, L_k=64, P=8)
    # (the dictionary words; the first and last padded rows are all ones over the whole of L_k and P: their uniform weights are 1 / L_k)
    assert torch.equal(g["pron_attn"][:, 1:-1, :7].cpu(), forward_ids(m, ib, None, None)["pron_attn"][:, 1:-1].cpu())
    assert not g["pron_attn"][:, 1:-1, 7:].any()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------- red zones
REDZONE = [("default", "rows_148-257_mixed_with_1.flat"),                                  # <1, 3, true> and <3, 4, false>
           ("h256_heads4-mha_dk64-s2pa_1x4-post_cond_f32", "width_h256.rows.flat"),       # <1, 4, true>
           ("h384_heads4-mfma_c384-s2pa_table_d384", "width_h384.rows.flat")]             # <3, 4, false> with `entry` set


@pytest.mark.parametrize("hp_name,name", REDZONE, ids=[h.split("_")[0] for h, _ in REDZONE])
def test_s2pa_memory_safety(hp_name, name):
    """debug_redzone: no zone damaged after the table, tensor and alias forward, every output bit-identical to the release context's"""
    c = cases()[name]
    hp = tk.shape_hp(hp_name)
    rel, dbg = model(hp_name), tk.make_model(hp, dtts_debug_redzone=1)
    tab = sp.table(c.entries)
    rel.upload_dict_table(tab)
    dbg.upload_dict_table(tab)
    batch = c.batch()
    m2w, z = teacher(c, batch, hp)
    s = torch.cuda.current_stream().cuda_stream
    for form in ("table", "tensor", "alias"):
        run = (lambda m: forward_ids(m, c.ids(tab), m2w, z)) if form == "table" else (lambda m: forward(m, batch, m2w, z, form == "alias"))
        a, b = run(rel), run(dbg)
        assert dbg.ctx.debug_check(s) == 0, f"{name} {form}: {dbg.ctx.last_error()}"
        for k in OUT + ("mel_out", "mel2word"):
            x, y = a[k].cpu(), b[k].cpu()
            assert torch.isfinite(y.float()).all() and torch.equal(x, y), (name, form, k)
