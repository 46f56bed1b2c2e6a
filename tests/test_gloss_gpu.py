"""The gloss encoder on the GPU (dict_tts_amd/gloss_encoder.py, csrc/gloss.hip) against the float64 restatement tests/gloss_ref.py, which
tests/test_gloss_cpu.py anchors on Hugging Face's RoFormerForMaskedLM.  Seeded weights (gloss_shapes.seeded_state), never a checkpoint.

Error gate: max |gpu - float64| over a call <= 8 x max |float32 restatement - float64| on the same inputs, both measured here.  Both sides
form the same exact fp32 products and differ in summation order and in exp / erf / rsqrt, which moves the rounding error by a single-digit
factor: 8 is the project's margin for that situation (tests/test_disc_gpu.py, tests/test_spkenc_gpu.py).  The ratios are printed.

Measured on an MI355X (LABNOTES.md "Gloss encoder"): mixed lengths 0.37 x (h128x7), 1.06 x (h768x1), 0.62 x (h384x2); a single token
0.71 / 1.52 / 1.18 x; the golden 0.74 x of the float32 restatement's error (gate 9 x); table path - tensor path pron_attn 6.0e-8, dict_attn
1.8e-6."""
import numpy as np
import pytest
import torch

import gloss_ref as R
import gloss_shapes as S
from dict_tts_amd import abi, synth
from dict_tts_amd import gloss_encoder as G
from dict_tts_amd import model as M

pytestmark = pytest.mark.gpu
MARGIN = 8.0
_CACHE = {}


def setup(name):
    """per configuration, once: the weights, the encoder, the mixed-length id set, its float64 / float32 restatements and the GPU's result"""
    if name not in _CACHE:
        cfg, n_hidden = (S.GOLDEN_CFG, 8) if name == "golden" else S.CFGS[name]
        st = S.seeded_state(cfg)
        enc = G.GlossEncoder.from_pretrained(st, cfg, n_hidden=n_hidden)
        ids = S.id_sets(S.MIXED_LENGTHS)
        c = {"cfg": cfg, "n_hidden": n_hidden, "state": st, "enc": enc, "ids": ids}
        if name != "golden":
            c["f64"] = R.encode_np(st, cfg, ids, torch.float64, n_hidden)
            c["f32"] = R.encode_np(st, cfg, ids, torch.float32, n_hidden)
            c["gpu"] = enc.encode(ids)
        _CACHE[name] = c
    return _CACHE[name]


@pytest.fixture(autouse=True, scope="module")
def _module():
    yield
    _CACHE.clear()


def cat(outs):
    return torch.cat(outs).double().cpu().numpy()


@pytest.mark.parametrize("name", list(S.CFGS))
def test_accuracy_mixed_lengths(name):
    c = setup(name)
    assert sum(S.MIXED_LENGTHS) % 32 and sum(S.MIXED_LENGTHS) % 128
    got = cat(c["gpu"])
    assert [tuple(o.shape) for o in c["gpu"]] == [(L, c["cfg"]["hidden_size"]) for L in S.MIXED_LENGTHS] and np.isfinite(got).all()
    e_gpu, e_f32 = np.abs(got - c["f64"]).max(), np.abs(c["f32"] - c["f64"]).max()
    print(f"GLOSSMEAS {name}: gpu - f64 {e_gpu:.3g}, f32 - f64 {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}, scale {np.abs(c['f64']).max():.3g}")
    assert e_gpu <= MARGIN * e_f32


@pytest.mark.parametrize("name", list(S.CFGS))
def test_accuracy_single_token(name):
    c = setup(name)
    ids = S.id_sets((1,), seed=S.SEED + 1)
    got = cat(c["enc"].encode(ids))
    f64 = R.encode_np(c["state"], c["cfg"], ids, torch.float64, c["n_hidden"])
    f32 = R.encode_np(c["state"], c["cfg"], ids, torch.float32, c["n_hidden"])
    e_gpu, e_f32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
    print(f"GLOSSMEAS {name} L = 1: gpu - f64 {e_gpu:.3g}, f32 - f64 {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}")
    assert got.shape == (1, c["cfg"]["hidden_size"]) and e_gpu <= MARGIN * e_f32


def test_golden():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_gloss.npz"))
    c = setup("golden")
    ids = [g["ids"][a:b] for a, b in zip(g["tok_off"][:-1], g["tok_off"][1:])]
    got = cat(c["enc"].encode(ids))
    e_f32 = np.abs(R.encode_np(c["state"], c["cfg"], ids, torch.float32, 8) - g["feat"]).max()
    e_gpu = np.abs(got - g["feat"]).max()
    print(f"GLOSSMEAS golden: gpu - golden {e_gpu:.3g}, f32 - golden {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}")
    assert e_gpu <= (MARGIN + 1) * e_f32


def test_batch_independence():
    """a gloss alone, first, last and in the middle of a 40-gloss call, and the whole call under two row budgets: the same bits"""
    c = setup("h128x7")
    enc = c["enc"]
    lengths = [1 + (7 * i) % 64 for i in range(39)]
    others = S.id_sets(lengths, seed=S.SEED + 2)
    fails = []
    for L in (1, 33, 64):
        me = S.id_sets((L,), seed=S.SEED + 3)[0]
        alone = enc.encode([me])[0]
        for place in (0, 20, 39):
            seqs = others[:place] + [me] + others[place:]
            got = enc.encode(seqs)[place]
            if not torch.equal(got, alone):
                fails.append(f"L = {L} at place {place} of 40: differs from the gloss alone by {float((got - alone).abs().max()):.3g}")
    small = G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=c["n_hidden"], row_budget=64)
    a, b = enc.encode(others), small.encode(others)
    fails += [f"gloss {i} (L = {lengths[i]}): row budgets 16384 and 64 differ" for i in range(len(others)) if not torch.equal(a[i], b[i])]
    assert not fails, "\n".join(fails)


def test_refusals_and_status():
    c = setup("h128x7")
    enc = c["enc"]
    ctx, dev = enc.ctx, enc.device
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.zeros(128, dtype=torch.int64, device=dev)
    out = torch.empty(128, 128, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(off, sum_L, L_max):
        t = torch.tensor(off, dtype=torch.int32, device=dev)
        ctx.gloss_encode(len(off) - 1, stream, ids=ids.data_ptr(), tok_off=t.data_ptr(), sum_L=sum_L, L_max=L_max, out=out.data_ptr(), status=status.data_ptr())

    for off, sum_L, L_max, word in (([0, 3, 68], 68, 64, "gloss 1 has L = 65"), ([0, 0, 5], 5, 5, "gloss 0 has L = 0"), ([0, 3, 8], 8, 6, "L_max = 6"),
                                    ([1, 3, 8], 8, 5, "tok_off[0] = 1"), ([0, 3, 7], 8, 5, "tok_off[n_gloss] = 7")):
        with pytest.raises(abi.DttsError, match=r"\(-22\).*" + word.replace("[", r"\[").replace("]", r"\]")):
            call(off, sum_L, L_max)
    call([0, 3, 8], 8, 5)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0]
    # an id equal to the vocabulary's size: a zero embedding row, the status names row and id, Python raises with the gloss and the position
    seqs = [np.array([1, 2, 3]), np.array([4, S.VOCAB, 5, S.VOCAB + 1])]
    with pytest.raises(abi.DttsError, match=rf"gloss 1, position 1: token id {S.VOCAB} .*row 4"):
        enc.encode(seqs)
    with pytest.raises(abi.DttsError, match="no weights"):
        G.GlossEncoder().encode([[1, 2]])
    fresh = abi.Context()
    with pytest.raises(abi.DttsError, match=r"\(-1\).*before dtts_finalize_weights\(DTTS_PART_GLOSS\)"):
        fresh.gloss_encode(1, stream, ids=ids.data_ptr(), tok_off=ids.data_ptr(), sum_L=3, L_max=3, out=out.data_ptr(), status=status.data_ptr())
    # finalize names what it refuses
    w = dict(enc._state())
    for change, word in (({"config": np.array([4, 1e-12, 0, 0], np.float32)}, "heads of 64"), ({"config": np.array([2, 1e-12, 1, 0], np.float32)}, "rotary_value"),
                         ({"config": np.array([2, 1e-12, 0, 1], np.float32)}, "hidden_act"),
                         ({"embeddings.word_embeddings.weight": np.zeros((S.VOCAB, 64), np.float32)}, "embedding_size = 64")):
        bad = abi.Context()
        bad.load_state_dict("gloss", {**w, **change})
        with pytest.raises(abi.DttsError, match=r"\(-22\).*" + word):
            bad.finalize(abi.PART_GLOSS)
    bad = abi.Context()
    bad.load_state_dict("gloss", {k: v for k, v in w.items() if k != "encoder.layer.2.intermediate.dense.bias"})
    with pytest.raises(abi.DttsError, match=r"\(-22\).*missing tensor gloss.encoder.layer.2.intermediate.dense.bias"):
        bad.finalize(abi.PART_GLOSS)


def test_red_zones_stay_whole():
    """debug_redzone = 1: every workspace buffer between red zones and 0xFF before each call; no launch damages a zone, no stale word is
    consumed (the result would be NaN), and the bits are those of the plain context"""
    c = setup("h128x7")
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    enc = G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=c["n_hidden"], ctx=ctx, row_budget=128)
    got = enc.encode(c["ids"])
    damaged = ctx.debug_check(torch.cuda.current_stream().cuda_stream)
    assert damaged == 0, ctx.last_error()
    assert all(torch.equal(a, b) for a, b in zip(got, c["gpu"]))


def test_end_to_end_through_the_dictionary_table():
    """build_table -> dtts_dict_table_upload -> dtts_text2mel_encode_ids on a three-word sentence: pron_attn and dict_attn equal those of
    the tensor path (dtts_text2mel_encode) fed the same embeddings, within the per-row maxima tests/test_s2pa_gpu.py holds both paths to
    (acoustic_ref.BOUNDS)"""
    import acoustic_ref as ar
    c = setup("h768x1")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    g = S.id_sets((5, 3, 5, 32, 7), seed=S.SEED + 4)
    n_words = 8
    entries = {3: [(("zh", "ong1"), g[0])], 4: [(("h", "ang2"), g[1]), (("x", "ing2"), g[2]), (("h", "ang4"), g[3])], 6: [(("d", "e5"), g[4])]}
    table = c["enc"].build_table(entries, n_words)
    assert table["keys"].shape == (3 * 5 + 5 + 40 + 7, 768) and np.isfinite(table["keys"]).all() and np.abs(table["keys"][table["tok_off"][3]:table["tok_off"][4]]).max() > 0.1
    m = M.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(1234).items()})
    m.upload_dict_table(table)
    sent = [[3, 4, 5]]   # one gloss, three glosses, a word the dictionary lacks
    ib = synth.make_id_batch(sent, table, pron_every=0)
    assert (ib["L_k"], ib["P"]) == (40, 6)
    Tw = 5
    keys = np.zeros((1, Tw, 40, 768), np.float32)
    key_map, pinyin, pinyin_map = np.zeros((1, Tw, 40), np.float32), np.zeros((1, Tw, 6), np.int64), np.zeros((1, Tw, 6), np.int64)
    for t, w in enumerate(sent[0]):
        a, b, p, q = table["tok_off"][w], table["tok_off"][w + 1], table["pin_off"][w], table["pin_off"][w + 1]
        keys[0, t + 1, :b - a], key_map[0, t + 1, :b - a] = table["keys"][a:b], table["key_map"][a:b]
        pinyin[0, t + 1, :q - p], pinyin_map[0, t + 1, :q - p] = table["pinyin"][p:q], table["pinyin_map"][p:q]
    key_map[:, [0, -1]] = 1
    pinyin_map[:, [0, -1]] = 1
    m2w = T(synth.teacher_mel2word(ib["word_tokens"], 8, 4))
    assert m2w.shape[1] == 32
    z = T(synth.noise(1234, 1, 8, "gloss.z"))
    by_id = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], mel2word=m2w, z_p=z)
    by_tensor = m((T(ib["word_tokens"]), None), T(ib["pron_modified"]), (None, None, None), None, None,
                  (T(keys), T(keys.copy()), T(key_map), T(pinyin), T(pinyin_map)), infer=True, z_p=z, mel2word=m2w)
    for k in ("pron_attn", "dict_attn"):
        d = float((by_id[k].double() - by_tensor[k].double()).abs().max())
        print(f"GLOSSMEAS end to end: {k} table - tensor {d:.3g}")
        assert by_id[k].shape == by_tensor[k].shape and d <= ar.BOUNDS[k]["max"], k
    # the words attend to their glosses: weights on the live rows of the three-gloss word sum to 1, the missing word's single live row takes all
    da = by_id["dict_attn"][0, 0].cpu().numpy()   # [L_k, T_w]
    assert abs(da[:40, 2].sum() - 1) < 1e-5 and abs(da[1, 3] - 1) < 1e-5
