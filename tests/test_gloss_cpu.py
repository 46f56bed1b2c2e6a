"""The gloss encoder without a GPU: the float64 restatement tests/gloss_ref.py against the golden of Hugging Face's RoFormerForMaskedLM
(tests/golden/g18_gloss.npz, tools/make_golden_gloss.py) and, where ``transformers`` is importable, against the live model; the item
assembly of dict_tts_amd/gloss_encoder.py against hand-written items; the refusals that need no device; the argument block.

The gates of tests/test_gloss_gpu.py (gloss_ref.BOUNDS: max 8 x, global RMS 4 x, every row 6 x the float32 restatement's error) against
the planted defects gloss_ref.DEFECTS, each run in float32 and judged as the GPU's result is.  Every defect fails at least one gate at
every shape where it applies.  What the earlier max-only gate caught: all of them but eps_1e-6 at h128x7 (0.72 of that gate) and at
h384x2 (0.64), which the RMS gate (6.55, 7.46) and the row gate (21, 10.7) flag.  two_bf16_pieces (gloss_ref.SUBLIMINAL) is below the
float32 yardstick and is not claimed: its ratios are printed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import gloss_ref as R
import gloss_shapes as S
from dict_tts_amd import abi, dict_embed
from dict_tts_amd import gloss_encoder as G

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "g18_gloss.npz"))


def split(g):
    return [g["ids"][a:b] for a, b in zip(g["tok_off"][:-1], g["tok_off"][1:])]


def test_restatement_equals_the_golden(golden):
    ids = split(golden)
    assert [len(i) for i in ids] == list(S.GOLDEN_LENGTHS) and all(np.array_equal(a, b) for a, b in zip(ids, S.id_sets(S.GOLDEN_LENGTHS)))
    got = R.encode_np(S.seeded_state(S.GOLDEN_CFG), S.GOLDEN_CFG, ids)
    err = np.abs(got - golden["feat"]).max()
    print(f"restatement - golden: {err:.3g} at scale {np.abs(golden['feat']).max():.3g}")
    assert got.shape == golden["feat"].shape and err <= 1e-9
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g18_gloss.npz")) < 200 * 1024


def test_restatement_against_live_transformers():
    pytest.importorskip("transformers")
    cfg, n_hidden = S.CFGS["h384x2"]
    st = S.seeded_state(cfg)
    model = S.hf_model(cfg, st, torch.float64)
    ids = S.id_sets((1, 2, 7, 33))
    want = np.concatenate([S.hf_feat(model, i, n_hidden).numpy() for i in ids])
    assert np.abs(R.encode_np(st, cfg, ids, n_hidden=n_hidden) - want).max() <= 1e-9


def test_the_rotation_and_the_unused_tensors_matter_as_stated():
    cfg, n_hidden = S.CFGS["h128x7"]
    st = S.seeded_state(cfg)
    ids = S.id_sets((5, 9))
    base = R.encode_np(st, cfg, ids, n_hidden=3)
    # with or without the prefix, with a (ruined) position table and an MLM head: the same features
    noisy = {"roformer." + k: v for k, v in st.items()}
    noisy["roformer.encoder.embed_positions.weight"] = np.full((128, 64), 7.0, np.float32)
    noisy["cls.predictions.bias"] = np.ones(cfg["vocab_size"], np.float32)
    assert np.array_equal(R.encode_np(noisy, cfg, ids, n_hidden=3), base)
    # a permutation of a gloss's inner tokens permutes no row: the rotary position enters the scores
    perm = [ids[0][[0, 2, 1, 3, 4]], ids[1]]
    moved = R.encode_np(st, cfg, perm, n_hidden=3)
    assert np.abs(moved[[0, 2, 1, 3, 4]] - base[:5]).max() > 1e-4 and np.array_equal(moved[5:], base[5:])
    sin, cos = R.rotary_table(64)
    assert sin.dtype == np.float32 and sin.shape == (64, 32) and sin[0].max() == 0 and cos[0].min() == 1
    assert sin[3, 0] == np.float32(np.sin(3.0)) and cos[5, 31] == np.float32(np.cos(5 / 10000 ** (62 / 64)))


# ---- the three gates (gloss_ref.BOUNDS) against planted defects: every defect runs in float32 on the mixed-length ids and is judged as
# the GPU's result is, with the clean float32 run as the yardstick
_CLEAN = {}
# where a defect applies: the partial head group exists where heads % 4 != 0 (2, 6 and 3 heads); everything else at the three accuracy shapes
DEFECT_SHAPES = {d: (("h128x7", "h384x2", "h192_nh3_pad") if d == "last_head_of_group_dropped" else tuple(S.CFGS)) for d in R.DEFECTS}
# what the max-only gate (max |g - d| <= 8 x max |s - d|) let through: eps_1e-6 reads 0.72 of it at h128x7 and 0.64 at h384x2 (1.37 at
# h768x1: caught).  Every other planted defect is a gross error in at least one row (>= 9e3 x the yardstick) and was caught by it as well.
OLD_GATE_MISSES = {("eps_1e-6", "h128x7"), ("eps_1e-6", "h384x2")}


def clean(name):
    if name not in _CLEAN:
        cfg, n_hidden = S.ALL_CFGS[name]
        st, ids = S.seeded_state(cfg), S.id_sets(S.MIXED_LENGTHS)
        _CLEAN[name] = (cfg, n_hidden, st, ids, R.encode_np(st, cfg, ids, torch.float64, n_hidden), R.encode_np(st, cfg, ids, torch.float32, n_hidden))
    return _CLEAN[name]


def test_margins_keep_the_conditions_of_the_planted_defects():
    assert R.BOUNDS["max"] == 8.0 and 1.0 < R.BOUNDS["rms"] <= 6.0 and 1.0 < R.BOUNDS["row"] <= 8.0
    for name in S.CFGS:   # the yardstick passes its own gates with ratios of exactly 1
        cfg, n_hidden, st, ids, d, s = clean(name)
        v = R.ratios(s, d, s)
        assert (v["max"], v["rms"], v["row"]) == (1.0, 1.0, 1.0) and R.judge(name + " clean", s, d, s, say=False) == []
    nan = clean("h128x7")[5].copy()
    nan[17, 3] = np.nan
    assert len(R.judge("nan", nan, clean("h128x7")[4], clean("h128x7")[5], say=False)) == 3   # a NaN fails every gate


@pytest.mark.parametrize("defect,name", [(d, n) for d in R.DEFECTS for n in DEFECT_SHAPES[d]])
def test_planted_defect_fails_a_gate(defect, name):
    """Measured (max / rms / row ratios): eps_1e-6 5.78 / 6.55 / 21 (h128x7), 11 / 13.2 / 15 (h768x1), 5.11 / 7.46 / 10.7 (h384x2) — the
    max-only gate passed the first and the last (on a second CPU 8.66 / 7.58 / 20.2, 10.4 / 16.9 / 19.3, 4.64 / 7.79 / 10.8: the RMS and
    the row ratios keep their distance to the margins 4 and 6, the maximum does not); every other defect >= 9e3 in all three at every shape"""
    cfg, n_hidden, st, ids, d, s = clean(name)
    g = R.encode_np(st, cfg, ids, torch.float32, n_hidden, defect=defect)
    assert np.abs(g - s).max() > 0, "the defect changed nothing at this shape"
    fails = R.judge(f"{name} {defect}", g, d, s)
    assert fails, f"{defect} at {name} passes all three gates"
    old_gate_passes = R.ratios(g, d, s)["max"] <= R.BOUNDS["max"]
    print(f"GLOSSMEAS {name} {defect}: the max-only gate " + ("MISSES it" if old_gate_passes else "catches it"))
    # the recorded misses sit so close to the old gate that the CPU's float32 summation order decides them (h128x7: 5.78 on one machine,
    # 8.66 on another, whose float32 maximum is 1.94e-5 instead of 2.88e-5): recorded and printed, not asserted.  Every other defect is
    # gross (>= 9e3) and the old gate catches it on any machine
    assert not old_gate_passes or (defect, name) in OLD_GATE_MISSES, (defect, name, "the max-only gate missed it")
    if defect == "eps_1e-6":   # a systematic error: the global RMS gate alone must flag it, and so must the row gate
        assert any(" rms " in f for f in fails) and any(" row " in f for f in fails), fails


def test_two_bf16_pieces_is_below_the_yardstick():
    """NOT claimed: the last layer's intermediate.dense weight as two bf16 pieces (2^-17 relative) moves the statistics by 1.0 .. 2.0 at
    these shapes (h768x1: max 1.67, rms 1.86, row 1.98; h128x7: 0.99 / 1.00 / 1.01), inside any margin a float32 yardstick can carry.  A
    comparison of the final mean cannot detect this class reliably; the ratios are printed, nothing about detection is asserted"""
    for name in S.CFGS:
        cfg, n_hidden, st, ids, d, s = clean(name)
        g = R.encode_np(st, cfg, ids, torch.float32, n_hidden, defect="two_bf16_pieces")
        R.judge(f"{name} two_bf16_pieces", g, d, s)
        assert np.isfinite(g).all() and np.abs(g - s).max() > 0


def test_edge_shapes_force_the_branches_they_are_named_after():
    short_tile = lambda c_in: 32 * (2 * ((c_in + 63) // 64 * 64) + 16) * 3   # conv1d.hip: short_lds of an ENG_BF16X6 layer, K = 1
    limit = 150 * 1024
    assert short_tile(768) == 148992 <= limit < short_tile(832) == 161280
    for name, (cfg, n_hidden) in S.EDGE_CFGS.items():
        G.check_config(cfg, n_hidden)
        assert cfg["vocab_size"] == 97 and n_hidden == cfg["num_hidden_layers"] + 1 <= 3
    H = lambda n: S.EDGE_CFGS[n][0]
    assert H("h64_nh1_wideffn")["num_attention_heads"] % 4 == 1 and H("h64_nh1_wideffn")["intermediate_size"] > 4 * 64
    f = H("h192_nh3_pad")["intermediate_size"]
    assert H("h192_nh3_pad")["num_attention_heads"] % 4 == 3 and f % 32 and f % 4 == 0 and ((f + 31) // 32 * 32, (f + 63) // 64 * 64) == (224, 256)
    assert H("h832_generic")["num_attention_heads"] % 4 == 1 and short_tile(H("h832_generic")["intermediate_size"]) <= limit
    assert short_tile(H("h1024_generic")["hidden_size"]) > limit and short_tile(H("h1024_generic")["intermediate_size"]) > limit
    assert [sum(l) for l in S.SEAM_LENGTHS[:5]] == [32, 64, 65, 128, 256] and [max(l) for l in S.SEAM_LENGTHS[5:]] == [2, 33]


def test_intermediate_size_must_be_a_multiple_of_4():
    """output.dense stages rows of intermediate_size floats in 16-byte pieces guarded by their first channel (conv1d.hip): 202 would
    misalign every odd row's loads and read two floats past the last row (0xFF = NaN under debug_redzone, NaN x 0 = NaN)"""
    cfg = S.config(64, 1, 202, 1)
    with pytest.raises(ValueError, match="intermediate_size = 202"):
        G.check_config(cfg, 2)
    with pytest.raises(ValueError, match="intermediate_size = 202"):
        G.GlossEncoder.from_pretrained(S.seeded_state(cfg), cfg, n_hidden=2)
    with pytest.raises(ValueError, match="intermediate_size = 65540"):
        G.check_config(S.config(64, 1, 65540, 1), 2)
    G.check_config(S.config(64, 1, 204, 1), 2)
    G.check_config(S.config(64, 1, 65536, 1), 2)


class FakeEncoder(G.GlossEncoder):
    """build_items on known features: encode returns rows whose value names (gloss, token)"""

    def __init__(self, hidden=8):
        super().__init__()
        self.hidden = hidden
        self.calls = []

    def encode(self, seqs):
        self.calls.append([list(s) for s in seqs])
        return [torch.arange(len(s), dtype=torch.float32)[:, None].repeat(1, self.hidden) + 100 * g for g, s in enumerate(seqs)]


def test_build_items_by_hand():
    enc = FakeEncoder()
    ids3, ids5, ids32 = list(range(3)), list(range(5)), list(range(32))
    entries = {0: [(("zh", "ong1"), ids5)], 2: [(("h", "ang2"), ids3), (("x", "ing2"), ids5), (("h", "ang4"), ids32)]}
    items = enc.build_items(entries, 4)
    assert len(items) == 4 and enc.calls == [[ids5, ids3, ids5, ids32]]   # every gloss of the dictionary in ONE encode call
    one, unk, three, unk2 = items
    assert one["key"] is one["value"] and one["key"].shape == (5, 8) and one["key_map"] == [0, 1, 1, 1, 0]
    assert one["pinyin"] == ["zh", "ong1"] and one["pinyin_map"] == [1, 1] and one["tokens_gloss"] == ids5
    assert torch.equal(one["key"][:, 0], torch.arange(5.0))
    for u in (unk, unk2):   # the binariser's item of a word that the dictionary lacks
        assert u["key"].shape == (3, 8) and not u["key"].any() and not u["value"].any()
        assert (u["key_map"], u["pinyin"], u["pinyin_map"], u["tokens_gloss"]) == ([0, 1, 0], ["<UNK>"], [1], ["O"])
    assert three["key"].shape == (40, 8)
    assert three["key_map"] == [0, 1, 0] + [0, 2, 2, 2, 0] + [0] + [3] * 30 + [0]
    assert three["pinyin"] == ["h", "ang2", "x", "ing2", "h", "ang4"] and three["pinyin_map"] == [1, 1, 2, 2, 3, 3]
    assert torch.equal(three["key"][:, 0], torch.cat([100 + torch.arange(3.0), 200 + torch.arange(5.0), 300 + torch.arange(32.0)]))
    # ... and through the existing reader of dict_embed items
    enc2 = FakeEncoder()
    tab = enc2.build_table(entries, 4)
    assert tab["pinyin_encoder"] == ["<UNK>", "zh", "ong1", "h", "ang2", "x", "ing2", "ang4"]
    assert list(tab["tok_off"]) == [0, 5, 8, 48, 51] and list(tab["pin_off"]) == [0, 2, 3, 9, 10] and tab["values"] is None
    assert list(tab["pinyin"]) == [1, 2, 0, 3, 4, 5, 6, 3, 7, 0] and tab["keys"].shape == (51, 8)
    assert np.array_equal(tab["key_map"][5:8], [0, 1, 0]) and tab["key_map"].dtype == np.float32
    again = dict_embed.table_from_items(items, tab["pinyin_encoder"])
    assert all(np.array_equal(again[k], tab[k]) for k in ("tok_off", "keys", "key_map", "pin_off", "pinyin", "pinyin_map"))
    with pytest.raises(ValueError, match="word id 9"):
        FakeEncoder().build_items({9: entries[0]}, 4)


def test_refusals_without_a_device(tmp_path):
    cfg, n_hidden = S.CFGS["h128x7"]
    st = S.seeded_state(cfg)
    for bad, word in (({"num_attention_heads": 4}, "heads of 64"), ({"hidden_size": 96, "num_attention_heads": 1}, "multiple of 64"),
                      ({"embedding_size": 64}, "embedding_size = 64"), ({"rotary_value": True}, "rotary_value"),
                      ({"hidden_act": "relu"}, "hidden_act = 'relu'"), ({"hidden_act": "gelu_new"}, "erf GELU")):
        with pytest.raises(ValueError, match=re.escape(word)):
            G.GlossEncoder.from_pretrained(st, {**cfg, **bad}, n_hidden=n_hidden)
    with pytest.raises(ValueError, match="n_hidden = 9"):
        G.GlossEncoder.from_pretrained(st, cfg, n_hidden=9)
    with pytest.raises(ValueError, match="needs its config"):
        G.GlossEncoder.from_pretrained(st)
    key = "encoder.layer.3.output.LayerNorm.bias"
    with pytest.raises(KeyError, match=re.escape(key)):
        G.GlossEncoder.from_pretrained({k: v for k, v in st.items() if k != key}, cfg, n_hidden=8)
    # ... which a shallower encoder does not need; layers behind n_hidden - 2, the MLM head and the position table are not taken
    enc = G.GlossEncoder.from_pretrained({"roformer." + k: torch.from_numpy(v) for k, v in st.items() if k != key}, cfg, n_hidden=4)
    assert max(int(k.split(".")[2]) for k in enc.weights if k.startswith("encoder.layer.")) == 2 and len(enc.weights) == 4 + 3 * 16
    with pytest.raises(ValueError, match=r"word_embeddings.weight is \[97, 64\]"):
        G.GlossEncoder.from_pretrained({**st, "embeddings.word_embeddings.weight": np.zeros((97, 64), np.float32)}, cfg)
    with pytest.raises(ValueError, match="row_budget"):
        G.GlossEncoder(row_budget=63)
    with pytest.raises(abi.DttsError, match="no weights"):
        G.GlossEncoder().encode([[1, 2, 3]])
    enc = G.GlossEncoder.from_pretrained(st, cfg, n_hidden=n_hidden)
    assert list(enc._state()["config"]) == [2.0, np.float32(1e-12), 0.0, 0.0]
    for seqs, word in (([[1] * 65], "gloss 0 has L = 65"), ([[1, 2], []], "gloss 1 has L = 0")):
        with pytest.raises(ValueError, match=word):
            enc.encode(seqs)
    if not torch.cuda.is_available():
        with pytest.raises(abi.DttsError, match="needs a ROCm GPU"):
            enc.encode([[1, 2, 3]])
    # a model directory: the configuration is refused before the checkpoint is opened
    (tmp_path / "config.json").write_text(json.dumps({**cfg, "rotary_value": True}))
    with pytest.raises(ValueError, match="rotary_value"):
        G.GlossEncoder.from_pretrained(str(tmp_path))
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    torch.save({"roformer." + k: torch.from_numpy(v) for k, v in st.items()}, tmp_path / "pytorch_model.bin")
    enc = G.GlossEncoder.from_pretrained(str(tmp_path))
    assert enc.n_hidden == 8 and enc.vocab == S.VOCAB and all(np.array_equal(enc.weights[k], st[k]) for k in enc.weights)


def test_argument_block_is_checked_before_the_handle():
    """the refusals of dtts_text2mel_fetch(DTTS_GLOSS_ENCODE) are reachable without a device: a NULL handle is the last thing looked at"""
    lib = abi.load_library()
    call = lambda a: (lib.dtts_text2mel_fetch(None, abi.GLOSS_ENCODE, C.byref(a), None), lib.dtts_last_error(None).decode())
    ok = dict(n_gloss=2, ids=256, tok_off=256, sum_L=40, L_max=32, out=256, status=256)
    text = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    fields = re.search(r"typedef struct dtts_gloss_args \{(.*?)\} dtts_gloss_args;", text, re.S).group(1)
    assert len(re.findall(r"int32_t \w+;", fields)) == 4 and len(re.findall(r"\* ?\w+;", fields)) == 4
    assert C.sizeof(abi.GlossArgs) == 4 * 4 + 4 * 8 == 48
    assert f"#define DTTS_PART_GLOSS {abi.PART_GLOSS}" in text and f"#define DTTS_GLOSS_MAX_L {abi.GLOSS_MAX_L}" in text
    # the encoder goes through the dispatcher of the block items: no entry point of its own, and no DTTS_OUT_* output item either
    assert f"#define DTTS_GLOSS_ENCODE {abi.GLOSS_ENCODE}" in text and abi.GLOSS_ENCODE not in abi.OUT_NAMES
    assert len(abi.EXPORTS) == 32 and not [s for s in abi.EXPORTS if "gloss" in s]
    a = abi.gloss_args(**ok)
    a.size -= 8
    assert call(a)[0] == -22 and "size" in call(a)[1]
    assert lib.dtts_text2mel_fetch(None, abi.GLOSS_ENCODE, None, None) == -22
    for bad, word in ((dict(n_gloss=0), "n_gloss = 0"), (dict(L_max=0), "L_max = 0"), (dict(L_max=65, sum_L=70), "L_max = 65"), (dict(sum_L=1), "sum_L = 1"),
                      (dict(sum_L=65), "sum_L = 65"), (dict(out=None), "null"), (dict(ids=260), "ids_dev"), (dict(tok_off=258), "tok_off_dev"),
                      (dict(out=264), "out_dev")):
        rc, msg = call(abi.gloss_args(**{**ok, **bad}))
        assert rc == -22 and word in msg, (bad, rc, msg)
    rc, msg = call(abi.gloss_args(**ok))
    assert rc == -22 and msg == "dtts_text2mel_fetch(DTTS_GLOSS_ENCODE): null handle"
