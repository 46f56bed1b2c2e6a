"""The in-place dictionary edit without a GPU: the two block items of include/dicttts_hip.h (DTTS_DICT_EDIT 69, DTTS_DICT_ENTRY 70) refuse a
short block, a null handle and a bad argument in the shared wording of the block-first units (tests/test_fetch_units_cpu.py shows the
form); they stand outside the DTTS_OUT_* numbering; the host packing of an edit is the packing of ``dict_embed.table_from_items``; and
``GlossEncoder.build_items`` without its new flag returns what it returned before."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dict_edit_shapes as S
from dict_tts_amd import abi, dict_embed
from dict_tts_amd import gloss_encoder as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDIT, ENTRY = "dtts_text2mel_fetch(DTTS_DICT_EDIT)", "dtts_text2mel_fetch(DTTS_DICT_ENTRY)"


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def fetch(lib, what, block):
    rc = lib.dtts_text2mel_fetch(None, what, C.byref(block), None)
    return rc, lib.dtts_last_error(None).decode()


class Edit:
    """a well-formed two-entry edit in host arrays (kept alive by the object); ``block`` points into them"""

    def __init__(self):
        self.ids, self.tok_off, self.pin_off = np.array([1, 3], np.int32), np.array([0, 2, 5], np.int32), np.array([0, 2, 4], np.int32)
        self.key_map, self.pinyin, self.pinyin_map = np.zeros(5, np.float32), np.zeros(4, np.int64), np.ones(4, np.int64)
        self.keys = np.zeros((5, 768), np.float32)

    def block(self, **kw):
        p = lambda a: a.ctypes.data
        return abi.dict_edit_args(2, p(self.ids), p(self.tok_off), p(self.pin_off), p(self.key_map), p(self.pinyin), p(self.pinyin_map),
                                  kw.pop("keys", p(self.keys)), **kw)


def test_the_items_word_size_and_handle_like_the_block_first_units(lib):
    e = Edit()
    for what, name, make in ((abi.DICT_EDIT, EDIT, e.block), (abi.DICT_ENTRY, ENTRY, lambda: abi.dict_entry_args(0, k=0x1000, pinyin=0x2000))):
        a = make()
        a.size -= 8
        rc, msg = fetch(lib, what, a)
        assert rc == -22 and msg == f"{name}: argument block of size = {C.sizeof(a) - 8} bytes, this library's is {C.sizeof(a)}", (rc, msg)
        rc, msg = fetch(lib, what, make())
        assert rc == -22 and msg == f"{name}: null handle", (rc, msg)
    assert fetch(lib, abi.DICT_EDIT, e.block(rows_on_device=True, keys=0x1000)) == (-22, f"{EDIT}: null handle")   # device rows: aligned
    assert lib.dtts_text2mel_fetch(None, abi.DICT_EDIT, None, None) == -22 and lib.dtts_text2mel_fetch(None, abi.DICT_ENTRY, None, None) == -22


def test_argument_refusals_precede_the_handle(lib):
    """each names its cause; none needs a device.  (A gap before the appended ids, a missing table and unfinalised weights need the
    context: tests/test_dict_edit_gpu.py)"""
    def refused(change, word):
        e = Edit()
        kw = change(e) or {}
        rc, msg = fetch(lib, abi.DICT_EDIT, e.block(**kw))
        assert rc == -22 and msg.startswith(EDIT + ": ") and word in msg, (rc, msg)

    def set_(name, i, v):
        return lambda e: getattr(e, name).__setitem__(i, v)

    refused(set_("ids", 1, 1), "strictly ascending (entry_id[1] = 1 after 1)")
    refused(set_("ids", slice(None), [3, 1]), "strictly ascending (entry_id[1] = 1 after 3)")
    refused(set_("ids", 0, -1), "non-negative")
    refused(set_("tok_off", slice(None), [0, 3, 2]), "offsets must be non-decreasing (edit 1, entry 3)")
    refused(set_("pin_off", slice(None), [0, 5, 4]), "offsets must be non-decreasing (edit 1, entry 3)")
    refused(set_("tok_off", 0, 1), "tok_off[0] = 1")
    refused(set_("pinyin_map", 3, 16), "entry 3 has sense index 16; at most 15 senses per word are supported")   # the upload's wording
    refused(set_("key_map", 0, 16.0), "entry 1 has sense index 16; at most 15 senses per word are supported")
    refused(set_("tok_off", 2, 2 ** 30), f"{2 ** 30} gloss rows")                                                   # more than INT_MAX / 2 rows
    refused(lambda e: {"keys": 0}, "null keys")
    refused(lambda e: {"rows_on_device": True, "keys": 0x1008}, "keys = 0x1008 is not aligned to 16 bytes")
    a = Edit().block()
    a.n_edit = -1
    rc, msg = fetch(lib, abi.DICT_EDIT, a)
    assert rc == -22 and "n_edit = -1" in msg
    rc, msg = fetch(lib, abi.DICT_ENTRY, abi.dict_entry_args(-2))
    assert rc == -22 and msg.startswith(ENTRY) and "entry = -2" in msg
    rc, msg = fetch(lib, abi.DICT_ENTRY, abi.dict_entry_args(0, pinyin_map=0x1004))
    assert rc == -22 and msg == f"{ENTRY}: pinyin_map_dev = 0x1004 is not aligned to 8 bytes"


def test_the_items_stand_outside_the_out_numbering():
    with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as f:
        text = f.read()
    defs = {n: int(v) for n, v in re.findall(r"^#define (DTTS_\w+) (\d+)\b", text, re.M)}
    assert defs["DTTS_DICT_EDIT"] == abi.DICT_EDIT == 69 and defs["DTTS_DICT_ENTRY"] == abi.DICT_ENTRY == 70
    assert defs["DTTS_PS_DECODER_INP"] == 68 and defs["DTTS_MAX_SENSES"] == abi.MAX_SENSES
    assert not any(n.startswith("DTTS_OUT_") and v in (69, 70) for n, v in defs.items())
    assert abi.DICT_EDIT not in abi.OUT_NAMES and abi.DICT_ENTRY not in abi.OUT_NAMES
    assert defs["DTTS_TIMER_DICT_SEG_COPY"] == abi.TIMER_DICT_SEG_COPY == defs["DTTS_TIMER_COUNT"] - 1
    # the blocks of abi.py are the header's structs, field for field
    for cls, name in ((abi.DictEditArgs, "dtts_dict_edit_args"), (abi.DictEntryArgs, "dtts_dict_entry_args")):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], (fields, [f[0] for f in cls._fields_])


class Recorder:
    """stands in for abi.Context under PortaSpeech_dict.edit_dict_table: keeps what the library would be handed"""

    def __init__(self, n_entries):
        self.n, self.calls = n_entries, []

    def dict_table_entry(self, entry, stream, **dst):
        return self.n, 0, 0

    def dict_table_edit(self, *a, **kw):
        self.calls.append((a, kw))


def edit_on_recorder(n_entries, replace, append, monkeypatch, **kw):
    from dict_tts_amd import model as M
    m = M.PortaSpeech_dict.__new__(M.PortaSpeech_dict)
    torch.nn.Module.__init__(m)
    m.ctx, m.cfg, m.device = Recorder(n_entries), abi.DttsConfig(gloss_dim=768, hidden_size=192), torch.device("cpu")
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: type("S", (), {"cuda_stream": None})())
    new_ids = m.edit_dict_table(replace, append, **kw)
    (a, k), = m.ctx.calls
    return new_ids, a, k


@pytest.mark.parametrize("own_value", [False, True])
def test_the_host_packing_of_an_edit_is_table_from_items(monkeypatch, own_value):
    """edit_dict_table hands the library the ragged arrays table_from_items makes of the same items, in ascending id order, appended last"""
    rep, app = S.mixed(own_value)
    order = sorted(rep)
    new_ids, a, k = edit_on_recorder(S.N_BASE, {e: rep[e] for e in reversed(order)}, app, monkeypatch)
    ids, tok_off, pin_off, key_map, pinyin, pinyin_map, keys, values, _ = a
    assert new_ids == [S.N_BASE, S.N_BASE + 1] and list(ids) == order + new_ids and k == {"rows_on_device": False}
    enc = [f"p{i}" for i in range(64)]   # a pinyin encoder whose token i is id i: table_from_items looks tokens up
    items = [{**it, "pinyin": [enc[i] for i in it["pinyin"]], "value": it.get("value", it["key"])} for it in [rep[e] for e in order] + app]
    want = dict_embed.table_from_items(items, enc)
    for got, name in ((tok_off, "tok_off"), (pin_off, "pin_off"), (key_map, "key_map"), (pinyin, "pinyin"), (pinyin_map, "pinyin_map"), (keys, "keys")):
        assert np.array_equal(got, want[name]) and np.asarray(got).dtype == want[name].dtype, name
    assert (values is None) == (want["values"] is None) == (not own_value)
    if own_value:
        assert np.array_equal(values, want["values"])
    # tokens through a pinyin encoder give the same arrays; CPU tensors are host rows too
    t_items = [{**it, "key": torch.from_numpy(it["key"]), "value": torch.from_numpy(it["value"])} for it in items]
    _, a2, k2 = edit_on_recorder(S.N_BASE, dict(zip(order, t_items)), t_items[len(order):], monkeypatch, pinyin_encoder=enc)
    assert all(np.array_equal(x, y) for x, y in zip(a[:7], a2[:7])) and k2 == {"rows_on_device": False}
    # nothing to do is still one (empty) call: the library answers n_edit = 0
    new_ids, a0, _ = edit_on_recorder(S.N_BASE, None, None, monkeypatch)
    assert new_ids == [] and len(a0[0]) == 0 and list(a0[1]) == [0] and a0[6].shape == (0, 768)
    with pytest.raises(ValueError, match="replace names entry 24"):
        edit_on_recorder(S.N_BASE, {S.N_BASE: app[0]}, None, monkeypatch)
    with pytest.raises(ValueError, match="gloss_dim = 768"):
        edit_on_recorder(S.N_BASE, None, [{**app[0], "key": app[0]["key"][:, :64], "value": None}], monkeypatch)


def test_pack_items_and_the_edited_dictionary():
    """the shapes module's own yardstick: apply() edits the item list, table_of() packs it as table_from_items would"""
    base = S.base_items()
    assert len(base) == S.N_BASE and {it["key"].shape[0] for it in base} >= {0, 1} and max(it["key"].shape[0] for it in base) <= 40
    for name, (rep, app) in S.edits().items():
        new = S.apply(base, rep, app)
        t = S.table_of(new)
        assert len(new) == S.N_BASE + len(app) and t["tok_off"][-1] == sum(it["key"].shape[0] for it in new) == t["keys"].shape[0], name
        assert t["key_map"].max() <= abi.MAX_SENSES and t["pinyin_map"].max() <= abi.MAX_SENSES
        assert sorted(w for s in S.sentences(len(new)) for w in s) == sorted(t["ids"])   # the batch uses every entry
    assert all(len(rep) + len(app) <= 1 for rep, app in S.single_edits().values())
    assert len(base) == S.N_BASE   # apply() copies


class FakeEncoder(G.GlossEncoder):
    def __init__(self, hidden=8):
        self.hidden = hidden

    def encode(self, seqs):
        return [torch.arange(len(s), dtype=torch.float32)[:, None].repeat(1, self.hidden) + 100 * g for g, s in enumerate(seqs)]


def test_build_items_without_the_flag_is_unchanged():
    entries = {0: [(("zh", "ong1"), list(range(5)))], 2: [(("h", "ang2"), list(range(3))), (("x", "ing2"), list(range(5)))]}
    a, b = FakeEncoder().build_items(entries, 4), FakeEncoder().build_items(entries, 4, device=False)
    for x, y in zip(a, b):
        assert x.keys() == y.keys() == {"tokens_gloss", "key", "key_map", "value", "pinyin", "pinyin_map"}
        assert torch.equal(x["key"], y["key"]) and torch.equal(x["value"], y["value"]) and x["key"].device.type == "cpu"
        assert all(x[k] == y[k] for k in ("tokens_gloss", "key_map", "pinyin", "pinyin_map"))
    one, unk, two, _ = a
    assert one["key"] is one["value"] and one["key_map"] == [0, 1, 1, 1, 0] and two["key"].shape == (8, 8)
    assert unk["key"].shape == (3, 8) and not unk["key"].any() and unk["key"] is not unk["value"] and unk["pinyin"] == ["<UNK>"]
