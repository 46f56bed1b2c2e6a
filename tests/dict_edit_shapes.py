"""Dictionaries and edits for the tests of the in-place dictionary edit (tests/test_dict_edit_cpu.py, tests/test_dict_edit_gpu.py).

A dictionary here is a list of ``dict_embed`` items (key f32 [L, 768], key_map [L], pinyin ids [P], pinyin_map [P], optional value).  The
base has 24 entries of 0 .. 40 gloss rows: 22 entries of the Biaobei structure file through ``synth.dict_table(SEED, entries=subset)``, plus
an entry of ONE row at index 5 and one of NO row at index 17.  An edit is (replace {index: item}, append [items]); ``apply`` gives the edited
dictionary, whose fresh upload is the yardstick of every case."""
import numpy as np

from dict_tts_amd import dict_embed, synth

SEED = 1234
D = synth.GLOSS_DIM
N_BASE = 24
ONE_ROW, NO_ROW = 5, 17       # where the base keeps its entry of one row / of no row
WORD0 = 10                    # entry e is word WORD0 + e of the sentences (any id below word_size)


def item(name, L, senses=1, seed=SEED, own_value=False):
    """a seeded item of L gloss rows spread over ``senses`` senses (the first and last row of a sense are its [CLS] / [SEP]: key_map 0), with
    two pinyin slots per sense.  L < 2 * senses keeps every row live.  own_value: a value that differs from the key"""
    key = synth.randn(seed, f"edit.{name}.key", (L, D), 0.5)
    per = [L // senses + (1 if s < L % senses else 0) for s in range(senses)]
    key_map, pinyin, pinyin_map = [], [], []
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    for s, n in enumerate(per):
        key_map += ([0] + [s + 1] * (n - 2) + [0]) if n > 2 else [s + 1] * n
        pinyin += [int(v) for v in rng.integers(1, 60, 2)]
        pinyin_map += [s + 1, s + 1]
    it = {"key": key, "key_map": np.array(key_map, np.float32), "pinyin": np.array(pinyin, np.int64), "pinyin_map": np.array(pinyin_map, np.int64)}
    if own_value:
        it["value"] = synth.randn(seed, f"edit.{name}.value", (L, D), 0.5)
    return it


def items_of(table):
    """the items of a ragged table (synth.dict_table / table_of)"""
    out = []
    for e in range(len(table["L"])):
        a, b, p, q = table["tok_off"][e], table["tok_off"][e + 1], table["pin_off"][e], table["pin_off"][e + 1]
        it = {"key": table["keys"][a:b], "key_map": table["key_map"][a:b], "pinyin": table["pinyin"][p:q], "pinyin_map": table["pinyin_map"][p:q]}
        if table.get("values") is not None:
            it["value"] = table["values"][a:b]
        out.append(it)
    return out


def table_of(items):
    """items -> the ragged arrays of upload_dict_table; ``ids`` maps word WORD0 + e to entry e (synth.make_id_batch reads it)"""
    p = dict_embed.pack_items(items)   # (table_from_items looks pinyin tokens up; these items hold ids)
    return {"ids": {WORD0 + e: e for e in range(len(items))}, "tok_off": p["tok_off"], "pin_off": p["pin_off"], "keys": np.concatenate(p["keys"]),
         "values": None if p["same"] else np.concatenate(p["values"]), "key_map": p["key_map"], "pinyin": p["pinyin"], "pinyin_map": p["pinyin_map"],
         "L": np.diff(p["tok_off"]), "P": np.diff(p["pin_off"])}


_BASE = None


def base_items():
    """the 24 base entries (the same list object every time: a reference computed once; never modified)"""
    global _BASE
    if _BASE is None:
        ent = synth.biaobei_struct()["entries"]
        subset = {w: ent[w] for w in [w for w in sorted(ent) if ent[w][0][2] >= 0 and sum(s[0] for s in ent[w]) <= 40][:N_BASE - 2]}
        its = items_of(synth.dict_table(SEED, entries=subset))
        its.insert(ONE_ROW, item("base.one", 1))
        its.insert(NO_ROW, item("base.none", 0))
        assert len(its) == N_BASE and its[ONE_ROW]["key"].shape[0] == 1 and its[NO_ROW]["key"].shape[0] == 0
        _BASE = its
    return _BASE


def apply(items, replace=None, append=None):
    """the edited dictionary"""
    out = list(items)
    for e, it in (replace or {}).items():
        out[e] = it
    return out + list(append or [])


def rows(e):
    return base_items()[e]["key"].shape[0]


FIRST, MID, LAST = 0, 11, N_BASE - 1


def single_edits():
    """name -> (replace, append): the first, a middle and the last entry, each with more rows, fewer rows and the same number; the one-row and
    the no-row entry as the victim and as the replacement"""
    c = {}
    for where, e in (("first", FIRST), ("mid", MID), ("last", LAST)):
        L = rows(e)
        assert L >= 4
        for how, n in (("more", L + 7), ("fewer", L - 3), ("same", L)):
            c[f"{where}_{how}"] = ({e: item(f"{where}.{how}", n, senses=2 if how == "more" else 1)}, [])
    c["victim_one_row"] = ({ONE_ROW: item("v1", 9, senses=3)}, [])
    c["victim_no_row"] = ({NO_ROW: item("v0", 4)}, [])
    c["to_one_row"] = ({8: item("r1", 1)}, [])
    c["to_no_row"] = ({14: item("r0", 0)}, [])
    return c


def all_in_one():
    s = single_edits()
    rep = {}
    for name in ("first_more", "mid_fewer", "last_same", "victim_one_row", "victim_no_row", "to_one_row", "to_no_row"):
        rep.update(s[name][0])
    return rep, []


def mixed(own_value=False):
    """a replace-and-append edit: a longer first entry, a shorter middle one, the no-row entry filled, two appended entries (one of one row)"""
    rep = {FIRST: item("mx.a", rows(FIRST) + 5, senses=2, own_value=own_value), MID: item("mx.b", rows(MID) - 2, own_value=own_value),
           NO_ROW: item("mx.c", 6, own_value=own_value)}
    return rep, [item("mx.d", 13, senses=3, own_value=own_value), item("mx.e", 1, own_value=own_value)]


def edits():
    """every (name -> edit) of the first three groups of the issue's list"""
    c = dict(single_edits())
    c["all_in_one_call"] = all_in_one()
    c["append_1"] = ({}, [item("ap.0", 12, senses=2)])
    c["append_5"] = ({}, [item(f"ap5.{i}", L, senses=1 + i % 3) for i, L in enumerate((3, 40, 1, 0, 17))])
    c["append_and_replace"] = mixed()
    c["every_second"] = ({e: item(f"e2.{e}", (e * 7) % 23 + 1) for e in range(0, N_BASE, 2)}, [])     # every unchanged run has length 1
    c["replace_all"] = ({e: item(f"all.{e}", (e * 5) % 31) for e in range(N_BASE)}, [])               # no unchanged run
    c["n_edit_0"] = ({}, [])
    return c


def sentences(n_entries):
    """three sentences that together use EVERY entry of a dictionary of n_entries: unchanged, replaced and appended ones"""
    words = [WORD0 + e for e in range(n_entries)]
    k = (n_entries + 2) // 3
    return [words[:k], words[k:2 * k], words[2 * k:]]


def collate(table, sents):
    """the tensors DictTTSDataset.collater would build from the table for these sentences (synth.make_batch's layout)"""
    ib = synth.make_id_batch(sents, table, pron_every=3)
    B, Tw = ib["word_tokens"].shape
    keys = np.zeros((B, Tw, ib["L_k"], D), np.float32)
    values = np.zeros_like(keys)
    key_map, pinyin = np.zeros((B, Tw, ib["L_k"]), np.float32), np.zeros((B, Tw, ib["P"]), np.int64)
    pinyin_map = np.zeros_like(pinyin)
    tv = table["values"] if table.get("values") is not None else table["keys"]
    for b, s in enumerate(sents):
        for t, w in enumerate(s):
            e = table["ids"][w]
            a, z, p, q = table["tok_off"][e], table["tok_off"][e + 1], table["pin_off"][e], table["pin_off"][e + 1]
            keys[b, t + 1, :z - a], values[b, t + 1, :z - a], key_map[b, t + 1, :z - a] = table["keys"][a:z], tv[a:z], table["key_map"][a:z]
            pinyin[b, t + 1, :q - p], pinyin_map[b, t + 1, :q - p] = table["pinyin"][p:q], table["pinyin_map"][p:q]
    key_map[:, [0, -1]] = 1
    pinyin_map[:, [0, -1]] = 1
    return ib, {"keys": keys, "values": values, "key_map": key_map, "pinyin": pinyin, "pinyin_map": pinyin_map}
