"""S2PA (dict_tts_amd/csrc/ops.hip: s2pa_kernel) along its own axes: a synthetic dictionary built from per-entry tuples, both input forms
from the same tuples, the kernel's row -> (wave, step, group) rules restated from its constants, a float64 restatement of its partition
that can plant defects, and the case table of tests/test_s2pa_cpu.py and tests/test_s2pa_gpu.py (test infrastructure).

An entry is the tuple synth.dict_entry returns, ``(emb [L,768], key_map [L], pinyin [P], pinyin_map [P])``, with an optional fifth
element ``values [L,768]`` (the reference stores value == key; a separate array makes a dropped VALUE row visible at a flat gloss scale,
where keys of std 0.02 would shrink the context with them).  ``table`` lays entries out as synth.dict_table does, ``collate`` as
synth.make_batch does (the all-ones first and last padded rows included); synth.make_id_batch supplies entry -1 / -2.

Gloss scales.  With the synthetic weights and synth.dict_entry's gloss std 0.5 the softmax is almost one-hot (largest weight 0.84-1.00),
so a row that is dropped, read twice or merged with the wrong factor barely moves the outputs unless it is the dominant one.  At FLAT
(std 0.02) the weights of n live rows stay within a small factor of 1/n and every row counts.  Every row-count and pattern case runs at
both.  Glosses are never scaled ABOVE the synthetic default: the fp32 oracle's own context error grows with the scale (3.9e-5 at 8x,
more than half the bound).
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import acoustic_ref as ar
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    """S2PA_* out of ops.hip and DTTS_MAX_SENSES out of the public header, by regex (as fft_shapes.py / rbn_shapes.py do)"""
    with open(os.path.join(_ROOT, "dict_tts_amd", "csrc", "ops.hip")) as f:
        src = f.read()
    with open(os.path.join(_ROOT, "include", "dicttts_hip.h")) as f:
        hdr = f.read()
    out = {}
    for name in ("S2PA_LMAX", "S2PA_NW", "S2PA_RU", "S2PA_RU_P", "S2PA_NTHR"):
        m = re.search(rf"constexpr int [^;]*\b{name} = ([^,;]+)[,;]", src)
        assert m, name
        out[name] = int(eval(m.group(1), {}, dict(out)))   # S2PA_NTHR = S2PA_NW * 64
    out["DTTS_MAX_SENSES"] = int(re.search(r"#define DTTS_MAX_SENSES (\d+)", hdr).group(1))
    return out


C = _constants()
LMAX, NW, RU, RU_P, NTHR, MAX_SENSES = (C[k] for k in ("S2PA_LMAX", "S2PA_NW", "S2PA_RU", "S2PA_RU_P", "S2PA_NTHR", "DTTS_MAX_SENSES"))
PEAKED, FLAT = 0.5, 0.02
GD = synth.GLOSS_DIM


# ------------------------------------------------------------------------------------------------------------- partition rules
# Each rule twice: the closed form the issue states, and the kernel's loop restated literally.  test_s2pa_cpu.py checks that both agree
# and cover every row exactly once.
def table_slot(l):
    """table form: row l -> (wave, step, 16-lane group)"""
    return (l // 4) % NW, l // (4 * NW), l % 4


def table_loop(nrow):
    """s2pa_kernel<.., true>'s stream: wave w starts at i = 4 w, takes rows i .. i + 3 (group g takes i + g), steps by 4 NW.
    -> {(wave, group): [rows in step order]}; a slot past the entry (l >= nrow) is the clamped read of row 0 and is NOT a row"""
    out = {(w, g): [] for w in range(NW) for g in range(4)}
    for w in range(NW):
        i = 4 * w
        while i < nrow:
            for g in range(4):
                if i + g < nrow:
                    out[(w, g)].append(i + g)
            i += 4 * NW
    return out


def list_chunk(pos, rv):
    """tensor form: listed position pos -> (chunk, wave): chunk c of rv = RU / 2 listed rows goes to wave c % NW"""
    return pos // rv, (pos // rv) % NW


def list_loop(n, rv, alias):
    """the list-driven loops: -> {wave: [chunk = [listed positions]]} in the order the wave folds them.  The alias form keeps chunks c and
    c + NW of a wave in flight together and leaves the second out when it starts past the list (`if (i0 >= n) break`)"""
    out = {w: [] for w in range(NW)}
    for w in range(NW):
        if alias:
            for i in range(w * rv, n, 2 * NW * rv):
                for h in range(2):
                    i0 = i + h * NW * rv
                    if i0 >= n:
                        break
                    out[w].append(list(range(i0, min(i0 + rv, n))))
        else:
            for i in range(w * rv, n, NW * rv):
                out[w].append(list(range(i, min(i + rv, n))))
    return out


def strided(L):
    """fill, softmax and dict_attn loops: thread tid takes l = tid, tid + NTHR, ... -> {tid: [rows]}"""
    return {tid: list(range(tid, L, NTHR)) for tid in range(NTHR)}


def ballot_bases(nrow):
    """the live-row list: wave 0 ballots 64 rows per base -> [(base, [rows of the base])]"""
    return [(b, list(range(b, min(b + 64, nrow)))) for b in range(0, nrow, 64)]


def sense_rows(L):
    """the sense merge: thread 16 j + i (j = tid >> 4 in [0, NTHR / 16)) sums the rows l = j (mod 16) of sense i -> {j: [rows]}"""
    assert NTHR // 16 == 16
    return {j: list(range(j, L, 16)) for j in range(NTHR // 16)}


def pinyin_fours(P):
    """the pinyin mix: slots p0 .. p0 + 3 in flight, p0 stepping by 4, the last group cut at P"""
    return [list(range(p0, min(p0 + 4, P))) for p0 in range(0, P, 4)]


def nolive_loop(nrow):
    """the no-live-row path: wave w takes rows l0 + j NW (j < 4) for l0 = w, w + 4 NW, ... -> {wave: [rows]}"""
    out = {w: [] for w in range(NW)}
    for w in range(NW):
        for l0 in range(w, nrow, 4 * NW):
            for j in range(4):
                if l0 + j * NW >= nrow:
                    break
                out[w].append(l0 + j * NW)
    return out


# ------------------------------------------------------------------------------------------------------------- entries
def entry(name, key_map, pinyin_map=None, pinyin=None, scale=PEAKED, zero_rows=(), values_scale=None):
    """one dictionary entry.  key_map decides which rows are live; pinyin_map defaults to two slots per sense of key_map (one sense when
    no row is live), pinyin to ids in [1, N_PINYIN); values_scale: a separate `values` array of that std"""
    km = np.asarray(key_map, np.float32)
    emb = synth.randn(ar.SEED, f"s2pa.{name}", (len(km), GD), scale)
    emb[list(zero_rows)] = 0
    if pinyin_map is None:
        senses = sorted(set(int(k) for k in km) - {0}) or [1]
        pinyin_map = [s for s in senses for _ in range(2)]
    pm = np.asarray(pinyin_map, np.int64)
    if pinyin is None:
        pinyin = 1 + (np.arange(len(pm)) * 7 + len(km)) % (synth.N_PINYIN - 1)
    py = np.asarray(pinyin, np.int64)
    assert py.shape == pm.shape
    if values_scale is None:
        return emb, km, py, pm
    val = synth.randn(ar.SEED, f"s2pa.{name}.values", (len(km), GD), values_scale)
    return emb, km, py, pm, val


def natural(sizes):
    """dict_entry's own pattern: sense i of n gloss tokens is [0] + [i] * (n - 2) + [0] (the first and last token of a sense are masked)"""
    km = []
    for i, n in enumerate(sizes):
        km += [0] + [i + 1] * (n - 2) + [0]
    return km


def pattern(kind, L):
    """the live patterns -> (key_map, zero_rows)"""
    l = np.arange(L)
    z = ()
    if kind == "all_live":
        km = np.ones(L)
    elif kind == "first_only":
        km = (l == 0)
    elif kind == "last_only":
        km = (l == L - 1)
    elif kind == "one_per_group":          # rows 21 g (5 g in a short entry): group g of wave g, each at its own step
        km = np.isin(l, [(21 if L >= 64 else 5) * g for g in range(4)])
    elif kind == "wave3_only":
        km = (l // 4) % NW == NW - 1
    elif kind == "alternate":
        km = l % 2 == 0
    elif kind == "natural":
        a = L // 3
        km = np.array(natural([a, a, L - 2 * a]))
    elif kind == "none_live":
        km = np.zeros(L)
    elif kind == "zero_row":               # live all-zero rows (the unknown-character entry has one): logit exactly 0
        km = np.ones(L)
        z = (1, L - 1)
    else:
        raise KeyError(kind)
    return np.asarray(km, np.float32), z


PATTERNS = ("all_live", "first_only", "last_only", "one_per_group", "wave3_only", "alternate", "natural", "none_live", "zero_row")
ROWS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 148, 255, 256, 257)


# ------------------------------------------------------------------------------------------------------------- both input forms
def table(entries):
    """the resident table of a list of entries (word id = 3 + index), synth.dict_table's layout (+ 'values' when an entry has its own)"""
    tok_off = np.zeros(len(entries) + 1, np.int32)
    pin_off = np.zeros(len(entries) + 1, np.int32)
    for i, e in enumerate(entries):
        tok_off[i + 1] = tok_off[i] + e[0].shape[0]
        pin_off[i + 1] = pin_off[i] + e[2].shape[0]
    t = {"ids": {3 + i: i for i in range(len(entries))}, "tok_off": tok_off, "pin_off": pin_off,
         "keys": np.concatenate([e[0] for e in entries]), "key_map": np.concatenate([e[1] for e in entries]),
         "pinyin": np.concatenate([e[2] for e in entries]), "pinyin_map": np.concatenate([e[3] for e in entries]),
         "L": np.diff(tok_off), "P": np.diff(pin_off)}
    if any(len(e) > 4 for e in entries):
        t["values"] = np.concatenate([e[4] if len(e) > 4 else e[0] for e in entries])
    return t


def collate(entries, sentences, pron=None, valid=None):
    """the collated tensors of sentences (lists of word ids 3 + index), built the way synth.make_batch builds them.  pron: {(b, t): sense}
    -> pron_modified; valid: per utterance, the number of valid words (word_tokens is zeroed from there on: the words after it are DEAD
    but keep their dictionary rows)"""
    B = len(sentences)
    items = [[entries[w - 3] for w in s] for s in sentences]
    Tw = max(len(s) for s in sentences) + 2
    Lk = max([e[0].shape[0] for it in items for e in it] + [1])
    P = max([e[2].shape[0] for it in items for e in it] + [1])
    word_tokens = np.zeros((B, Tw), np.int64)
    keys = np.zeros((B, Tw, Lk, GD), np.float32)
    values = np.zeros((B, Tw, Lk, GD), np.float32)
    key_map = np.zeros((B, Tw, Lk), np.float32)
    pinyin = np.zeros((B, Tw, P), np.int64)
    pinyin_map = np.zeros((B, Tw, P), np.int64)
    pron_modified = np.zeros((B, Tw), np.int64)
    for b, (s, it) in enumerate(zip(sentences, items)):
        word_tokens[b, :len(s) + 2] = [synth.BOS_ID] + list(s) + [synth.EOS_ID]
        for t, e in enumerate(it):
            keys[b, t + 1, :e[0].shape[0]] = e[0]
            values[b, t + 1, :e[0].shape[0]] = e[4] if len(e) > 4 else e[0]
            key_map[b, t + 1, :e[1].shape[0]] = e[1]
            pinyin[b, t + 1, :e[2].shape[0]] = e[2]
            pinyin_map[b, t + 1, :e[3].shape[0]] = e[3]
    key_map[:, 0, :] = 1
    key_map[:, -1, :] = 1
    pinyin_map[:, 0, :] = 1
    pinyin_map[:, -1, :] = 1
    for (b, t), v in (pron or {}).items():
        pron_modified[b, t] = v
    for b, n in enumerate(valid or []):
        word_tokens[b, n:] = 0
    return {"word_tokens": word_tokens, "keys": keys, "values": values, "key_map": key_map, "pinyin": pinyin, "pinyin_map": pinyin_map,
            "pron_modified": pron_modified}


def id_batch(entries, sentences, pron=None, valid=None, tab=None):
    """the id form of collate(): synth.make_id_batch on the table (entry -1 / -2 are its), pron / valid as in collate"""
    ib = synth.make_id_batch(sentences, tab if tab is not None else table(entries), pron_every=0)
    for (b, t), v in (pron or {}).items():
        ib["pron_modified"][b, t] = v
    for b, n in enumerate(valid or []):
        ib["word_tokens"][b, n:] = 0
    return ib


def for_reference(batch):
    """the batch as the reference can take it: the kernel reads a pinyin id outside [0, n_pinyin) as 0 (the padding row of the embedding,
    all zero); nn.Embedding raises there"""
    py = batch["pinyin"]
    if ((py < 0) | (py >= synth.N_PINYIN)).any():
        batch = dict(batch)
        batch["pinyin"] = np.where((py < 0) | (py >= synth.N_PINYIN), 0, py)
    return batch


# ------------------------------------------------------------------------------------------------------------- the case table
class Case:
    """name: the branch the case forces; entries (a list, or a callable that builds it on first use: collecting the tests draws no
    gloss array) / sentences / pron / valid: see collate; hp: 'default' or an acoustic_ref.CONFIGS key"""

    def __init__(self, name, entries, sentences=None, pron=None, valid=None, hp="default"):
        self.name, self._entries, self._sentences, self.pron, self.valid, self.hp = name, entries, sentences, pron, valid, hp

    @property
    def entries(self):
        if callable(self._entries):
            self._entries = self._entries()
        return self._entries

    @property
    def sentences(self):
        return self._sentences if self._sentences is not None else [[3 + i for i in range(len(self.entries))]]

    def batch(self):
        return collate(self.entries, self.sentences, self.pron, self.valid)

    def ids(self, tab=None):
        return id_batch(self.entries, self.sentences, self.pron, self.valid, tab)

    def frames(self, per_word=2):
        wt = self.batch()["word_tokens"]
        return [per_word * max(1, int((r > 0).sum())) for r in wt]


def rows_entries(rows, scale, tag, values_scale=None):
    return [entry(f"{tag}.rows{n}", np.ones(n), scale=scale, values_scale=values_scale) for n in rows]


def pattern_entries(L, scale, tag, values_scale=None):
    out = []
    for kind in PATTERNS:
        km, z = pattern(kind, L)
        out.append(entry(f"{tag}.{kind}{L}", km, scale=scale, zero_rows=z, values_scale=values_scale))
    return out


def sense_entries(scale):
    """senses and pinyin slots: 1, 2 and 15 senses (P = 2, 4, 30), P not a multiple of 4, a sense of key_map that pinyin_map lacks and the
    reverse, pinyin ids outside [0, n_pinyin)"""
    e = [entry("sense.s1", natural([9]), scale=scale),
         entry("sense.s2", natural([7, 12]), scale=scale),
         entry("sense.s15", natural([3 + (i % 4) for i in range(15)]), scale=scale),
         entry("sense.p3", natural([6, 6]), pinyin_map=[1, 2, 2], scale=scale),
         entry("sense.p5", natural([5, 5, 5]), pinyin_map=[1, 1, 2, 3, 3], scale=scale),
         entry("sense.km_only", natural([6, 6, 6]), pinyin_map=[1, 1, 3, 3], scale=scale),            # sense 2 has rows but no slot
         entry("sense.pm_only", natural([6, 6]), pinyin_map=[1, 1, 2, 2, 4, 4], scale=scale),         # sense 4 has slots but no row
         entry("sense.bad_pinyin", natural([6, 6]), pinyin=[-3, 5, synth.N_PINYIN, 1 << 40], scale=scale)]
    return e


def p_entries(P, scale):
    """a hand-built entry with P pinyin slots over 15 senses of 4 rows (+ a plain two-sense entry beside it)"""
    return [entry(f"sense.P{P}", natural([4] * 15), pinyin_map=[1 + p % 15 for p in range(P)], scale=scale),
            entry(f"sense.P{P}.plain", natural([5, 6]), scale=scale)]


def cases():
    """every case, by name.  The row-count and pattern families come at both scales (suffix .flat / .peaked); .vfull: flat keys with
    separate full-scale values (a dropped value row shows in context)."""
    later = lambda f, *a: (lambda: f(*a))
    out = []
    for tag, sc in (("flat", FLAT), ("peaked", PEAKED)):
        out.append(Case(f"rows_1-17.{tag}", later(rows_entries, ROWS[:8], sc, tag)))
        out.append(Case(f"rows_31-65.{tag}", later(rows_entries, ROWS[8:14], sc, tag)))
        # (also the mixed batch: a 1-row and a 257-row entry in one batch, L_k = 257 the batch maximum, Lrow < L_k)
        out.append(Case(f"rows_148-257_mixed_with_1.{tag}", later(rows_entries, ROWS[14:] + (1,), sc, tag), [[3, 4, 5], [7, 6]]))
        out.append(Case(f"rows_lmax_{LMAX}.{tag}", later(rows_entries, (LMAX,), sc, tag)))
        for L in (17, 66, 258):
            out.append(Case(f"patterns_{L}.{tag}", later(pattern_entries, L, sc, tag)))
        out.append(Case(f"senses.{tag}", later(sense_entries, sc)))
    out.append(Case("rows_1-17.vfull", later(rows_entries, ROWS[:8], FLAT, "vfull", PEAKED)))
    out.append(Case("rows_31-65.vfull", later(rows_entries, ROWS[8:14], FLAT, "vfull", PEAKED)))
    out.append(Case("rows_148-257_mixed_with_1.vfull", later(rows_entries, ROWS[14:] + (1,), FLAT, "vfull", PEAKED), [[3, 4, 5], [7, 6]]))
    for L in (17, 66, 258):
        out.append(Case(f"patterns_{L}.vfull", later(pattern_entries, L, FLAT, "vfull", PEAKED)))
    out.append(Case("slots_P64", later(p_entries, 64, FLAT)))
    out.append(Case("slots_P63", later(p_entries, 63, FLAT)))
    # pron_modified.  Utterance 0: s2 s15 s1 p5, utterance 1: s2 s1 (batch maximum of pinyin_map: 15)
    out.append(Case("pron_forced", later(sense_entries, FLAT), [[4, 5, 3, 7], [4, 3]],
                    pron={(0, 1): 2,                 # an existing sense
                          (0, 2): MAX_SENSES,        # the batch maximum
                          (0, 3): 1,
                          (0, 4): MAX_SENSES + 1,    # one above the batch maximum: must not fire
                          (1, 1): 1,
                          (1, 2): 9}))               # a sense of ANOTHER utterance's entry; this word's own entry has one sense
    # dead words: utterance 0 keeps 2 valid words of 6 (BOS and the 5-row entry); the 257-row and the 65-row live entries, the forced
    # two-sense entry and the last padded row lie past its end.  Utterance 1 is shorter (3 valid words; then entry -2, and the batch's
    # last padded row: entry -1 / the collated all-ones row, dead)
    de = lambda: rows_entries((5, 257, 65, 17), FLAT, "dead") + [entry("dead.s2", natural([7, 12]), scale=FLAT)]
    out.append(Case("dead_words", de, [[3, 4, 5, 7], [6]], pron={(0, 4): 2}, valid=[2, 3]))
    # widths: the same rows at the other instantiations
    for hp in ("h128_heads2-mha_dk64-s2pa_d128-conv_cout128", "h256_heads4-mha_dk64-s2pa_1x4-post_cond_f32",
               "h384_heads4-mfma_c384-s2pa_table_d384"):
        short = hp.split("_")[0]
        out.append(Case(f"width_{short}.rows.flat", later(rows_entries, (1, 5, 17, 65, 257), FLAT, "w"), hp=hp))
        out.append(Case(f"width_{short}.patterns_66.flat", later(pattern_entries, 66, FLAT, "w"), hp=hp))
        out.append(Case(f"width_{short}.rows.peaked", later(rows_entries, (1, 5, 17, 65, 257), PEAKED, "wp"), hp=hp))
    return {c.name: c for c in out}


def order_cases(base_logits):
    """row order: the 66- and 258-row entries of case 'order_base' with their rows ordered by ascending (a new running maximum at every
    step of every stream) and by descending reference logit (none).  base_logits: {word index: [L] float64 logits of the base case}"""
    base = order_base()
    out = {}
    for tag, sign in (("ascending", 1), ("descending", -1)):
        ent = []
        for i, e in enumerate(base.entries):
            o = np.argsort(sign * np.asarray(base_logits[i]), kind="stable")
            ent.append((e[0][o], e[1], e[2], e[3]))   # (all rows live: key_map is unchanged by the permutation)
        out[f"order_{tag}"] = Case(f"order_{tag}", ent)
    return out


def order_base():
    return Case("order_base", lambda: rows_entries((66, 258), FLAT, "order"))


ORDER_NAMES = ("order_ascending", "order_descending")


# ------------------------------------------------------------------------------------------------------------- float64 restatement
DEFECTS = ("drop_last_row_mod16_1", "merge_without_rescale", "clamped_row_live", "alias_second_chunk_skipped", "fill_stops_at_nthr",
           "sense_ignores_rows_256", "pinyin_drops_tail", "dead_reads_values")


def _fold(m, acc, lg, v):
    mn = max(m, lg)
    return mn, acc * np.exp(m - mn) + v * np.exp(lg - mn)


def _merge(ma, a, mb, b, rescale=True):
    mn = max(ma, mb)
    return mn, a * np.exp(ma - mn) + b * (np.exp(mb - mn) if rescale else 1.0)


def kernel_word(form, lg_rows, km_rows, v_rows, pm, mod, pm_max, L_k, dead=False, special=0, defect=None):
    """one word through the kernel's partition, in float64.  form: 'table' | 'tensor' | 'alias'; lg_rows [Lrow]: the rows' logits k . q;
    km_rows [Lrow]; v_rows [Lrow, H]: projected value rows; pm [P]: pinyin_map row; special: -1 / -2 (table entry ids; Lrow = 0).
    -> weights [L_k], wv [H] (the weighted value sum before output_transform), pw [P], slots (how many of pw the pinyin mix uses)"""
    Lrow, H = len(lg_rows), v_rows.shape[1]
    km_g = np.concatenate([km_rows, np.full(L_k - Lrow, 1.0 if special == -1 else 0.0)])
    # fill (strided by NTHR)
    km = np.zeros(L_k)
    fill_to = min(L_k, NTHR) if defect == "fill_stops_at_nthr" else L_k
    km[:fill_to] = km_g[:fill_to]
    lg = np.where(km == 0, -1e9, 0.0)
    parts = []          # (m, acc) per wave
    n = 0
    if form == "table":
        streams = table_loop(Lrow)
        if defect == "drop_last_row_mod16_1" and Lrow % 16 == 1:
            for k in streams:
                streams[k] = [l for l in streams[k] if l != Lrow - 1]
        for w in range(NW):
            grp = []
            for g in range(4):
                m, acc = -3.0e38, np.zeros(H)
                rows = list(streams[(w, g)])
                for l in rows:
                    if km_rows[l] != 0:
                        lg[l] = lg_rows[l]
                        n += 1
                        if not dead:
                            m, acc = _fold(m, acc, lg_rows[l], v_rows[l])
                grp.append((m, acc))
            if defect == "clamped_row_live" and Lrow % 4 and (((Lrow - 1) // 4) % NW) == w:
                # the last step of this wave holds slots past the entry: they read row 0 (`in ? l : 0`) and count as live
                for g in range(Lrow % 4, 4):
                    l = (Lrow - 1) // 4 * 4 + g
                    if l < L_k:
                        lg[l] = lg_rows[0]
                    n += 1
                    if not dead:
                        grp[g] = _fold(*grp[g], lg_rows[0], v_rows[0])
            r = defect != "merge_without_rescale"
            a01 = _merge(*grp[0], *grp[1], rescale=r)
            a23 = _merge(*grp[2], *grp[3], rescale=r)
            parts.append(_merge(*a01, *a23, rescale=r))
    else:
        live = [l for base, rows in ballot_bases(Lrow) for l in rows if km[l] != 0]
        n = len(live)
        rv = RU // 2
        chunks = list_loop(n, rv, form == "alias")
        if form == "alias" and defect == "alias_second_chunk_skipped":
            first = list_loop(n, rv, False)
            chunks = {w: [c for c in first[w] if (c[0] // rv // NW) % 2 == 0] for w in range(NW)}
        for w in range(NW):
            m, acc = -3.0e38, np.zeros(H)
            for ch in chunks[w]:
                rows = [live[i] for i in ch]
                if defect == "clamped_row_live" and len(ch) < rv:
                    rows += [live[n - 1]] * (rv - len(ch))           # min(i + j, n - 1) read again and folded
                for l in rows:
                    lg[l] = lg_rows[l]
                    if not dead:
                        m, acc = _fold(m, acc, lg_rows[l], v_rows[l])
            parts.append((m, acc))
    mx = lg.max()
    e = np.exp(lg - mx)
    sm = e.sum()
    wts = e / sm
    if n > 0 or dead:
        wv = sum(acc * np.exp(m - mx) / sm for m, acc in parts)
        if dead and defect != "dead_reads_values":
            wv = np.zeros(H)
        elif dead:   # the value rows read and folded as for a live word, and the sum not zeroed
            _, wv, _, _ = kernel_word(form, lg_rows, km_rows, v_rows, pm, mod, pm_max, L_k, False, special, None)
    else:
        wv = np.zeros(H)
        for w, rows in nolive_loop(Lrow).items():
            for l in rows:
                wv = wv + wts[l] * v_rows[l]
    # tail
    sense = np.zeros(16)
    lim = min(L_k, 256) if defect == "sense_ignores_rows_256" else L_k
    for i in range(1, 16):
        sense[i] = wts[:lim][km[:lim] == i].sum()
    pmv = np.asarray(pm)
    pw = np.array([sense[int(p)] if 1 <= p < 16 else 0.0 for p in pmv])
    if 1 <= mod <= pm_max:
        pw = (pmv == mod).astype(np.float64)
    P = len(pmv)
    return wts, wv, pw, (P - P % 4 if defect == "pinyin_drops_tail" else P)


def s2pa_inputs(sd, hp, batch):
    """float64 pieces of the reference's dictionary encoder up to S2PA: q (scaled), projected keys / values, x_mask"""
    sh = synth.acoustic_shape(hp)
    p = "dict_encoder.S2PA_module"
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    wt = t["word_tokens"]
    with torch.no_grad():
        lens = (wt > 0).long().sum(-1)
        x = F.embedding(wt, sd[p + ".word_emb.weight"]) * np.sqrt(sh["hidden_size"])
        x = x.transpose(1, -1)
        x_mask = (torch.arange(x.size(2)).unsqueeze(0) < lens.unsqueeze(1)).unsqueeze(1).to(x.dtype)
        x = ref.rel_encoder(sd, p + ".semantic_encoder", x, x_mask, 4, sh["num_heads"], sh["enc_ffn_kernel_size"])
        a = p + ".s2pa_attention"
        q = F.linear(x.transpose(1, 2), sd[a + ".q_transform.weight"]) * GD ** -0.5
        k = F.linear(t["keys"].double(), sd[a + ".k_transform.weight"])
        v = F.linear(t["values"].double(), sd[a + ".v_transform.weight"])
        logits = torch.matmul(k, q.unsqueeze(-1)).squeeze(-1)
    return {"q": q, "k": k, "v": v, "logits": logits, "x_mask": x_mask, "lens": lens}


def restated(sd, hp, case, form, defect=None, pre=None):
    """the dictionary encoder with S2PA replaced by kernel_word per word (float64) -> dict_attn [B,1,L_k,T_w], pron_attn, context,
    word_encoder_out, wv (before output_transform and the mask).  pre: s2pa_inputs of the case's batch (reused between defects)"""
    sh = synth.acoustic_shape(hp)
    batch = for_reference(case.batch())
    ib = case.ids()
    pre = pre or s2pa_inputs(sd, hp, batch)
    B, T_w, L_k = batch["key_map"].shape
    P = batch["pinyin"].shape[2]
    H = sh["hidden_size"]
    lg, v = pre["logits"].numpy(), pre["v"].numpy()
    pm_max = int(batch["pinyin_map"].max())
    wts, wv, pw = np.zeros((B, T_w, L_k)), np.zeros((B, T_w, H)), np.zeros((B, T_w, P))
    slots = P
    for b in range(B):
        for t in range(T_w):
            dead = t >= int(pre["lens"][b])
            e = int(ib["entry_ids"][b, t])
            if form == "table":
                Lrow = len(case.entries[e][1]) if e >= 0 else 0
                r = kernel_word(form, lg[b, t, :Lrow], batch["key_map"][b, t, :Lrow].astype(np.float64), v[b, t, :Lrow],
                                batch["pinyin_map"][b, t], int(batch["pron_modified"][b, t]), pm_max, L_k, dead, min(e, 0), defect)
            else:
                r = kernel_word(form, lg[b, t], batch["key_map"][b, t].astype(np.float64), v[b, t], batch["pinyin_map"][b, t],
                                int(batch["pron_modified"][b, t]), pm_max, L_k, dead, 0, defect)
            wts[b, t], wv[b, t], pw[b, t], slots = r
    p = "dict_encoder.S2PA_module"
    a = p + ".s2pa_attention"
    with torch.no_grad():
        ctx = F.linear(torch.from_numpy(wv), sd[a + ".output_transform.weight"]).transpose(1, 2) * pre["x_mask"]
        pin = F.embedding(torch.from_numpy(batch["pinyin"]), sd[a + ".pinyin_embedding.weight"])
        res = torch.from_numpy(pw)
        pron = torch.matmul(res[..., :slots].unsqueeze(-2), pin[:, :, :slots]).squeeze(-2).transpose(1, 2)
        x = ref.rel_encoder(sd, p + ".linguistic_encoder", ctx + pron, pre["x_mask"], 4, sh["num_heads"], sh["enc_ffn_kernel_size"])
        weo = x.transpose(1, 2) * torch.from_numpy(batch["word_tokens"] > 0).double()[:, :, None]
    return {"dict_attn": torch.from_numpy(wts).unsqueeze(1).permute(0, 1, 3, 2), "pron_attn": res, "context": ctx.transpose(1, 2),
            "word_encoder_out": weo, "wv": torch.from_numpy(wv)}
