"""The case list of the validation-loss tests (test infrastructure): seeded inputs for dtts_text2mel_fetch(DTTS_OUT_LOSSES), shared by
tools/make_golden_losses.py (which feeds them to the reference), tests/test_losses_cpu.py and tests/test_losses_gpu.py.

Mel cases derive from R = abi.LOSS_TILE_ROWS: T in {1, 5, 6, 10, 11} (shorter than, equal to and just past the 11-tap window and its
half), {R - 1, R, R + 1} (the tile seam), 2 R + 3 (three tiles), n_mel in {1, 11, 20, 128} at T = R + 1, and the special cases: leading
dimensions beyond T with poisoned rows, an all-zero target row in mid-utterance, an utterance whose target is entirely zero, a zero row
exactly on a tile seam.  Every batch has three utterances: one that fills T, one that ends early (zero target rows behind it, non-zero
predictions there, as a decoder leaves them) and one more that fills T or carries the special rows.  Predictions lie 0.1 .. 0.3 from the
targets, where the reference's float32 SSIM is itself accurate to about 5e-4 relative.

Duration cases: T_w in {1, 7, 64, 300}, both dur_scale values; each batch has a word with no frame, an utterance with word_len < T_w
(whose mel2word still names words beyond word_len), zeros inside mel2word and a trailing pad.
"""
import zlib

import numpy as np

from dict_tts_amd import abi

SEED = 20240613
R = abi.LOSS_TILE_ROWS
BIAS = 6.0


def _rng(name):
    return np.random.Generator(np.random.Philox(key=[SEED, zlib.crc32(name.encode())]))


def _mel_case(name, T, n_mel=80, pad_ld=(0, 0), zero_rows=(), all_zero=None):
    return {"name": name, "T": T, "n_mel": n_mel, "pad_ld": pad_ld, "zero_rows": tuple(zero_rows), "all_zero": all_zero}


MEL_CASES = [_mel_case(f"T{T}", T) for T in (1, 5, 6, 10, 11, R - 1, R, R + 1, 2 * R + 3)]
MEL_CASES += [_mel_case(f"T{R + 1}_m{m}", R + 1, n_mel=m) for m in (1, 11, 20, 128)]
MEL_CASES += [
    _mel_case("ld_poisoned", R + 1, pad_ld=(3, 5)),                          # pred_ld = T + 3, tgt_ld = T + 5, NaN rows beyond T
    _mel_case("zero_row_mid", R + 1, zero_rows=((2, 7),)),                   # utterance 2, frame 7: weight 0 inside the utterance
    _mel_case("all_zero_utt", 11, all_zero=1),                               # utterance 1: count 0, sums 0; the batch figure stays finite
    _mel_case("zero_row_seam", 2 * R + 3, zero_rows=((2, R - 1), (2, R), (0, 2 * R))),   # the last row of tile 0, the first of tiles 1 and 2
]
MEL_BY_NAME = {c["name"]: c for c in MEL_CASES}
B_MEL = 3


def mel_inputs(case):
    """-> pred [B, T + pad_ld[0], n_mel], tgt [B, T + pad_ld[1], n_mel] float32 (rows >= T are NaN), lens [B]"""
    T, M, name = case["T"], case["n_mel"], case["name"]
    rng = _rng("mel." + name)
    lens = [T, max(1, (2 * T) // 3), T]
    tgt = np.zeros((B_MEL, T, M), np.float32)
    pred = np.zeros((B_MEL, T, M), np.float32)
    for b in range(B_MEL):
        m = (rng.standard_normal((T, M)) * 1.2 - 3.0).astype(np.float32)
        m[1:] = 0.6 * m[1:] + 0.4 * m[:-1]
        tgt[b, :lens[b]] = np.clip(m, -5.9, 1.5)[:lens[b]]
        off = rng.uniform(0.1, 0.3, (T, M)) * rng.choice([-1.0, 1.0], (T, M))
        pred[b] = (tgt[b] + off).astype(np.float32)       # behind the utterance's end: +-0.1 .. 0.3 around zero, not zero
    for b, t in case["zero_rows"]:
        tgt[b, t] = 0.0
    if case["all_zero"] is not None:
        tgt[case["all_zero"]] = 0.0
        lens[case["all_zero"]] = 0
    pp, tp = case["pad_ld"]
    if pp:
        pred = np.concatenate([pred, np.full((B_MEL, pp, M), np.nan, np.float32)], 1)
    if tp:
        tgt = np.concatenate([tgt, np.full((B_MEL, tp, M), np.nan, np.float32)], 1)
    return np.ascontiguousarray(pred), np.ascontiguousarray(tgt), np.array(lens, np.int64)


DUR_CASES = [{"name": f"Tw{tw}_{scale}", "T_w": tw, "scale": scale} for tw in (1, 7, 64, 300) for scale in ("log", "linear")]
DUR_BY_NAME = {c["name"]: c for c in DUR_CASES}
B_DUR = 3


def dur_inputs(case):
    """-> dur_pred [B, T_w] float32, mel2word [B, T_mel] int64, word_len [B] int64 (max = T_w, as the reference's T = word_len.max())"""
    T_w, name = case["T_w"], case["name"]
    rng = _rng("dur." + name)
    word_len = np.array([T_w, max(1, T_w - 2), max(1, (2 * T_w) // 3)], np.int64)
    rows, durs = [], np.zeros((B_DUR, T_w), np.int64)
    for b in range(B_DUR):
        d = rng.integers(1, 7, T_w)
        if T_w > 2:
            d[int(rng.integers(1, T_w - 1))] = 0               # a word with no frame
        if b == 2:
            d[word_len[b]:] = 0                                # utterance 2 ends at word_len; utterance 1 names words beyond word_len
        if b == 0 and T_w == 1:
            d[0] = 3
        row = np.repeat(np.arange(1, T_w + 1), d)
        if row.size > 4:
            row[[2, row.size // 2]] = 0                        # zeros inside the utterance
        rows.append(row)
        durs[b] = np.bincount(row, minlength=T_w + 1)[1:]
    T_mel = max(r.size for r in rows) + 3                      # a trailing pad on every row
    m2w = np.zeros((B_DUR, T_mel), np.int64)
    for b, r in enumerate(rows):
        m2w[b, :r.size] = r
    noise = rng.uniform(-0.2, 0.2, (B_DUR, T_w))
    base = np.log(durs + 1.0) if case["scale"] == "log" else durs.astype(np.float64)
    return (base + noise).astype(np.float32), m2w, word_len


def fingerprint(*arrays):
    """float64 (sum, sum of squares) of every array with its NaNs taken as zero: G13 stores these instead of the regenerable inputs"""
    out = []
    for a in arrays:
        a = np.nan_to_num(np.asarray(a, np.float64), nan=0.0)
        out += [a.sum(), np.square(a).sum()]
    return np.array(out, np.float64)
