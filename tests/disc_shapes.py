"""The shape cases of the discriminator tests (tests/test_disc_cpu.py, tests/test_disc_gpu.py) and of the fixture generator
(tools/make_golden_disc.py).  Lengths are in samples; the longest is 4099, so a case takes about a second on either side.

Where the lengths come from (rows: ceil division through the strides):
  * 6 = DISC_MIN_LEN: period 11 pads 5 samples by reflection, which needs 6; the third scale then sees 1 sample.
  * 12, 13: the third scale sees 3 samples, every k = 41 window is mostly padding; 13 pads for every period but 13 % p == 0 never holds.
  * 2309 / 2310 / 2311: 2310 = 2 * 3 * 5 * 7 * 11 needs no reflect padding for any period; one sample less pads 1, one more pads p - 1.
  * 576 / 577: at period 2 the rows after the second dense layer are 32 / 33: the dense kernels' 32-row tile (DISC_DENSE_TILE), stride 3.
  * 256 / 257 and 2048 / 2049: the grouped kernel's 128-row tile (DISC_GROUP_TILE) after the stride-2 layer 1 (rows = ceil(L / 2)) and
    after the stride-4 layer 3 (rows = ceil(L / 16)); 4099 gives 65 rows after layer 4: its 64-row tile (DISC_GROUP_TILE_WIDE) at stride 4.
"""
import zlib

import numpy as np

SEED = 1616
PERIODS = (2, 3, 5, 7, 11)

CASES = [
    {"name": "min", "lens": [6]},
    {"name": "L12_13", "lens": [12, 13]},
    {"name": "primorial", "lens": [2309, 2310, 2311]},
    {"name": "dense_tile", "lens": [576, 577]},
    {"name": "group_tile", "lens": [256, 257, 2048, 2049]},
    {"name": "L4099", "lens": [4099]},
    {"name": "mixed", "lens": [6, 4099, 13]},
    {"name": "same", "lens": [777], "kind": "same"},
    {"name": "zeros", "lens": [500], "kind": "zeros"},
]
CASE_BY_NAME = {c["name"]: c for c in CASES}


def _rng(name):
    return np.random.Generator(np.random.Philox(key=[SEED, zlib.crc32(name.encode())]))


def utterance(case, b):
    """(y, y_hat) float32 of utterance b of a case, at its own length.  The utterance depends on (case name, b) only."""
    L = case["lens"][b]
    kind = case.get("kind", "noise")
    if kind == "zeros":
        return np.zeros(L, np.float32), np.zeros(L, np.float32)
    r = _rng(f"{case['name']}.{b}")
    t = np.arange(L)
    y = (0.25 * np.sin(2 * np.pi * t * (0.01 + 0.003 * b)) + 0.15 * r.standard_normal(L)).astype(np.float32)
    if kind == "same":
        return y, y.copy()
    return y, (y + 0.08 * r.standard_normal(L).astype(np.float32)).astype(np.float32)


def batch(case, pad=0):
    """the case as a padded batch: y, y_hat [B, T] float32 with T = max(lens) + pad, NaN behind every utterance's own length (nothing of the
    padding may enter a result), lens int32 [B]"""
    lens = np.asarray(case["lens"], np.int32)
    T = int(lens.max()) + pad
    y = np.full((len(lens), T), np.nan, np.float32)
    yh = np.full((len(lens), T), np.nan, np.float32)
    for b, L in enumerate(lens):
        y[b, :L], yh[b, :L] = utterance(case, b)
    return y, yh, lens


def rows_after(L, strides):
    for s in strides:
        L = -(-L // s)
    return L


def d_count(d, L):
    """outputs of discriminator d (0 .. 4 the periods, 5 .. 7 the scales) for L samples"""
    if d < 5:
        p = PERIODS[d]
        return rows_after(-(-L // p), (3, 3, 3, 3)) * p
    for _ in range(d - 5):
        L = L // 2
    return rows_after(L, (2, 2, 4, 4))
