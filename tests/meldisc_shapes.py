"""The shape cases of the mel-discriminator tests (tests/test_meldisc_cpu.py, tests/test_meldisc_gpu.py) and of the fixture generator
(tools/make_golden_meldisc.py).  Lengths are in frames; the longest is 200, so a case takes well under a second on either side.

Where the lengths come from.  A window of win frames gives maps of (win / 2, 40), (win / 4, 20), (win / 8, 10): 16 x 40 ... 64 x 40 after
block 1, 8 x 20 ... 32 x 20 after block 2, 4 x 10 ... 16 x 10 after block 3.  The implicit GEMM's tile is 32 output positions as 8 x 4
(block 2, and block 3 of the 64-frame window: 10 columns = 4 + 4 + 2, a ragged last tile), 4 x 8 (block 3 of the 32-frame window: 8 + 2) or
16 x 2 (block 3 of the 128-frame window), so the three windows cover every tile shape, several tiles per clip in both axes and all four
zero-padded borders.  win - 1 / win / win + 1 frames: no clip, one clip, two clips at hop 1 (the second ends on the last frame).
"""
import zlib

import numpy as np

SEED = 1717
WINS = (32, 64, 128)
N_MEL = 80

CASES = [
    {"name": "short", "lens": [31], "hop": 1},
    {"name": "w32_edge", "lens": [32, 33], "hop": 1},
    {"name": "w64_edge", "lens": [63, 64, 65], "hop": 1},
    {"name": "w128_edge", "lens": [127, 128, 129], "hop": 1},
    {"name": "multi", "lens": [200], "hop": 16, "extra": True},     # hop 16 plus the starts len - win and an odd one (37)
    {"name": "mixed", "lens": [32, 200, 129]},                      # default hop: win / 2
    {"name": "same", "lens": [90], "kind": "same"},
    {"name": "zeros", "lens": [70], "kind": "zeros"},
]
CASE_BY_NAME = {c["name"]: c for c in CASES}
ALL = [c["name"] for c in CASES]

# (norm, hidden, reduction, win_num, cases)
RUNS = [
    ("in", 128, "stack", 3, ALL),
    ("bn", 128, "stack", 3, ["multi", "mixed"]),
    ("sn", 128, "stack", 3, ["multi", "mixed"]),
    ("in", 128, "sum", 3, ["multi", "mixed"]),
    ("in", 128, "none", 3, ["multi", "mixed"]),
    ("in", 64, "stack", 3, ["multi", "mixed"]),
    ("in", 128, "stack", 1, ["multi", "mixed"]),
    ("in", 96, "stack", 3, ["mixed"]),      # three co-tiles: the fourth wave of a workgroup idles; two statistics groups of 96 threads
    ("in", 256, "stack", 3, ["mixed"]),     # two workgroups of four co-tiles per tile; eight 32-channel chunks
]
RUN_CASES = [(r, name) for r in RUNS for name in r[4]]
# the clip whose hidden maps the fixture holds (the 32-frame window only), and the channels it keeps of them
HIDDEN_CASE, HIDDEN_B, HIDDEN_START, HIDDEN_CH = "multi", 0, 37, slice(0, None, 16)
# forward(): zero-padded batches with given starts, one start per window shared by the batch
FORWARD = [
    {"name": "fw_mixed", "case": "mixed", "starts": [5, 40, 72]},    # clips run behind the 32- and 129-frame utterances' own lengths
    {"name": "fw_edge", "case": "w128_edge", "starts": [97, 65, 1]},
    {"name": "fw_none", "case": "w64_edge", "starts": [0, 0, 0]},    # the 128-frame window does not fit: y is None
]


def run_id(run):
    return f"{run[0]}_{run[1]}_{run[2]}_{run[3]}"


def _rng(name):
    return np.random.Generator(np.random.Philox(key=[SEED, zlib.crc32(name.encode())]))


def utterance(case, b):
    """(mel_g, mel_p) float32 [len, 80] of utterance b of a case: log10-scale values around -2 +- 1, smoothed along time; the generated
    mel is the recording plus noise.  Depends on (case name, b) only."""
    L = case["lens"][b]
    kind = case.get("kind", "noise")
    if kind == "zeros":
        return np.zeros((L, N_MEL), np.float32), np.zeros((L, N_MEL), np.float32)
    r = _rng(f"{case['name']}.{b}")
    g = r.standard_normal((L, N_MEL))
    g[1:] = 0.7 * g[1:] + 0.3 * g[:-1]
    g = (-2.0 + g).astype(np.float32)
    if kind == "same":
        return g, g.copy()
    return g, (g + 0.3 * r.standard_normal((L, N_MEL)).astype(np.float32)).astype(np.float32)


def batch(case, pad=0, fill=np.nan):
    """the case as a padded batch: mel_g, mel_p [B, T, 80] float32 with T = max(lens) + pad and `fill` behind every utterance's own length
    (NaN for scores: nothing of the padding may enter a result; 0 for forward), lens int32 [B]"""
    lens = np.asarray(case["lens"], np.int32)
    T = int(lens.max()) + pad
    g = np.full((len(lens), T, N_MEL), fill, np.float32)
    p = np.full((len(lens), T, N_MEL), fill, np.float32)
    for b, L in enumerate(lens):
        g[b, :L], p[b, :L] = utterance(case, b)
    return g, p, lens


def case_starts(case, win):
    """None (the hop rule, default hop win / 2 or the case's hop) or, for a case with ``extra``, the explicit starts of window `win`"""
    if not case.get("extra"):
        return None
    L = max(case["lens"])
    return list(range(0, L - win + 1, case["hop"])) + [L - win, 37]


def starts_of(case, b, win):
    """the starts of utterance b's clips of window `win`, by either rule"""
    L = case["lens"][b]
    ex = case_starts(case, win)
    if ex is not None:
        return [s for s in ex if s + win <= L]
    hop = case.get("hop", win // 2)
    return list(range(0, L - win + 1, hop))
