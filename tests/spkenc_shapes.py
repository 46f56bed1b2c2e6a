"""The shape cases of the speaker-encoder tests (tests/test_spkenc_cpu.py, tests/test_spkenc_gpu.py).  Lengths are in samples at 16 kHz,
rate 1.3 (77 frames between partials) and min_coverage 0.75.

Where the lengths come from:
  * 1, 200: shorter than a frame / than the window; one partial, all of it zero padding.
  * 25600: exactly one partial; a second one would cover (25600 - 12320) / 25600 = 0.519 of itself and is dropped.
  * 31519 / 31520: the second partial covers 0.74996 (dropped) / exactly 0.75 (kept).
  * P partials need L >= 12320 (P - 1) + 19200 (the last one at frame 77 (P - 1) covered to 0.75): M - 1, M, M + 1 partials for M = 32
    sequences per workgroup of the recurrent kernel, a full tile and one sequence into the next.  (M = 16: the mixed batch's 102 sequences
    cross its tile edges too.)
"""
import zlib

import numpy as np

SEED = 2020
M = 32                      # abi.SPKENC_TILE_M
HOP, PART, FRAME_STEP = 160, 160, 77


def len_for_partials(P):
    """the shortest utterance of P >= 2 partials"""
    return HOP * FRAME_STEP * (P - 1) + (3 * PART * HOP) // 4


UTTERANCES = {"L1": 1, "L200": 200, "L25600": 25600, "L31519": 31519, "L31520": 31520,
              "Pm1": len_for_partials(M - 1), "Pm": len_for_partials(M), "Pp1": len_for_partials(M + 1)}
PARTIALS = {"L1": 1, "L200": 1, "L25600": 1, "L31519": 1, "L31520": 2, "Pm1": M - 1, "Pm": M, "Pp1": M + 1}
SHORT = ("L1", "L200", "L25600", "L31519", "L31520")
MIXED = ("L31520", "L1", "Pm", "L200", "Pp1", "L25600", "Pm1", "L31519")
FORWARD_CASES = [(N, T) for N in (1, M, M + 1) for T in (1, 2, 3, 160)]


def _rng(name):
    return np.random.Generator(np.random.Philox(key=[SEED, zlib.crc32(name.encode())]))


def wav(name):
    """the float32 waveform of an utterance, a function of its name only: two drifting tones and noise under a slow envelope"""
    L = UTTERANCES[name]
    r = _rng("wav." + name)
    t = np.arange(L, dtype=np.float64)
    f0 = 110.0 + 60.0 * r.random()
    env = 0.6 + 0.4 * np.sin(2 * np.pi * t / 16000.0 * (0.7 + r.random()))
    x = env * (0.2 * np.sin(2 * np.pi * f0 * t / 16000.0) + 0.08 * np.sin(2 * np.pi * 7.3 * f0 * t / 16000.0)) + 0.05 * r.standard_normal(L)
    return x.astype(np.float32)


def batch(names, pad=37, fill=np.nan):
    """(wavs float32 [B, max L + pad], lens int32 [B]): what lies behind each utterance is `fill` (NaN: a read past lens would show)"""
    lens = np.array([UTTERANCES[n] for n in names], np.int32)
    out = np.full((len(names), int(lens.max()) + pad), fill, np.float32)
    for b, n in enumerate(names):
        out[b, :lens[b]] = wav(n)
    return out, lens


def mels(N, T, scale=0.05, name="mels"):
    """power-mel-like inputs float32 [N, T, 40]: non-negative, of the size a recording at -20 dBFS gives"""
    r = _rng(f"{name}.{N}.{T}")
    return (scale * r.standard_normal((N, T, 40)) ** 2).astype(np.float32)
