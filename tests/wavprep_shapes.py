"""The cases of the waveform-conditioning tests (tests/test_wavprep_cpu.py, tests/test_wavprep_gpu.py), with their float64 restatement
computed once and shared (``rs_ref`` / ``ld_ref``; nothing mutates what they return).  The lengths derive from the kernels' own
constants: abi.RESAMPLE_TILE outputs per workgroup, abi.LOUD_SEGMENT samples per segment of the recurrence.
"""
import functools

import numpy as np

import wavprep_ref as wr
from dict_tts_amd import abi
from dict_tts_amd import wavprep as W

TILE, SEG = abi.RESAMPLE_TILE, abi.LOUD_SEGMENT
RATIOS = [(48000, 22050), (44100, 22050), (16000, 22050), (22050, 16000), (24000, 22050), (8000, 48000), (48000, 8000)]


@functools.lru_cache(None)
def table(name):
    return {"kaiser_best": W.kaiser_best, "kaiser_fast": W.kaiser_fast}[name]()


def _noise(L, seed, amp=0.5):
    return (amp * np.random.RandomState(seed).randn(L)).astype(np.float32)


def _sine(L, sr, f=440.0, amp=0.7):
    return (amp * np.sin(2 * np.pi * f * np.arange(L) / sr)).astype(np.float32)


def _impulse(L, p):
    x = np.zeros(L, np.float32)
    x[p] = 1.0
    return x


# ---------------------------------------------------------------- resampler
def _rs(name, sr_in, sr_out, x, filt="kaiser_best"):
    return dict(name=name, sr_in=sr_in, sr_out=sr_out, x=np.ascontiguousarray(x, np.float32), L=len(x), filter=filt)


def _len_for_outputs(n, sr_in, sr_out):
    """the shortest L with int(L ratio) == n"""
    L = 1
    while W.resampled_len(L, sr_in, sr_out)[0] < n:
        L += 1
    return L


RS_CASES = []
for _i, (_a, _b) in enumerate(RATIOS):                                  # every ratio: noise over more than one tile of outputs, odd length
    _L = 3001 if (_a, _b) == (48000, 8000) else (131 if (_a, _b) == (8000, 48000) else 601)
    RS_CASES.append(_rs(f"noise_{_a}_{_b}", _a, _b, _noise(_L, 10 + _i)))
RS_CASES.append(_rs("fast_48000_22050", 48000, 22050, _noise(601, 30), "kaiser_fast"))
A, Bq = 48000, 22050                                                    # the lengths, at the ratio whose step is truncated (147 / 320)
for _L in (1, 2, 50):                                                   # shorter than one wing (139 input samples): both wings clipped
    RS_CASES.append(_rs(f"len_{_L}", A, Bq, _noise(_L, 40 + _L)))
for _L in (319, 320, 321, 640, 960, 961):                               # L ratio on an integer (320 k) and its neighbours
    RS_CASES.append(_rs(f"len_{_L}", A, Bq, _noise(_L, 40 + _L)))
for _n in (TILE - 1, TILE, TILE + 1, 3 * TILE + 5):                     # the workgroup's tile of outputs +- 1, and several tiles
    _L = _len_for_outputs(_n, A, Bq)
    RS_CASES.append(_rs(f"outputs_{_n}", A, Bq, _noise(_L, 60 + _n % 7)))
RS_CASES.append(_rs("sine", A, Bq, _sine(700, A)))
RS_CASES.append(_rs("dc", A, Bq, np.full(500, 0.25, np.float32)))
RS_CASES.append(_rs("impulse_0", A, Bq, _impulse(400, 0)))
RS_CASES.append(_rs("impulse_last", A, Bq, _impulse(400, 399)))
RS_CASES.append(_rs("impulse_0_up", 16000, 22050, _impulse(300, 0)))
RS_CASES.append(_rs("impulse_last_up", 16000, 22050, _impulse(300, 299)))
RS_BY_NAME = {c["name"]: c for c in RS_CASES}
RS_BATCH = [c["name"] for c in RS_CASES if (c["sr_in"], c["sr_out"], c["filter"]) == (A, Bq, "kaiser_best")]   # mixed lengths at one ratio


@functools.lru_cache(None)
def rs_ref(name, per_tap_f32=False):
    c = RS_BY_NAME[name]
    win, nt = table(c["filter"])
    return wr.resample(c["x"], c["sr_in"], c["sr_out"], win, nt, per_tap_f32=per_tap_f32)


def rs_batch_inputs(names, pad=13):
    """wav [B, max L + pad] with NaN behind every utterance's own length, lens [B]"""
    cs = [RS_BY_NAME[n] for n in names]
    wav = np.full((len(cs), max(c["L"] for c in cs) + pad), np.nan, np.float32)
    for b, c in enumerate(cs):
        wav[b, :c["L"]] = c["x"]
    return wav, np.array([c["L"] for c in cs], np.int32)


# ---------------------------------------------------------------- loudness
def _ld(name, rate, x, kind="ok"):
    return dict(name=name, rate=rate, x=np.ascontiguousarray(x, np.float32), L=len(x), kind=kind)


def _impulses(L, every, first, amp=0.9):
    x = np.zeros(L, np.float32)
    x[first::every] = amp
    return x


LD_CASES = [
    _ld("rate_22050", 22050, _noise(22050, 1, 0.1)),
    _ld("rate_16000", 16000, _noise(16000, 2, 0.1)),
    _ld("rate_48000", 48000, _noise(40000, 3, 0.1)),
    _ld("rate_44100", 44100, _noise(30000, 4, 0.1)),
    _ld("rate_11025", 11025, _noise(22051, 5, 0.1)),                   # 0.1 s is 1102.5 samples: the bounds' truncations alternate
    _ld("one_block", 16000, _noise(6400, 6, 0.2)),                     # exactly one block: 25 whole segments
    _ld("one_block_less", 16000, _noise(6399, 7, 0.2), "short"),       # status bit 0
    _ld("one_block_more", 16000, _noise(6401, 8, 0.2)),
    _ld("tie_7200", 16000, _noise(7200, 9, 0.2)),                      # (T - 0.4) / 0.1 = 0.5 -> 0: one block
    _ld("tie_8800", 16000, _noise(8800, 10, 0.2)),                     # 1.5 -> 2: three blocks
    _ld("cut_7360", 16000, _noise(7360, 11, 0.2)),                     # the last block [1600, 8000) is cut by the end
    _ld("seg_less", 22050, _noise(35 * SEG - 1, 12, 0.2)),             # the segment size +- 1 around 35 segments (8960 samples)
    _ld("seg_exact", 22050, _noise(35 * SEG, 13, 0.2)),
    _ld("seg_more", 22050, _noise(35 * SEG + 1, 14, 0.2)),
    _ld("level_0.5", 22050, _noise(12000, 15, 0.5)),
    _ld("level_0.05", 22050, _noise(12000, 16, 0.05)),
    _ld("level_0.001", 22050, _noise(12000, 17, 0.001)),
    _ld("loud_quiet", 16000, np.concatenate([_noise(24000, 18, 0.3), _noise(24000, 19, 0.3e-3)])),   # the relative gate drops the quiet half
    _ld("inaudible", 16000, _noise(16000, 20, 1e-5), "silent"),        # every block below -70: status bit 1
    _ld("zeros_first", 16000, np.concatenate([np.zeros(16000, np.float32), _noise(16000, 21, 0.2)])),   # blocks with z_j = 0 exactly
    _ld("all_zero", 16000, np.zeros(8000, np.float32), "silent"),
    _ld("dc", 22050, _noise(12000, 22, 0.1) + np.float32(0.1)),
    _ld("seam_impulse", 16000, _impulses(8000, 5 * SEG, 5 * SEG - 1)),  # an impulse one sample before a seam: the decaying state crosses it
    _ld("peaky", 16000, _impulses(16000, 2000, 100), "peak"),          # sparse impulses: the normalised peak exceeds 1, status bit 2
]
LD_BY_NAME = {c["name"]: c for c in LD_CASES}
LD_BATCH = [c["name"] for c in LD_CASES if c["rate"] == 16000 and c["L"] <= 16000]


@functools.lru_cache(None)
def ld_ref(name, f32_storage=False):
    c = LD_BY_NAME[name]
    return wr.loudness(c["x"], c["rate"], -22.0, f32_storage=f32_storage)


def ld_batch_inputs(names, pad=37):
    cs = [LD_BY_NAME[n] for n in names]
    wav = np.full((len(cs), max(c["L"] for c in cs) + pad), np.nan, np.float32)
    for b, c in enumerate(cs):
        wav[b, :c["L"]] = c["x"]
    return wav, np.array([c["L"] for c in cs], np.int32)
