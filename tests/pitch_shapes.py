"""The seeded case list of the F0 extraction tests (tests/test_pitch_cpu.py, tests/test_pitch_gpu.py).  Every waveform is float32 and has at
most 16 x 256 samples.  At (22050 Hz, hop 256, floor 80, ceiling 750) the window has 824 samples: 827 samples are the shortest utterance
with one frame, 1083 the shortest with two."""
import numpy as np

import pitch_ref as pr

P0 = pr.params(22050, 256, 80.0, 750.0)
PARAM_SETS = {"22050_256_80_750": P0, "22050_128_80_750": pr.params(22050, 128, 80.0, 750.0), "16000_128_80_750": pr.params(16000, 128, 80.0, 750.0),
              "22050_256_50_1100": pr.params(22050, 256, 50.0, 1100.0)}
TONES = (90.0, 123.4, 220.5, 440.0, 700.0)
MAX_SAMPLES = 16 * 256


def tone(f, L, sr=22050, amp=0.3, phase=0.3):
    """five harmonics with amplitudes 1 / k"""
    t = np.arange(L, dtype=np.float64) / sr
    return amp * sum(np.sin(2.0 * np.pi * k * f * t + phase * k) / k for k in range(1, 6))


def glide(L, sr=22050):
    """120 +- 60 Hz, then a stretch of digital zeros, a low-noise stretch and a loud-noise stretch"""
    rng = np.random.RandomState(77)
    t = np.arange(L, dtype=np.float64) / sr
    f = 120.0 + 60.0 * np.sin(2.0 * np.pi * 4.0 * t)
    ph = 2.0 * np.pi * np.cumsum(f) / sr
    x = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 4))
    x[1400:2300] = 0.0
    x[2300:3000] = 1e-4 * rng.standard_normal(700)
    x[3000:] = 0.4 * rng.standard_normal(L - 3000)
    return x


def _case(name, x, p=P0):
    x = np.asarray(x, np.float64).astype(np.float32)
    assert len(x) <= MAX_SAMPLES
    return dict(name=name, x=x, L=len(x), p=p)


def _build():
    rng = np.random.RandomState(1234)
    cases = [_case(f"len_{L}", tone(150.0, L)) for L in (827, 1082, 1083, 12 * 256, 12 * 256 + 1, 12 * 256 + 255)]
    cases += [_case(f"short_{L}", tone(150.0, L)) for L in (826, 0)]
    cases += [_case(f"tone_{f:g}", tone(f, 12 * 256)) for f in TONES]
    cases.append(_case("sine_1500", 0.3 * np.sin(2.0 * np.pi * 1500.0 * np.arange(12 * 256) / 22050.0)))
    cases.append(_case("glide", glide(MAX_SAMPLES)))
    cases.append(_case("noise", 0.2 * rng.standard_normal(12 * 256)))
    cases.append(_case("zeros", np.zeros(12 * 256)))
    cases.append(_case("tone_dc", tone(220.5, 12 * 256) + 0.5))
    cases.append(_case("p_22050_128", tone(200.0, 2500) + 0.01 * rng.standard_normal(2500), PARAM_SETS["22050_128_80_750"]))
    cases.append(_case("p_16000_128", tone(180.0, 2000, sr=16000) + 0.01 * rng.standard_normal(2000), PARAM_SETS["16000_128_80_750"]))
    cases.append(_case("p_22050_50_1100", tone(65.0, MAX_SAMPLES) + 0.01 * rng.standard_normal(MAX_SAMPLES), PARAM_SETS["22050_256_50_1100"]))
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
BATCH = ("tone_123.4", "len_1083", "short_826", "glide", "short_0", "noise", "len_3073")   # mixed lengths, two of them without a frame
BATCH_LD = MAX_SAMPLES + 100


def batch_inputs():
    """-> wav [B, BATCH_LD] float32 with NaN behind each length, lens [B]"""
    wav = np.full((len(BATCH), BATCH_LD), np.nan, np.float32)
    lens = np.zeros(len(BATCH), np.int32)
    for b, name in enumerate(BATCH):
        c = BY_NAME[name]
        wav[b, :c["L"]] = c["x"]
        lens[b] = c["L"]
    return wav, lens


_REFS = {}


def ref(name):
    """the restatement of a case, computed once"""
    if name not in _REFS:
        c = BY_NAME[name]
        _REFS[name] = pr.pitch(c["x"], c["p"])
    return _REFS[name]
