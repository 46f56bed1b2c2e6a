"""The shapes the PortaSpeech baseline's tests run (test infrastructure): the golden batch and the seeded cases of
tests/test_portaspeech_cpu.py / tests/test_portaspeech_gpu.py, with their float64 and float32 restatements computed once and shared.

A case is {'words': phonemes per word per utterance, 'frames': None (predicted durations) or the teacher-forced frames per utterance
(tests/../synth.ps_spread_mel2word) or an explicit mel2word, 'hp': acoustic hparams, 'seed': of the tokens, 'T_ph' / 'T_w': wider padded axes}.  Every case
totals at most a few hundred frames.  T_ph: 5 = window + 1 is where the reference switches between padding and slicing its relative
table; 4 / 6 / 9 / 10 straddle the band, 31 .. 33 and 64 / 65 / 129 the 16-query and 64-key tiles of the attention kernel."""
import numpy as np
import torch

import portaspeech_ref as pr
from dict_tts_amd import synth

SEED = pr.SEED
N_PHONE = synth.PS_N_PHONE
H128 = {"hidden_size": 128, "num_heads": 2}

GOLDEN_WORDS = [[2, 3, 1, 2, 3, 3, 2, 2, 3, 2], [2, 3, 1, 3, 2, 3, 3], [1]]     # 23 / 17 / 1 phonemes
GOLDEN_TF_FRAMES = [37, 22, 3]                                                  # the teacher-forced run: 37 is no multiple of 4


def words_of(n_ph, seed):
    """words of 1 .. 3 phonemes that add up to n_ph"""
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < n_ph:
        out.append(int(min(rng.integers(1, 4), n_ph - sum(out))))
    return out


def _zero_frame_m2w():
    # word 2 of the first utterance has no frames between live words; 11 frames: the padding repeats the last word
    return np.array([[1, 1, 1, 3, 3, 4, 4, 4, 4, 5, 5], [1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0]], np.int64)


CASES = {"ragged3": {"words": [[3, 1, 2, 2, 3, 1, 2], [2, 2], [1]]},
         "words_of_1": {"words": [[1] * 12, [1] * 5]},
         "word70": {"words": [[2, 70, 3]], "frames": [37]},
         "one_word": {"words": [[3]]},
         "zero_frame_word": {"words": [[2, 1, 3, 2, 1], [3, 2]], "frames": _zero_frame_m2w()},
         "raw_not_mult4": {"words": [[2, 3, 1, 2], [1, 2]], "frames": [41, 18]},
         "h128_heads2": {"words": [[3, 1, 2, 2, 3, 1, 2], [2, 2], [1]], "hp": H128},
         "h128_tph33": {"words": [words_of(33, 133)], "hp": H128}}
# (seeds chosen so that every predicted exp(dur) - 1 stays >= 1e-3 from a half-integer in float64: tests/test_portaspeech_cpu.py asserts it)
_TOKEN_SEED = {31: SEED + 1}
for _n in (1, 4, 5, 6, 9, 10, 31, 32, 33):
    CASES[f"tph{_n}"] = {"words": [words_of(_n, 100 + _n)], "seed": _TOKEN_SEED.get(_n, SEED)}
for _n in (64, 65, 129):   # teacher-forced (two or three frames per word): predicted durations would give ~8 frames per word
    _w = words_of(_n, 100 + _n)
    CASES[f"tph{_n}"] = {"words": [_w], "frames": [2 * len(_w) + len(_w) // 2 + 1]}
GPU_CASES = list(CASES)
PREDICTED = [k for k, c in CASES.items() if c.get("frames") is None]

_SD, _IN, _REF = {}, {}, {}


def sd_np(hp=None):
    key = tuple(sorted((hp or {}).items()))
    if key not in _SD:
        _SD[key] = synth.portaspeech_state_dict(SEED, N_PHONE, acoustic=hp or {})
    return _SD[key]


def inputs(name):
    """-> dict: txt_tokens, ph2word [B, T_ph] int64 numpy, T_w, mel2word (numpy or None), hp, words"""
    if name in _IN:
        return _IN[name]
    c = {"words": GOLDEN_WORDS} if name == "golden" else {"words": GOLDEN_WORDS, "frames": GOLDEN_TF_FRAMES} if name == "golden_tf" else CASES[name]
    b = synth.portaspeech_batch(c["words"], c.get("seed", SEED), N_PHONE, T_ph=c.get("T_ph"), T_w=c.get("T_w"))
    fr = c.get("frames")
    m2w = None if fr is None else (fr if isinstance(fr, np.ndarray) else synth.ps_spread_mel2word(c["words"], fr))
    _IN[name] = {"txt_tokens": b["txt_tokens"], "ph2word": b["ph2word"], "T_w": b["T_w"], "mel2word": m2w, "hp": c.get("hp") or {}, "words": c["words"]}
    return _IN[name]


def noise(name, B, T4, latent=16):
    return synth.randn(SEED, f"ps.z.{name}", (B, latent, T4))


def reference(name, dtype=torch.float64, decode=True):
    """the restatement of case `name` in `dtype`, computed once (float64: the reference; float32: the yardstick of the gate)"""
    key = (name, dtype)
    if key not in _REF:
        i = inputs(name)
        T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
        _REF[key] = pr.forward(pr.state(sd_np(i["hp"]), dtype), i["hp"], T(i["txt_tokens"]), T(i["ph2word"]), i["T_w"], T(i["mel2word"]),
                               z_p=lambda B, T4: T(noise(name, B, T4)), decode=decode)
    return _REF[key]


def live_words(name):
    """words the length regulator reads per utterance: min(live phonemes, T_w)"""
    i = inputs(name)
    return np.minimum((i["txt_tokens"] > 0).sum(1), i["T_w"])
