"""The cases of the speaker-conditioning tests (tests/test_speaker_cpu.py, tests/test_speaker_kernels_gpu.py), their float64 references
(tests/acoustic_ref.forward(form=, spk=), tests/posterior_ref.forward_posterior) and the planted defects of the speaker epilogue.

What only a conditioned run reaches, and the shapes that exercise it:
  * layernorm_kernel<true> puts 4 rows in a workgroup and picks the speaker row with b = row / T: ROWMAP has padded T_w 1, 2, 3, 5, 7 at
    B = 4 and B = 5 (B T_w a multiple of 4 and not), every utterance its own speaker, word counts from 1 to the full T_w.
  * spk_linear_kernel strides o += 256 over the channels of a host-transposed W^T [256][C]: HIDDEN has C = 128, 192, 256, 384 (idle
    threads, one full trip, a second trip), words [12, 33, 65], tensor API and resident-table ids; two decoder shapes for the condition.
  * the speaker row handed through run_encoder's split-attention path and the last LayerNorm past the tile: LONG, T_w 129 and 161.
  * spk_gather_kernel's range search strides u += 256: WIDE has B = 257 and B = 300 (T_w = 3), ids 0 and num_spk - 1, repeats, num_spk
    2, 8 and 1000.
  * the posterior pass with speakers: POSTERIOR, both forms, the default shape and hidden 256, ragged lengths and an interior hole.
  * EXACT: embeddings whose projection is exact in fp32 (zero, one-hot, a single -1) and the G11 unit-norm rows.
Each case is a dict: name, kind, shape (an acoustic_ref.CONFIGS key or "default"), form, num_spk, words, offset (into the corpus), fpw
(teacher-forced frames per word of the float64 decode), ids (whether the resident-table path can run it: every utterance needs its
BOS and EOS), spk (the speaker inputs, numpy).
"""
import functools

import numpy as np
import torch

import acoustic_ref as ar
import posterior_ref as pr
import speaker_ref as sr
from dict_tts_amd import synth

SEED = ar.SEED
FORMS = ("embed", "id")
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
H128, H192 = "h128_heads2-mha_dk64-s2pa_d128-conv_cout128", "h192_heads4-mha_dk48"
H256, H384 = "h256_heads4-mha_dk64-s2pa_1x4-post_cond_f32", "h384_heads4-mfma_c384-s2pa_table_d384"
NUM_SPK = {"embed": 4, "id": 8}     # as G11's two checkpoints
MAX_TIES = 1                        # utterances of one case whose mel2word may go uncompared (a duration within 5e-5 of a rounding tie)


def hidden_of(shape):
    return synth.acoustic_shape(ar.shape_hp(shape))["hidden_size"]


def _speakers(name, form, B, num_spk, distinct=False):
    if form == "embed":
        return synth.speaker_inputs(SEED, "embed", B, name=name + ".spk")
    ids = synth.speaker_inputs(SEED, "id", B, num_spk=num_spk, name=name + ".spk")
    if distinct:   # every utterance its own speaker: a seeded start, then steps of 3 (coprime with num_spk = 8)
        assert B <= num_spk and num_spk % 3
        ids = (ids[0] + 3 * np.arange(B)) % num_spk
    return ids.astype(np.int64)


def _case(name, kind, shape, form, words, offset, num_spk=None, fpw=2, spk=None, distinct=False):
    num_spk = NUM_SPK[form] if num_spk is None else num_spk
    spk = _speakers(name, form, len(words), num_spk, distinct) if spk is None else spk
    return {"name": f"{name}-{form}", "kind": kind, "shape": shape, "form": form, "num_spk": num_spk, "words": list(words),
            "offset": offset, "fpw": fpw, "ids": min(words) >= 2, "spk": spk}


def rowmap_words(T_w, B):
    """word counts of a row-mapping batch: utterance 0 fills the padded length (no padded row), utterance 1 has one word (every row
    but one padded), the rest lie between"""
    w = [T_w, 1, max(1, T_w - 1), max(1, T_w // 2), max(1, T_w - 2)]
    return w[:B]


ROWMAP = [_case(f"rowmap_Tw{t}_B{B}", "rowmap", "default", form, rowmap_words(t, B), 1300 + 10 * t, distinct=True, fpw=3)
          for t in (1, 2, 3, 5, 7) for B in (4, 5) for form in FORMS]

HIDDEN = [_case(f"hidden_{shape.split('_')[0]}", "hidden", shape, form, [12, 33, 65], 1400)
          for shape in (H128, H192, H256, H384) for form in FORMS] + \
         [_case("cond_fvae96", "hidden", "fvae96_k3_dec2-vconv", "embed", [12, 33, 65], 1400, fpw=4),
          _case("cond_glow8", "hidden", "glow_blocks8-flowstack_rc64", "id", [12, 33, 65], 1400, fpw=4)]

LONG = [_case(f"long_{'_'.join(map(str, w))}", "long", "default", form, w, 1450) for w in ([128, 129], [161]) for form in FORMS]


def wide_words(B):
    return [1 + b % 3 for b in range(B)]


def _wide_ids(name, B, num_spk):
    """both ends of [0, num_spk), repeats across the gather's 256-utterance search stride, the rest seeded"""
    ids = _speakers(name, "id", B, num_spk)
    ids[0], ids[1], ids[-1] = 0, num_spk - 1, num_spk - 1
    ids[254] = ids[255] = ids[256] = ids[2]
    return ids


WIDE = [_case(f"wide_B{B}_spk{n}", "wide", "default", "id", wide_words(B), 1700, num_spk=n, spk=_wide_ids(f"wide_B{B}_spk{n}", B, n))
        for B, n in ((257, 2), (257, 1000), (300, 8))] + \
       [_case(f"wide_B{B}", "wide", "default", "embed", wide_words(B), 1700) for B in (257, 300)]

POSTERIOR = [_case(f"posterior_{shape.split('_')[0]}", "posterior", shape, form, [12, 33, 65, 130], 1000)
             for shape in ("default", H256) for form in FORMS]


def _onehot(ks, signs):
    e = np.zeros((len(ks), synth.SPK_EMBED_DIM), np.float32)
    for b, (k, s) in enumerate(zip(ks, signs)):
        e[b, k] = s
    return e


ONEHOT_K, ONEHOT_SIGN = (0, 1, 127, 255, 100), (1.0, 1.0, 1.0, 1.0, -1.0)   # the last utterance: a single -1
EXACT = [_case("exact_zero", "exact", "default", "embed", [4, 7, 2, 5], 1420, spk=np.zeros((4, synth.SPK_EMBED_DIM), np.float32)),
         _case("exact_onehot", "exact", "default", "embed", [3, 7, 5, 2, 6], 1420, spk=_onehot(ONEHOT_K, ONEHOT_SIGN))]
G11 = {"name": "exact_g11-embed", "kind": "g11", "shape": "default", "form": "embed", "num_spk": 4, "words": None, "offset": None,
       "fpw": 4, "ids": False, "spk": sr.g11_speakers("embed")}
INFER = ROWMAP + HIDDEN + LONG + WIDE + EXACT + [G11]
BY_NAME = {c["name"]: c for c in INFER + POSTERIOR}
assert len(BY_NAME) == len(INFER) + len(POSTERIOR)


# ---------------------------------------------------------------------------------------------------------------------------------------
WORD_AXIS = ("word_tokens", "keys", "values", "key_map", "pinyin", "pinyin_map", "pron_modified")


@functools.lru_cache(maxsize=4)
def batch(name):
    """the collated batch of a case.  Padded T_w 1 and 2 hold no dictionary word (BOS and EOS only), which the collater cannot size:
    such a batch is collated beside a 3-word utterance that is then dropped and its word axis cut to T_w; the collater's value-1 pad
    of the last row moves with the cut."""
    c = BY_NAME[name]
    if c["kind"] == "g11":
        return sr.g11_batch()
    T_w, B = max(c["words"]), len(c["words"])
    if T_w >= 3:
        b = ar.batch_of(c["words"], c["offset"])
    else:
        b = {k: np.ascontiguousarray(v[:B, :T_w]) for k, v in ar.batch_of(c["words"] + [3], c["offset"]).items()}
        b["key_map"][:, -1, :] = 1
        b["pinyin_map"][:, -1, :] = 1
    assert set(b) == set(WORD_AXIS) and ((b["word_tokens"] > 0).sum(1) == c["words"]).all()
    return b


def word_counts(name):
    return [int(n) for n in (batch(name)["word_tokens"] > 0).sum(1)]


def sentences(name):
    c = BY_NAME[name]
    assert c["ids"]
    return ar.sentences_of(c["words"], c["offset"])


def mel2word(name):
    """teacher-forced: fpw frames per word.  The posterior cases take test_text2mel_kernels_gpu.shape_case's lengths (T_mel/4 at RC - 1,
    RC, RC + 1, 1.5 RC of the shape's flow chunk: ragged) and an 8-frame hole of zeros 4 frames before the end of utterance 1"""
    c = BY_NAME[name]
    wt = batch(name)["word_tokens"]
    if c["kind"] != "posterior":
        return ar.spread_mel2word(wt, [c["fpw"] * n for n in word_counts(name)])
    rc = ar.flow_rc(ar.shape_hp(c["shape"]))
    frames = [4 * t for t in (rc - 1, rc, rc + 1, rc + rc // 2)]
    m2w = ar.spread_mel2word(wt, frames)
    m2w[1, frames[1] - 12:frames[1] - 4] = 0
    return m2w


def prior_noise(name):
    c = BY_NAME[name]
    m2w = mel2word(name)
    T4 = (m2w.shape[1] + 3) // 4
    return synth.randn(SEED, name + ".z", (m2w.shape[0], synth.acoustic_shape(ar.shape_hp(c["shape"]))["latent_size"], T4))


def state_np(c):
    if c["kind"] == "g11":
        return sr.g11_state_dict(c["form"])
    return ar.sd_np(ar.shape_hp(c["shape"]), c["form"], c["num_spk"])


def spk_tensor(c, dtype):
    return T(c["spk"]) if c["form"] == "id" else T(c["spk"]).to(dtype)


def predicted_mel2word(want, word_tokens):
    """mel2word from the restatement's durations: add_dur's rounding and length regulator over the valid words (dur_input is masked:
    model.py:96), expand's pad to frames_multiple"""
    from oracle import dict_tts_ref as ref
    d = torch.clamp(torch.round(want["dur"].exp() - 1), min=0).long()
    m2w = ref.length_regulator(d, (word_tokens > 0).long().sum(-1))
    return ref.expand(want["word_encoder_out"], m2w)[2]


def near_ties(want, word_tokens):
    """utterances with a valid word whose duration lies within 5e-5 of a rounding tie in the reference"""
    v = want["dur"].exp() - 1
    tie = ((v - v.floor() - 0.5).abs() < 5e-5) & (word_tokens > 0)
    return sorted(set(int(b) for b in torch.nonzero(tie)[:, 0]))


def forward(name, dtype=torch.float64, spk_hook=None):
    """the restatement of an INFER case in `dtype`, decoding the teacher-forced mel2word(name) from prior_noise(name); adds
    'pred_mel2word' (what the predicted durations give) and 'ties'"""
    c = BY_NAME[name]
    b = batch(name)
    hp = ar.shape_hp(c["shape"])
    want = ar.forward(ar.state(state_np(c), dtype), hp, *ar.inputs(b, dtype), mel2word=T(mel2word(name)), z_p=T(prior_noise(name)),
                      form=c["form"], spk=spk_tensor(c, dtype), spk_hook=spk_hook)
    wt = T(b["word_tokens"])
    want["pred_mel2word"] = predicted_mel2word(want, wt)
    want["ties"] = near_ties(want, wt)
    return want


@functools.lru_cache(maxsize=2)
def reference(name):
    return forward(name)


def posterior_inputs(name):
    m2w = mel2word(name)
    mels = pr.tgt_mels_for(m2w, name=name + ".mel")
    c = BY_NAME[name]
    Z = synth.acoustic_shape(ar.shape_hp(c["shape"]))["latent_size"]
    return m2w, mels, synth.randn(SEED, name + ".eps", (mels.shape[0], Z, mels.shape[1] // 4))


def posterior(name, dtype=torch.float64):
    c = BY_NAME[name]
    m2w, mels, eps = posterior_inputs(name)
    return pr.forward_posterior(ar.state(state_np(c), dtype), *ar.inputs(batch(name), dtype), T(mels).to(dtype), T(m2w), T(eps).to(dtype),
                                form=c["form"], spk=spk_tensor(c, dtype), hp=ar.shape_hp(c["shape"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the projected rows, element by element
GAMMA_257 = 257 * 2.0 ** -24 / (1 - 257 * 2.0 ** -24)   # a fixed-order fp32 chain of 256 FMAs and one add (Higham, Accuracy and Stability, 3.1)


def speaker_rows(c):
    """-> (rows64 [B, C] float64, bound [B, C] or None): the projection in float64 and, for the linear form, the forward error bound
    gamma_257 (sum_k |W[o,k] e[k]| + |bias[o]|) of its fp32 evaluation in any fixed order.  Form "id": the table rows, exact."""
    sd = state_np(c)
    W = sd["spk_embed_proj.weight"].astype(np.float64)
    if c["form"] == "id":
        return W[c["spk"]], None
    e, bias = c["spk"].astype(np.float64), sd["spk_embed_proj.bias"].astype(np.float64)
    return e @ W.T + bias, GAMMA_257 * (np.abs(e) @ np.abs(W).T + np.abs(bias))


def exact_rows(c):
    """the EXACT cases' rows as the fp32 FMA chain gives them: exact zeros and at most one exact product, then the bias"""
    sd = state_np(c)
    W, bias = sd["spk_embed_proj.weight"], sd["spk_embed_proj.bias"]
    out = np.empty((len(c["spk"]), W.shape[0]), np.float32)
    for b, e in enumerate(c["spk"]):
        k = np.nonzero(e)[0]
        assert len(k) <= 1 and (len(k) == 0 or abs(e[k[0]]) == 1)
        out[b] = bias if len(k) == 0 else (np.float32(e[k[0]]) * W[:, k[0]]).astype(np.float32) + bias
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Planted defects of the speaker epilogue: spk_hook(weo, rows, nonpadding) -> (word_encoder_out, dur_input) for acoustic_ref.forward
def defect_neighbour_row(move=5e-5):
    """(a) the first valid row of every utterance b > 0 takes utterance b - 1's speaker row, scaled so that the row moves by `move`"""
    def hook(weo, rows, nonpadding):
        out = weo + rows[:, None, :]
        for b in range(1, weo.shape[0]):
            d = rows[b - 1] - rows[b]
            out[b, 0] += d * (move / float(d.abs().max()))
        return out, None
    return hook


def defect_untransposed_pair(sd, spk, o=5, k=200):
    """(b) one (o, k) pair of the linear projection read as (k mod C, o mod 256): W^T indexed untransposed"""
    W = sd["spk_embed_proj.weight"]
    C = W.shape[0]

    def hook(weo, rows, nonpadding):
        rows = rows.clone()
        rows[:, o] += (W[k % C, o % 256] - W[o, k]) * spk[:, k].to(W.dtype)
        return weo + rows[:, None, :], None
    return hook


def defect_unmasked_duration_input():
    """(c) the nonpadding mask in front of the duration predictor dropped: padded rows carry the speaker"""
    def hook(weo, rows, nonpadding):
        out = weo + rows[:, None, :]
        return out, out
    return hook
