"""Config-driven restatement of ``PortaSpeech_dict.forward(infer=True)`` at ANY acoustic shape the library accepts, in fp32 or float64
(test infrastructure), the non-default shapes the text-to-mel tests run, and the per-row comparison they use.

``forward`` composes the oracle's pieces (oracle/dict_tts_ref.py: dict_encoder, add_dur, expand, prior_flow_reverse, wn; fvae_infer's
body) with every shape taken from the hparams (synth.acoustic_shape); ``form`` / ``spk`` add the speaker conditioning of
tests/speaker_ref.py at any shape and dtype; the posterior pass is tests/posterior_ref.forward_posterior(hp=..., form=..., spk=...).
The dtype of the folded state dict decides the arithmetic: ``state(..., torch.float64)`` gives the float64 reference the GPU is compared
with.  At the ps_flow.yaml shape in fp32 it IS oracle.dict_tts_ref.forward_infer, bit for bit (tests/test_acoustic_ref_cpu.py).

``rowcmp`` reports, for outputs with rows on axis 1 (frames or words): the max abs error and where it is, the largest RMS over a
window of WIN consecutive rows of one utterance and where it starts, and the global RMS.  ``check`` prints one ``T2MMEAS {json}`` line
per comparison (run pytest with -s to see them) and returns the bounds it exceeds.
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

import speaker_ref
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref
from oracle import hifigan_ref as href

SEED = 1234
WIN = 8                       # rows per window: 8 frames of mel, 8 words of the encoder outputs
GLOW_LAYERS = 4               # WaveNet layers of a coupling layer (fvae_semantics.py:77-78: ResidualCouplingBlock(..., 4, ...))

# The non-default shapes: test id (named after the branch the shape forces) -> acoustic hparams.  Every one is accepted by dtts_create.
# An odd prior_glow_n_blocks (1 would give the flowstack chunk of 120 rows) is refused by dtts_finalize_weights (the flow's Flip parity).
CONFIGS = {
    "h256_heads4-mha_dk64-s2pa_1x4-post_cond_f32": {"hidden_size": 256, "num_heads": 4},
    "h128_heads2-mha_dk64-s2pa_d128-conv_cout128": {"hidden_size": 128, "num_heads": 2},
    "h384_heads4-mfma_c384-s2pa_table_d384": {"hidden_size": 384, "num_heads": 4},
    "h192_heads4-mha_dk48": {"hidden_size": 192, "num_heads": 4},
    "fvae96_k3_dec2-vconv": {"fvae_enc_dec_hidden": 96, "fvae_kernel_size": 3, "fvae_dec_n_layers": 2},
    "fvae160_k7_dec6-vconv": {"fvae_enc_dec_hidden": 160, "fvae_kernel_size": 7, "fvae_dec_n_layers": 6},
    "fvae256_k5-vconv": {"fvae_enc_dec_hidden": 256},
    "glow_blocks2-flowstack_rc112": {"prior_glow_n_blocks": 2},
    "glow_blocks8-flowstack_rc64": {"prior_glow_n_blocks": 8},
    "glow_k5_h128_latent8-flow_fallback": {"glow_kernel_size": 5, "prior_glow_hidden": 128, "latent_size": 8},
    "ffn3_dur_k3_l2-conv_k3": {"enc_ffn_kernel_size": 3, "dur_predictor_kernel": 3, "dur_predictor_layers": 2},
    "ffn9-conv_k9": {"enc_ffn_kernel_size": 9},
}


def flow_rc(hp=None):
    """rows a flowstack chunk keeps (flowstack.hip: W = 128 rows, halo = n_blocks * n_layers rows per side)"""
    return 128 - 2 * synth.acoustic_shape(hp)["prior_glow_n_blocks"] * GLOW_LAYERS


def state(sd_np, dtype=torch.float32):
    """numpy state dict -> folded torch state dict in `dtype` (the weight-norm fold itself runs in that dtype)"""
    return href.fold_weight_norm({k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd_np.items()})


def inputs(batch, dtype=torch.float32):
    """a synth.make_batch dict -> (word_tokens, dict_msg, pron_modified) as torch tensors, the float ones in `dtype`"""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in batch.items()}
    f = lambda x: x.to(dtype)
    return t["word_tokens"], (f(t["keys"]), f(t["values"]), f(t["key_map"]), t["pinyin"], t["pinyin_map"]), t["pron_modified"]


def forward(sd, hp, word_tokens, dict_msg, pron_modified, mel2word=None, z_p=None, hook=None, form=None, spk=None, spk_hook=None):
    """PortaSpeech_dict.forward(infer=True) (modules/dict_tts/model.py:36-62,84-121) at the shape of hparams hp.  sd: state(...);
    z_p: [B, latent, T_mel/4] or a callable (B, T4) -> tensor; hook: oracle.dict_tts_ref.wn's (plants a kernel defect).
    form / spk: speaker conditioning exactly as tests/speaker_ref.forward_infer_spk restates it ("embed": spk [B, 256] in sd's dtype,
    "id": int64 [B]; None = none, bit for bit the unconditioned forward); spk_hook(weo, rows, nonpadding) -> (weo, dur_input), if given,
    replaces the two speaker lines (plants a defect of the speaker epilogue: tests/speaker_shapes.py).
    -> word_encoder_out, dict_attn, pron_attn, context, dur, mel2word, x_mask, z (the reverse flow's output), mel_out"""
    sh = synth.acoustic_shape(hp)
    dt = sd["fvae.decoder.out_proj.weight"].dtype
    with torch.no_grad():
        ret = {}
        weo, dict_attn, pron_attn, context = ref.dict_encoder(sd, word_tokens, dict_msg, pron_modified, sh["hidden_size"], sh["num_heads"],
                                                              sh["enc_ffn_kernel_size"])
        nonpadding = (1 - word_tokens.eq(0).to(dt))[:, :, None]
        dur_input = None
        if form is not None:
            rows = speaker_ref.project(sd, form, spk)
            if spk_hook is not None:
                weo, dur_input = spk_hook(weo, rows, nonpadding)
            else:
                weo = weo + rows[:, None, :]                                    # model.py:94, every row
        ret.update(dict_attn=dict_attn, pron_attn=pron_attn, word_encoder_out=weo, context=context)
        if dur_input is None:
            dur_input = weo * nonpadding                                        # model.py:96
        dur, mel2word = ref.add_dur(sd, dur_input, mel2word, sh["dur_predictor_layers"], sh["dur_predictor_kernel"])
        ret["dur"] = dur
        x, tgt_nonpadding, mel2word = ref.expand(weo, mel2word)
        ret["mel2word"] = mel2word
        x = x * tgt_nonpadding
        ret["x_mask"] = tgt_nonpadding
        g = x.transpose(1, 2)
        if callable(z_p):
            z_p = z_p(g.shape[0], g.shape[2] // 4)
        z_p = z_p.to(dt)
        # fvae_infer (oracle) with the shape's widths, kernels and depths
        g_sqz = F.conv1d(g, sd["fvae.g_pre_net.0.weight"], sd["fvae.g_pre_net.0.bias"], stride=4, padding=2)
        z = ref.prior_flow_reverse(sd, z_p, g_sqz, sh["prior_glow_n_blocks"], sh["prior_glow_hidden"], sh["glow_kernel_size"], GLOW_LAYERS,
                                   hook)
        x = F.conv_transpose1d(z, sd["fvae.decoder.pre_net.0.weight"], sd["fvae.decoder.pre_net.0.bias"], stride=4)
        x = ref.wn(sd, "fvae.decoder.wn", x, g, sh["fvae_enc_dec_hidden"], sh["fvae_kernel_size"], sh["fvae_dec_n_layers"], hook)
        mel = F.conv1d(x, sd["fvae.decoder.out_proj.weight"], sd["fvae.decoder.out_proj.bias"])
        ret["z"] = z
        ret["mel_out"] = mel.transpose(1, 2)
        return ret


# ---------------------------------------------------------------------------------------------------------------------------------------
def spread_mel2word(word_tokens, frames):
    """teacher-forced mel2word giving utterance b exactly frames[b] frames (>= its word count), spread as evenly as possible over its
    words (the first words take the remainder): [B, max(frames)] int64, 0 = padding"""
    rows = []
    for wt, n_f in zip(np.asarray(word_tokens), frames):
        n = int((wt > 0).sum())
        assert 1 <= n <= n_f, (n, n_f)
        d = np.full(n, n_f // n)
        d[:n_f % n] += 1
        rows.append(np.repeat(np.arange(1, n + 1), d))
    out = np.zeros((len(rows), max(len(r) for r in rows)), np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


_SHORT = None


def short_gloss_words(max_len=40):
    """Biaobei word ids whose dictionary entry has at most max_len gloss tokens, in corpus order (long sentences built from them keep
    the collated key tensors, and so the float64 reference, small)"""
    global _SHORT
    if _SHORT is None:
        st = synth.biaobei_struct()
        ent = st["entries"]
        _SHORT = [w for s in st["sentences"] for w in s if sum(x[0] for x in ent[w]) <= max_len]
    return _SHORT


def sentences_of(word_counts, offset=0):
    """sentences of the given word counts (T_w per utterance INCLUDING BOS / EOS, >= 2) cut from the corpus; a count of 1 is an
    utterance whose only valid word is BOS (see batch_of)"""
    ids = short_gloss_words()
    out, at = [], offset
    for n in word_counts:
        k = max(0, n - 2)
        out.append(ids[at:at + k])
        at += k
    return out


def batch_of(word_counts, offset=0, pron_every=3):
    """a collated batch (synth.make_batch) whose utterances have exactly `word_counts` valid words"""
    batch = synth.make_batch(sentences_of(word_counts, offset), SEED, pron_every=pron_every)
    for b, n in enumerate(word_counts):
        if n == 1:   # only BOS: the word axis' valid length is 1
            batch["word_tokens"][b, 1:] = 0
            batch["pron_modified"][b, 1:] = 0
    return batch


# ---------------------------------------------------------------------------------------------------------------------------------------
def rowcmp(got, want, win=WIN):
    """got / want: [B, T, ...] (rows on axis 1).  -> {'max', 'at' [b, t], 'win' (largest RMS over `win` consecutive rows of one
    utterance), 'win_at' [b, t0], 'rms'}; the difference is taken in float64"""
    g = np.asarray(got.detach().cpu() if hasattr(got, "detach") else got, np.float64)
    w = np.asarray(want.detach().cpu() if hasattr(want, "detach") else want, np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    d = (g - w).reshape(g.shape[0], g.shape[1], -1)
    ad = np.abs(d)
    b, t = np.unravel_index(int(ad.max(axis=2).argmax()), ad.shape[:2])
    sq = np.square(d).sum(axis=2)                                  # [B, T]
    n = min(win, d.shape[1])
    cs = np.concatenate([np.zeros((d.shape[0], 1)), np.cumsum(sq, axis=1)], axis=1)
    wsum = (cs[:, n:] - cs[:, :-n]) / (n * d.shape[2])             # [B, T - n + 1]
    wb, wt = np.unravel_index(int(wsum.argmax()), wsum.shape)
    return {"max": float(ad.max()), "at": [int(b), int(t)], "win": float(np.sqrt(wsum.max())), "win_at": [int(wb), int(wt)],
            "rms": float(np.sqrt(np.mean(np.square(d))))}


def check(case, what, got, want, bounds, win=WIN):
    """rowcmp + one T2MMEAS line; -> list of '<what> <stat> <value> > <bound>' for the exceeded bounds (empty = within)"""
    v = rowcmp(got, want, win)
    print("T2MMEAS " + json.dumps({"case": case, "what": what, **v}), flush=True)
    return [f"{what} {k} {v[k]:.3g} > {bounds[k]:.3g} (max at {v['at']}, worst window at {v['win_at']})"
            for k in ("max", "win", "rms") if v[k] > bounds[k]]


# Per-row bounds of GPU - float64 (tests/test_text2mel_kernels_gpu.py), each at most 3x the worst value measured on MI355X over every case
# of that file (measured max / 8-row window RMS / RMS in the comments; the B = 1 encoder cases brought the encoder outputs' RMS to 1.5x).  These are the first GPU - float64 figures for text-to-mel; the
# earlier ones were GPU - fp32 oracle (mel 3e-5, posterior 1.5e-4), and the fp32 oracle is itself ~1e-5 from float64.
BOUNDS = {
    "mel": {"max": 1.0e-4, "win": 2.5e-5, "rms": 2.0e-5},                 # 3.5e-5 / 8.5e-6 / 7.0e-6 (infer; split-bf16 decoder)
    "mel_post": {"max": 8.9e-4, "win": 2.2e-4, "rms": 6.8e-5},            # 3.0e-4 / 7.5e-5 / 2.3e-5 (posterior reconstruction)
    "word_encoder_out": {"max": 3.8e-5, "win": 4.8e-6, "rms": 1.9e-6},    # 1.5e-5 / 2.6e-6 / 1.3e-6
    "context": {"max": 7.2e-5, "win": 8.5e-6, "rms": 2.9e-6},             # 2.9e-5 / 4.0e-6 / 2.0e-6
    "dur": {"max": 1.1e-5, "win": 5.4e-6, "rms": 2.0e-6},                 # 5.4e-6 / 2.4e-6 / 1.3e-6
    "dict_attn": {"max": 1.4e-5, "win": 1.3e-6, "rms": 5.1e-7},           # 6.0e-6 / 6.9e-7 / 3.3e-7
    "pron_attn": {"max": 7.7e-6, "win": 2.7e-6, "rms": 4.4e-7},           # 2.6e-6 / 9.1e-7 / 1.5e-7
    "z_p": {"max": 1.0e-2, "win": 9.6e-4, "rms": 3.3e-4},                 # 3.4e-3 / 3.2e-4 / 1.1e-4 (|z_p| reaches ~57)
    "m_q": {"max": 1.6e-4, "win": 4.4e-5, "rms": 3.2e-5},                 # 5.3e-5 / 1.5e-5 / 1.1e-5
    "logs_q": {"max": 1.7e-4, "win": 4.2e-5, "rms": 3.0e-5},              # 5.7e-5 / 1.4e-5 / 1.0e-5
}
KL_REL = 1.4e-5                                                           # |kl - kl64| / |kl64|: 4.8e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
# shared by tests/test_text2mel_kernels_gpu.py, tests/test_s2pa_cpu.py and tests/test_s2pa_gpu.py
_SD = {}


def sd_np(hp, form=None, num_spk=4):
    """the seeded state dict of shape hp; form "embed" / "id" adds the spk_embed_proj of a checkpoint with num_spk speakers"""
    key = tuple(sorted(hp.items())) + (() if form is None else (form, num_spk))
    if key not in _SD:
        _SD[key] = synth.dict_tts_state_dict(SEED, acoustic=hp, speaker=form, num_spk=num_spk)
    return _SD[key]


def shape_hp(name):
    return {} if name == "default" else CONFIGS[name]


def as_rows(k, x, word_mask):
    """-> [B, rows, ...] float64 numpy with rows on axis 1; the S2PA context only on valid words (the reference masks it)"""
    x = x.detach().cpu().double()
    if k == "dict_attn":
        x = x[:, 0].transpose(1, 2)           # [B, 1, L_k, T_w] -> [B, T_w, L_k]
    if k == "dur":
        x = x[..., None]
    if k == "context":
        x = x * word_mask[..., None]
    return x.numpy()


def compare(case, got, want, keys, fails, batch=None, sel=None, mel="mel"):
    """append the exceeded bounds of got vs want to fails; sel: an index into [B, rows] (e.g. (slice(b, b + 1), slice(0, n))), all rows by
    default; mel: the BOUNDS entry of mel_out"""
    word_mask = torch.from_numpy(batch["word_tokens"] > 0).double() if batch is not None else None
    for k in keys:
        g, w = as_rows(k, got[k], word_mask), as_rows(k, want[k], word_mask)
        if sel is not None:
            g, w = g[sel], w[sel]
        bk = mel if k == "mel_out" else k
        fails += [f"{case}: {f}" for f in check(case, k, g, w, BOUNDS[bk])]


def bf16_halo(sd, site, layer, row, halo_rows):
    """a planted kernel defect for forward(hook=...): the tile whose first output row is `row` reads its halo rows `halo_rows` of layer
    `layer` of WaveNet `site` rounded to bf16 (the low half of a split-bf16 operand dropped at the seam)"""
    def hook(p, i, x, x_in):
        if p != site or i != layer:
            return x_in
        xx = x.clone()
        for r in halo_rows:
            xx[:, :, r] = x[:, :, r].to(torch.bfloat16).to(x.dtype)
        w, b = sd[f"{p}.in_layers.{i}.weight"], sd[f"{p}.in_layers.{i}.bias"]
        y = F.conv1d(xx, w, b, padding=(w.shape[-1] - 1) // 2)
        x_in = x_in.clone()
        x_in[:, :, row] = y[:, :, row]
        return x_in
    return hook
