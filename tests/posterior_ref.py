"""CPU fp32 restatement of the teacher-forced ``PortaSpeech_dict.forward(infer=False)`` (no gradients, eval mode) and the G12 cases
(test infrastructure).

Composed from the oracle's pieces (oracle/dict_tts_ref.py: dict_encoder, add_dur, expand) plus what the posterior branch adds:
  - the masked WaveNet                    modules/commons/wavenet.py:54-78 (x = (x + res) * x_mask; output * x_mask)
  - the posterior encoder                 modules/dict_tts/fvae_semantics.py:10-35
  - the prior flow, forward, masked       modules/portaspeech/glow_modules.py:108-123,157-161
  - the KL                                modules/dict_tts/fvae_semantics.py:94-99
  - the decoder with the frame mask       modules/dict_tts/fvae_semantics.py:52-57
  - the return keys                       modules/dict_tts/model.py:55-58,109-121
G12 (tests/golden/g12_posterior.npz, written by tools/make_golden_posterior.py from the reference itself) pins this restatement.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import golden_cases as gc
import speaker_ref as sr
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref

SEED = gc.SEED
G12_SENTENCES = (4, 11, 18, 26, 34)     # Biaobei sentences: a ragged batch
G12_HOLE = (2, 20, 28)                  # utterance 2: frames [20, 28) get mel2word = 0 inside the utterance
G12_FRAMES = (6, 3)                     # teacher-forced frames per character / for BOS and EOS (short: a small fixture)
CASES = {"plain": {"form": None}, "id": {"form": "id"}}
G12_SPK_IDS = np.array([1, 6, 0, 6, 4], np.int64)


def g12_batch():
    st = synth.biaobei_struct()
    return synth.make_batch([st["sentences"][i] for i in G12_SENTENCES], SEED, pron_every=3)


def g12_mel2word(word_tokens):
    """teacher-forced mel2word (G12_FRAMES per character / BOS / EOS) with interior zeros in one utterance; the longest utterance
    loses two frames of its last word, so that the length is not a multiple of frames_multiple (the pad of model.py:98-100 runs)"""
    m2w = synth.teacher_mel2word(word_tokens, *G12_FRAMES)
    b, lo, hi = G12_HOLE
    m2w[b, lo:hi] = 0
    last = int(np.argmax([np.nonzero(r)[0].max() for r in m2w]))
    end = int(np.nonzero(m2w[last])[0].max()) + 1
    m2w[last, end - 2:end] = 0
    keep = int(max(np.nonzero(r)[0].max() for r in m2w)) + 1
    return np.ascontiguousarray(m2w[:, :keep])


def tgt_mels_for(mel2word, seed=SEED, name="g12.mel", frames_multiple=4):
    """[B, T_mel, 80]: random log-mels over each utterance's span (interior holes keep their frames: the mask must remove them), zero
    beyond the last frame, as the collater pads them; T_mel = mel2word's length after the frames_multiple pad"""
    B, T = mel2word.shape
    T_mel = T + (-T) % frames_multiple
    out = np.zeros((B, T_mel, synth.N_MEL), np.float32)
    for b in range(B):
        n = int(np.nonzero(mel2word[b])[0].max()) + 1
        out[b, :n] = synth.random_mel(seed, n, f"{name}.{b}")
    return out


def mels_fingerprint(mels):
    """per-utterance float64 sums and sums of squares: G12 stores these instead of the regenerable [B, T_mel, 80] inputs"""
    m = np.asarray(mels, np.float64)
    return np.stack([m.sum((1, 2)), np.square(m).sum((1, 2))], 1)


def g12_eps(name, B, T4):
    return synth.randn(SEED, f"g12.eps.{name}", (B, 16, T4))


def g12_state_dict(case):
    form = CASES[case]["form"]
    if form is None:
        return synth.dict_tts_state_dict(SEED)
    return sr.g11_state_dict(form)


def g12_speakers(case):
    return G12_SPK_IDS.copy() if CASES[case]["form"] == "id" else None


# ---------------------------------------------------------------------------------------------------------
def wn_masked(sd, p, x, x_mask, g, hidden, k, n_layers):
    """WN.forward with a frame mask, dilation_rate 1 (modules/commons/wavenet.py:54-78); x must arrive masked"""
    output = torch.zeros_like(x)
    g = F.conv1d(g, sd[p + ".cond_layer.weight"], sd[p + ".cond_layer.bias"])
    for i in range(n_layers):
        x_in = F.conv1d(x, sd[f"{p}.in_layers.{i}.weight"], sd[f"{p}.in_layers.{i}.bias"], padding=(k - 1) // 2)
        in_act = x_in + g[:, i * 2 * hidden:(i + 1) * 2 * hidden, :]
        acts = torch.tanh(in_act[:, :hidden, :]) * torch.sigmoid(in_act[:, hidden:, :])
        rs = F.conv1d(acts, sd[f"{p}.res_skip_layers.{i}.weight"], sd[f"{p}.res_skip_layers.{i}.bias"])
        if i < n_layers - 1:
            x = (x + rs[:, :hidden, :]) * x_mask
            output = output + rs[:, hidden:, :]
        else:
            output = output + rs
    return output * x_mask


def posterior_encoder(sd, x, x_mask, g_sqz, eps, hidden=192, k=5, n_layers=8, latent=16):
    """FVAEEncoder.forward (modules/dict_tts/fvae_semantics.py:29-35) with the sample's noise given: x [B,80,T], x_mask [B,1,T]"""
    h = F.conv1d(x, sd["fvae.encoder.pre_net.0.weight"], sd["fvae.encoder.pre_net.0.bias"], stride=4, padding=2)
    x_mask = x_mask[:, :, ::4][:, :, :h.shape[-1]]
    h = h * x_mask
    h = wn_masked(sd, "fvae.encoder.wn", h, x_mask, g_sqz, hidden, k, n_layers) * x_mask
    h = F.conv1d(h, sd["fvae.encoder.out_proj.weight"], sd["fvae.encoder.out_proj.bias"])
    m, logs = torch.split(h, latent, dim=1)
    z = m + eps * torch.exp(logs)
    return z, m, logs, x_mask


def prior_flow_forward(sd, z, x_mask, g_sqz, n_flows=4, hidden=64, k=3, n_layers=4):
    """ResidualCouplingBlock.forward(reverse=False) (modules/portaspeech/glow_modules.py:157-161): [coupling, Flip] x n_flows in order;
    ResidualCouplingLayer.forward mean_only (:108-123); Flip (:9-13)"""
    half = z.shape[1] // 2
    for f in range(n_flows):
        p = f"fvae.prior_flow.flows.{2 * f}"
        x0, x1 = z[:, :half], z[:, half:]
        h = F.conv1d(x0, sd[p + ".pre.weight"], sd[p + ".pre.bias"]) * x_mask
        h = wn_masked(sd, p + ".enc", h, x_mask, g_sqz, hidden, k, n_layers)
        m = F.conv1d(h, sd[p + ".post.weight"], sd[p + ".post.bias"]) * x_mask
        x1 = m + x1 * torch.exp(torch.zeros_like(m)) * x_mask
        z = torch.flip(torch.cat([x0, x1], 1), [1])
    return z


def normal_log_prob(value, loc, scale):
    """torch.distributions.Normal.log_prob"""
    var = scale ** 2
    log_scale = math.log(scale) if isinstance(scale, (int, float)) else scale.log()
    return -((value - loc) ** 2) / (2 * var) - log_scale - math.log(math.sqrt(2 * math.pi))


def kl_term(z_q, m_q, logs_q, z_p, x_mask_sqz):
    """fvae_semantics.py:94-99 (use_prior_glow)"""
    logqx = normal_log_prob(z_q, m_q, logs_q.exp())
    logpx = normal_log_prob(z_p, 0.0, 1.0)
    return ((logqx - logpx) * x_mask_sqz).sum() / x_mask_sqz.sum() / logqx.shape[1]


def decoder_masked(sd, z, x_mask, g, hidden=192, k=5, n_layers=4):
    """FVAEDecoder.forward with the frame mask (modules/dict_tts/fvae_semantics.py:52-57)"""
    x = F.conv_transpose1d(z, sd["fvae.decoder.pre_net.0.weight"], sd["fvae.decoder.pre_net.0.bias"], stride=4)
    x = x * x_mask
    x = wn_masked(sd, "fvae.decoder.wn", x, x_mask, g, hidden, k, n_layers) * x_mask
    return F.conv1d(x, sd["fvae.decoder.out_proj.weight"], sd["fvae.decoder.out_proj.bias"])


def forward_posterior(sd, word_tokens, dict_msg, pron_modified, tgt_mels, mel2word, eps, form=None, spk=None, hp=None):
    """PortaSpeech_dict.forward(infer=False) under no_grad, no post-glow (modules/dict_tts/model.py:36-62,84-121; fvae_semantics.py:84-108).
    sd: folded state dict (torch, fp32 or float64: every float input must have its dtype); tgt_mels [B,T_mel,80]; mel2word [B,T] or None
    (predicted durations); eps [B,latent,T_mel/4]; form / spk: speaker conditioning as in tests/speaker_ref.py (None = none); hp: the acoustic
    hparams of the shape (synth.acoustic_shape; None = ps_flow.yaml's)."""
    sh = synth.acoustic_shape(hp)
    Hd, kf = sh["fvae_enc_dec_hidden"], sh["fvae_kernel_size"]
    with torch.no_grad():
        ret = {}
        weo, dict_attn, pron_attn, context = ref.dict_encoder(sd, word_tokens, dict_msg, pron_modified, sh["hidden_size"], sh["num_heads"],
                                                              sh["enc_ffn_kernel_size"])
        nonpadding = (1 - word_tokens.eq(0).to(weo.dtype))[:, :, None]
        if form is not None:
            weo = weo + sr.project(sd, form, spk)[:, None, :]                  # model.py:94
        ret.update(dict_attn=dict_attn, pron_attn=pron_attn, word_encoder_out=weo)
        dur, mel2word = ref.add_dur(sd, weo * nonpadding, mel2word, sh["dur_predictor_layers"], sh["dur_predictor_kernel"])
        ret["dur"] = dur
        x, tgt_nonpadding, mel2word = ref.expand(weo, mel2word)
        ret["mel2word"] = mel2word
        x = x * tgt_nonpadding
        ret["x_mask"] = tgt_nonpadding
        g = x.transpose(1, 2)
        x_mask = tgt_nonpadding.transpose(1, 2)
        g_sqz = F.conv1d(g, sd["fvae.g_pre_net.0.weight"], sd["fvae.g_pre_net.0.bias"], stride=4, padding=2)   # semantics = 0
        z_q, m_q, logs_q, x_mask_sqz = posterior_encoder(sd, tgt_mels.transpose(1, 2), x_mask, g_sqz, eps, Hd, kf, sh["fvae_enc_n_layers"],
                                                         sh["latent_size"])
        mel = decoder_masked(sd, z_q, x_mask, g, Hd, kf, sh["fvae_dec_n_layers"])
        z_p = prior_flow_forward(sd, z_q, x_mask_sqz, g_sqz, sh["prior_glow_n_blocks"], sh["prior_glow_hidden"], sh["glow_kernel_size"])
        ret["kl"] = kl_term(z_q, m_q, logs_q, z_p, x_mask_sqz)
        ret.update(z_p=z_p, m_q=m_q, logs_q=logs_q)
        ret["mel_out"] = ret["mel_out_fvae"] = mel.transpose(1, 2)
        return ret
