"""Restatement of the PortaSpeech baseline's ``forward(infer=True)`` (modules/portaspeech/model.py::PortaSpeech, dur_level: word, no
speakers, no post-glow) in torch on the CPU, written from its formulas, in the dtype of the state dict it is given: float64 is the
reference the GPU is compared with, float32 gives the error of one float32-class computation against it (test infrastructure).

The FVAE from ``g`` on, the duration predictor and the length regulator are the oracle's pieces (oracle/dict_tts_ref.py), the word
encoder is tests/fft_ref.forward with FFN kernel 1; everything in front of them is restated here:

  phoneme encoder   emb * sqrt(H); prenet 3 x (conv5(x * mask) -> channel LayerNorm(eps 1e-4) -> ReLU), (x_org + proj(x)) * mask;
                    post-LN layers x = LN1(x * mask + attn), x = LN2(x + FFN(x)); relative attention with the shared tables
                    Ek, Ev [2 w + 1, d_k]: s_ij = (q_i.k_j + [|j-i| <= w] q_i.Ek[j-i+w]) / sqrt(d_k), keys >= len at -1e4,
                    o_i = sum_j p_ij v_j + sum_{|j-i| <= w} p_ij Ev[j-i+w]; output * (txt > 0)
  words             word_in = per-word mean (scatter-add in ascending t / clamp(count, 1)); durations per phoneme summed per word;
                    frames clamp(round(exp(dur) - 1), 0) over the first #live-phonemes words, all-zero -> ones
  positions         pos = (rank within the word) / (size of the word), 0 for word 0; [sin(pos f_i), cos(pos f_i)],
                    f_i = exp(-i ln 1e4 / (H/2 - 1))
  frame attention   one head without biases, every frame over the phonemes of its own word (-1e9 elsewhere)

``defect=`` plants ONE defect (DEFECTS); tests/test_portaspeech_cpu.py proves that each exceeds the GPU gate at its least sensitive shape.
"""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

import fft_ref
from dict_tts_amd import fft as _fft
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref
from oracle import hifigan_ref as href

SEED = 1234
WINDOW = synth.PS_WINDOW
GLOW_LAYERS = 4
GATE = 8.0   # max|gpu - f64| <= GATE * max|f32 restatement - f64|: the project's margin for two float32-class computations that differ in
             # summation order (tests/test_gloss_gpu.py)
DEFECTS = ("band_off_by_one",   # the band logit / value of offset m is taken from table row m + 1
           "ev_dropped",        # o_i lacks the sum over Ev
           "pos_rank_minus_1",  # position (rank - 1) / size instead of rank / size
           "mean_is_sum")       # the word pooling sums instead of averaging
KEYS = ("ph_encoder_out", "word_encoder_out", "dur", "decoder_inp", "attn")


def state(sd_np, dtype=torch.float32):
    """numpy state dict -> folded torch state dict in `dtype`"""
    return href.fold_weight_norm({k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in sd_np.items()})


def _cln(x, g, b, eps=1e-4):
    """channel LayerNorm of [B, C, T] with the biased variance (rel_transformer_encoder.py:261-279)"""
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * g[None, :, None] + b[None, :, None]


def rel_attention(q, k, v, ek, ev, lens, window=WINDOW, defect=None):
    """q, k, v [B, h, T, dk]; ek, ev [2 w + 1, dk]; lens [B] -> [B, h, T, dk], by the band formula"""
    B, h, T, dk = q.shape
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    rel = j - i + window                                   # [T, T]
    band = (rel >= 0) & (rel <= 2 * window)
    idx = rel.clamp(0, 2 * window)
    if defect == "band_off_by_one":
        idx = (rel + 1).clamp(0, 2 * window)
    scores = q @ k.transpose(-1, -2) / math.sqrt(dk)
    R = q @ ek.t()                                         # [B, h, T, 2 w + 1]
    local = torch.gather(R, -1, idx[None, None].expand(B, h, T, T)) * band.to(q.dtype)
    scores = scores + local / math.sqrt(dk)
    live = (torch.arange(T)[None] < torch.as_tensor(lens)[:, None])            # [B, T]
    mask = live[:, None, :, None] & live[:, None, None, :]
    scores = scores.masked_fill(~mask, -1e4)
    p = torch.softmax(scores, dim=-1)
    out = p @ v
    if defect != "ev_dropped":
        pb = p * band.to(p.dtype)
        W = torch.zeros(B, h, T, 2 * window + 1, dtype=p.dtype)
        W.scatter_add_(-1, idx[None, None].expand(B, h, T, T), pb)
        out = out + W @ ev
    return out


def ph_encoder(sd, txt, hidden, heads, window=WINDOW, defect=None, p="ph_encoder"):
    """TextEncoder.forward (model.py:119-130) -> [B, T, H], already * (txt > 0)"""
    dt = sd[p + ".emb.weight"].dtype
    lens = (txt > 0).sum(-1)
    T = txt.shape[1]
    mask = (torch.arange(T)[None] < lens[:, None]).to(dt)[:, None, :]          # [B, 1, T]
    x = (sd[p + ".emb.weight"][txt] * math.sqrt(hidden)).transpose(1, 2)
    x_org = x
    for i in range(3):
        x = F.conv1d(x * mask, sd[f"{p}.pre.conv_layers.{i}.weight"], sd[f"{p}.pre.conv_layers.{i}.bias"], padding=2)
        x = torch.relu(_cln(x, sd[f"{p}.pre.norm_layers.{i}.gamma"], sd[f"{p}.pre.norm_layers.{i}.beta"]))
    x = (x_org + F.conv1d(x, sd[p + ".pre.proj.weight"], sd[p + ".pre.proj.bias"])) * mask
    n_layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith(p + ".encoder.attn_layers."))
    B = x.shape[0]
    dk = hidden // heads
    for i in range(n_layers):
        a, f = f"{p}.encoder.attn_layers.{i}", f"{p}.encoder.ffn_layers.{i}"
        x = x * mask
        q, k, v = (F.conv1d(x, sd[f"{a}.conv_{n}.weight"], sd[f"{a}.conv_{n}.bias"]).view(B, heads, dk, T).transpose(2, 3) for n in "qkv")
        o = rel_attention(q, k, v, sd[a + ".emb_rel_k"][0], sd[a + ".emb_rel_v"][0], lens, window, defect)
        o = o.transpose(2, 3).reshape(B, hidden, T)
        y = F.conv1d(o, sd[a + ".conv_o.weight"], sd[a + ".conv_o.bias"])
        x = _cln(x + y, sd[f"{p}.encoder.norm_layers_1.{i}.gamma"], sd[f"{p}.encoder.norm_layers_1.{i}.beta"])
        K = sd[f + ".conv_1.weight"].shape[-1]
        y = torch.relu(F.conv1d(x * mask, sd[f + ".conv_1.weight"], sd[f + ".conv_1.bias"], padding=K // 2))
        y = F.conv1d(y * mask, sd[f + ".conv_2.weight"], sd[f + ".conv_2.bias"]) * mask
        x = _cln(x + y, sd[f"{p}.encoder.norm_layers_2.{i}.gamma"], sd[f"{p}.encoder.norm_layers_2.{i}.beta"])
    x = (x * mask).transpose(1, 2)
    return x * (txt > 0).to(dt)[:, :, None]


def segment_mean(hid, seg, T_w, defect=None):
    """group_hidden_by_segs (modules/portaspeech/utils.py): [B, T, H], seg [B, T] in 0 .. T_w -> [B, T_w, H]"""
    B, T, H = hid.shape
    s = hid.new_zeros(B, T_w + 1, H).scatter_add_(1, seg[:, :, None].expand(B, T, H), hid)[:, 1:]
    if defect == "mean_is_sum":
        return s
    cnt = hid.new_zeros(B, T_w + 1).scatter_add_(1, seg, hid.new_ones(B, T))[:, 1:]
    return s / cnt.clamp(min=1)[:, :, None]


def positions(x2word, T_w, dtype, defect=None):
    """build_pos_embed's scalar (model.py:359-363): [B, T] word ids in 0 .. T_w -> rank within the word / size of the word, 0 for word 0;
    words need not be contiguous"""
    w = torch.arange(1, T_w + 1)[None, :, None]
    m = (w == x2word[:, None, :]).to(dtype)                # [B, T_w, T]
    rank = m.cumsum(-1)
    if defect == "pos_rank_minus_1":
        rank = rank - 1
    return (rank / m.sum(-1).clamp(min=1)[..., None] * m).sum(1)


def sin_pos(pos, hidden):
    half = hidden // 2
    f = torch.exp(torch.arange(half, dtype=pos.dtype) * -(math.log(10000) / (half - 1)))
    e = pos[:, :, None] * f[None, None, :]
    return torch.cat([e.sin(), e.cos()], -1)


def frame_attention(sd, ph_out, enc_pos, weo, dec_pos, mel2word, ph2word):
    """attention (model.py:278-288) -> x [B, T_mel, H] (before the frame mask), weights [B, T_mel, T_ph]"""
    H = ph_out.shape[-1]
    lin = lambda n, x: F.linear(x, sd[n + ".weight"], sd[n + ".bias"])
    kv = lin("enc_pos_proj", torch.cat([ph_out, enc_pos], -1))
    e = torch.gather(F.pad(weo, [0, 0, 1, 0]), 1, mel2word[:, :, None].expand(-1, -1, H))
    cat = torch.cat([e, dec_pos], -1)
    q_in, x_res = lin("dec_query_proj", cat), lin("dec_res_proj", cat)
    Wq, Wk, Wv = sd["attn.in_proj_weight"].split(H, 0)
    q = F.linear(q_in, Wq) * H ** -0.5
    k, v = F.linear(kv, Wk), F.linear(kv, Wv)
    same = (mel2word[:, :, None] == ph2word[:, None, :]).to(q.dtype)
    w = torch.softmax(q @ k.transpose(1, 2) + (1 - same) * -1e9, dim=-1)
    return F.linear(w @ v, sd["attn.out_proj.weight"]) + x_res, w


def forward(sd, hp, txt, ph2word, T_w, mel2word=None, z_p=None, defect=None, pos_table=None, decode=True):
    """PortaSpeech.forward(infer=True) at the shape of hparams hp in the dtype of sd.  txt, ph2word [B, T_ph] int64; T_w = word_len.max();
    z_p [B, latent, T_mel / 4] or a callable (B, T4) -> tensor.  -> the reference's keys (+ 'mel2word', 'attn_live': attn with the
    rows of frames without a word zeroed, which is what the library returns)"""
    assert defect is None or defect in DEFECTS, defect
    sh = synth.acoustic_shape(hp)
    H, heads = sh["hidden_size"], sh["num_heads"]
    dt = sd["fvae.decoder.out_proj.weight"].dtype
    with torch.no_grad():
        ret = {}
        ph_out = ph_encoder(sd, txt, H, heads, int((hp or {}).get("ps_window_size", WINDOW)), defect)
        ret["ph_encoder_out"] = ph_out
        word_in = segment_mean(ph_out, ph2word, T_w, defect)
        wsd = {k[len("word_encoder."):]: v for k, v in sd.items() if k.startswith("word_encoder.")}
        if pos_table is None:
            pos_table = _fft.sinusoid_table(max(_fft.DEFAULT_MAX_TARGET_POSITIONS, T_w + 1), H, 0)
        weo = fft_ref.forward(wsd, word_in, None, heads, 1, pos_table=pos_table.to(dt))
        ret["word_encoder_out"] = weo
        src_padding = ph_out.abs().sum(-1) == 0
        dur_ph = ref.duration_predictor(sd, ph_out, src_padding, sh["dur_predictor_layers"], sh["dur_predictor_kernel"])
        dur = dur_ph.new_zeros(dur_ph.shape[0], T_w + 1).scatter_add_(1, ph2word, dur_ph)[:, 1:]
        ret["dur"] = dur
        if mel2word is None:
            d = torch.clamp(torch.round(dur.exp() - 1), min=0).long()
            mel2word = ref.length_regulator(d, (1 - src_padding.long()).sum(-1))
        fm = 4
        if mel2word.shape[1] % fm:
            mel2word = torch.cat([mel2word] + [mel2word[:, -1:]] * (fm - mel2word.shape[1] % fm), -1)
        ret["mel2word"] = mel2word
        nonpad = (mel2word > 0).to(dt)[:, :, None]
        enc_pos = sin_pos(positions(ph2word, T_w, dt, defect), H)
        dec_pos = sin_pos(positions(mel2word, T_w, dt, defect), H)
        x, w = frame_attention(sd, ph_out, enc_pos, weo, dec_pos, mel2word, ph2word)
        ret["attn"] = w
        ret["attn_live"] = w * nonpad
        ret["x_mask"] = nonpad
        ret["decoder_inp"] = x * nonpad
        if not decode:
            return ret
        g = ret["decoder_inp"].transpose(1, 2)
        if callable(z_p):
            z_p = z_p(g.shape[0], g.shape[2] // 4)
        z_p = z_p.to(dt)
        g_sqz = F.conv1d(g, sd["fvae.g_pre_net.0.weight"], sd["fvae.g_pre_net.0.bias"], stride=4, padding=2)
        z = ref.prior_flow_reverse(sd, z_p, g_sqz, sh["prior_glow_n_blocks"], sh["prior_glow_hidden"], sh["glow_kernel_size"], GLOW_LAYERS)
        y = F.conv_transpose1d(z, sd["fvae.decoder.pre_net.0.weight"], sd["fvae.decoder.pre_net.0.bias"], stride=4)
        y = ref.wn(sd, "fvae.decoder.wn", y, g, sh["fvae_enc_dec_hidden"], sh["fvae_kernel_size"], sh["fvae_dec_n_layers"])
        ret["mel_out"] = F.conv1d(y, sd["fvae.decoder.out_proj.weight"], sd["fvae.decoder.out_proj.bias"]).transpose(1, 2)
        return ret


def min_half_distance(dur, lens_w):
    """the smallest distance of exp(dur) - 1 from a half-integer over the words the length regulator reads (float64)"""
    d = np.exp(np.asarray(dur, np.float64)) - 1
    best = np.inf
    for b, n in enumerate(lens_w):
        v = d[b, :int(n)]
        if v.size:
            best = min(best, float(np.abs(v - np.floor(v) - 0.5).min()))
    return best


def row_err(got, want):
    """max |got - want| over everything, in float64"""
    g = np.asarray(got.detach().cpu() if hasattr(got, "detach") else got, np.float64)
    w = np.asarray(want.detach().cpu() if hasattr(want, "detach") else want, np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    return float(np.abs(g - w).max()) if g.size else 0.0


def gate_check(case, what, got, f32, f64, fails, rows=None):
    """max|got - f64| <= GATE * max|f32 - f64| per output, printed as one PSMEAS line; rows: an index applied to all three"""
    if rows is not None:
        got, f32, f64 = got[rows], f32[rows], f64[rows]
    e, base = row_err(got, f64), row_err(f32, f64)
    ratio = e / base if base > 0 else (0.0 if e == 0 else float("inf"))
    print("PSMEAS " + json.dumps({"case": case, "what": what, "err": e, "f32_err": base, "ratio": ratio}), flush=True)
    if e > GATE * base:
        fails.append(f"{case} {what}: |gpu - f64| = {e:.3g} > {GATE:g} x |f32 - f64| = {GATE * base:.3g}")
    return ratio
