"""Deterministic synthetic weights and inputs for the Dict-TTS inference path.

No trained checkpoint, Biaobei audio or roformer gloss embeddings exist offline, so tests,
``__graft_entry__.smoke()`` and ``bench.py`` run on tensors produced here: a counter-based generator (numpy
Philox keyed by (seed, crc32(tensor name))) so that any tensor can be regenerated independently, in any
order, on any machine.  The *shapes and key names* are exactly those of the reference state dicts
(``PortaSpeech_dict`` — modules/dict_tts/model.py:14-33 — and ``HifiGanGenerator`` —
modules/hifigan/hifigan.py:100-122), including the weight-norm ``weight_g/weight_v`` pairs and the tensors
that are loaded but unused at inference (SURVEY.md §8a "Parameter inventory").

The *structure* of the batches (sentences, senses per character, gloss lengths, pinyin ids) comes from
``data/biaobei_struct.json`` (derived from the reference's data files by oracle/make_biaobei_struct.py);
batch collation follows tasks/tts/dataset_utils.py:264-330.
"""
import json
import os
import zlib

import numpy as np

HIDDEN = 192
GLOSS_DIM = 768
N_MEL = 80
N_PINYIN = 185
WORD_SIZE = 8000

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def _rng(seed, name):
    return np.random.Generator(np.random.Philox(key=[int(seed) & 0xFFFFFFFFFFFFFFFF, zlib.crc32(name.encode())]))


def randn(seed, name, shape, scale=1.0):
    return (_rng(seed, name).standard_normal(size=shape, dtype=np.float32) * np.float32(scale)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------
# state dicts
# ----------------------------------------------------------------------------------------------------------
def _conv(sd, seed, name, cout, cin, k, gain=1.0, bias=0.05, wn=False, transposed=False):
    shape = (cin, cout, k) if transposed else (cout, cin, k)
    fan_in = cin * k if not transposed else cin * max(1, k // 2)
    w = randn(seed, name + ".w", shape, gain / np.sqrt(fan_in))
    if wn:
        # weight_norm(dim=0): g has shape [shape[0],1,1]; make g != ||v|| so that folding is exercised
        nrm = np.sqrt((w.reshape(shape[0], -1) ** 2).sum(1)).reshape(shape[0], 1, 1)
        sd[name + ".weight_g"] = (nrm * (1.0 + 0.1 * randn(seed, name + ".g", (shape[0], 1, 1)))).astype(np.float32)
        sd[name + ".weight_v"] = (w * np.float32(1.7)).astype(np.float32)
    else:
        sd[name + ".weight"] = w
    sd[name + ".bias"] = randn(seed, name + ".b", (cout,), bias)


def _linear(sd, seed, name, cout, cin, gain=1.0, bias=None):
    sd[name + ".weight"] = randn(seed, name + ".w", (cout, cin), gain / np.sqrt(cin))
    if bias is not None:
        sd[name + ".bias"] = randn(seed, name + ".b", (cout,), bias)


def _ln(sd, seed, name, c, g="gamma", b="beta"):
    sd[f"{name}.{g}"] = (1.0 + 0.1 * randn(seed, name + ".g", (c,))).astype(np.float32)
    sd[f"{name}.{b}"] = randn(seed, name + ".b", (c,), 0.1)


def _rel_encoder(sd, seed, p, layers=4, h=HIDDEN, f=4 * HIDDEN, k=5):
    for i in range(layers):
        for n in "qkvo":
            _conv(sd, seed, f"{p}.attn_layers.{i}.conv_{n}", h, h, 1, gain=1.0 if n in "qk" else 0.7)
        _ln(sd, seed, f"{p}.norm_layers_1.{i}", h)
        _conv(sd, seed, f"{p}.ffn_layers.{i}.conv_1", f, h, k, gain=1.2)
        _conv(sd, seed, f"{p}.ffn_layers.{i}.conv_2", h, f, 1, gain=0.7)
        _ln(sd, seed, f"{p}.norm_layers_2.{i}", h)
    _ln(sd, seed, f"{p}.last_ln", h)


def _wn(sd, seed, p, hidden, k, layers, gin):
    for i in range(layers):
        _conv(sd, seed, f"{p}.in_layers.{i}", 2 * hidden, hidden, k, gain=1.0, wn=True)
        rs = 2 * hidden if i < layers - 1 else hidden
        _conv(sd, seed, f"{p}.res_skip_layers.{i}", rs, hidden, 1, gain=0.8, wn=True)
    _conv(sd, seed, f"{p}.cond_layer", 2 * hidden * layers, gin, 1, gain=0.7, wn=True)


SPK_EMBED_DIM = 256   # utterance speaker embeddings of use_spk_embed (modules/portaspeech/model.py:163)


def speaker_state_dict(seed=1234, speaker="embed", num_spk=4, hidden=HIDDEN):
    """seeded spk_embed_proj weights (modules/portaspeech/model.py:159-163): "embed" = nn.Linear(256, hidden) (weight + bias),
    "id" = Embedding(num_spk, hidden) (weight only).  Rows of about the size of the word encoder output's, so that speakers move
    the durations."""
    sd = {}
    if speaker == "embed":
        _linear(sd, seed, "spk_embed_proj", hidden, SPK_EMBED_DIM, gain=0.5, bias=0.1)
    elif speaker == "id":
        sd["spk_embed_proj.weight"] = randn(seed, "spk_embed_proj.table", (num_spk, hidden), 0.5)
    else:
        raise ValueError(f"speaker must be 'embed' or 'id', got {speaker!r}")
    return sd


def speaker_inputs(seed, speaker, B, num_spk=4, name="spk"):
    """seeded per-utterance speaker inputs: "embed" -> fp32 [B, 256] unit-norm embeddings (one per utterance, as the binarizer's
    resemblyzer vectors are), "id" -> int64 [B] speaker ids in [0, num_spk)"""
    if speaker == "embed":
        e = randn(seed, name + ".embed", (B, SPK_EMBED_DIM))
        return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)
    if speaker == "id":
        return _rng(seed, name + ".ids").integers(0, num_spk, size=B).astype(np.int64)
    raise ValueError(f"speaker must be 'embed' or 'id', got {speaker!r}")


# the acoustic hparams dict_tts_state_dict(acoustic=...) reads, with the defaults it draws without them (hparams.BIAOBEI_DEFAULTS; the
# prior flow's WaveNets have 4 layers, modules/dict_tts/fvae_semantics.py:77-78)
ACOUSTIC_SHAPE = {"hidden_size": HIDDEN, "num_heads": 2, "enc_ffn_kernel_size": 5, "dur_predictor_layers": 3, "dur_predictor_kernel": 5,
                  "latent_size": 16, "fvae_enc_dec_hidden": HIDDEN, "fvae_kernel_size": 5, "fvae_dec_n_layers": 4, "fvae_enc_n_layers": 8,
                  "prior_glow_hidden": 64, "glow_kernel_size": 3, "prior_glow_n_blocks": 4}


def acoustic_shape(hp=None):
    """the ACOUSTIC_SHAPE keys of hparams dict hp (others ignored), defaults filled in, as ints"""
    hp = dict(hp or {})
    return {k: int(hp.get(k, v)) for k, v in ACOUSTIC_SHAPE.items()}


def dict_tts_state_dict(seed=1234, n_phone=6, word_size=WORD_SIZE, speaker=None, num_spk=4, acoustic=None):
    """numpy state dict with the key names / shapes of ``state_dict['model']``.  speaker = "embed" / "id" (opt-in)
    adds the spk_embed_proj of a multi-speaker checkpoint (speaker_state_dict); every other tensor is the same as without it.
    acoustic: hparams (ACOUSTIC_SHAPE keys) giving the model's shape, e.g. {"hidden_size": 256, "num_heads": 4}; None or {} = the
    ps_flow.yaml shape, drawn bit for bit as before.  num_heads shapes no tensor (it is read at run time only)."""
    sh = acoustic_shape(acoustic)
    sd = {}
    h = sh["hidden_size"]
    Hd, Z, Hf = sh["fvae_enc_dec_hidden"], sh["latent_size"], sh["prior_glow_hidden"]
    # PortaSpeech leftovers: loaded, never used by PortaSpeech_dict (modules/portaspeech/model.py:153-158)
    for n in ("enc_pos_proj", "dec_query_proj", "dec_res_proj"):
        _linear(sd, seed, n, h, 2 * h, bias=0.02)
    sd["attn.in_proj_weight"] = randn(seed, "attn.in_proj_weight", (3 * h, h), h ** -0.5)
    _linear(sd, seed, "attn.out_proj", h, h)
    # duration predictor (modules/portaspeech/model.py:38-66, n_chans = 128: :164-169)
    for i in range(sh["dur_predictor_layers"]):
        _conv(sd, seed, f"dur_predictor.conv.{i}.1", 128, h if i == 0 else 128, sh["dur_predictor_kernel"], gain=1.3)
        _ln(sd, seed, f"dur_predictor.conv.{i}.3", 128, "weight", "bias")
    sd["dur_predictor.linear.0.weight"] = randn(seed, "dur.lin.w", (1, 128), 0.6 / np.sqrt(128))
    sd["dur_predictor.linear.0.bias"] = np.array([2.2], np.float32)  # ~ exp(2.3)-1 = 9 frames / word
    # FVAE (modules/dict_tts/fvae_semantics.py:61-82)
    _conv(sd, seed, "fvae.g_pre_net.0", h, h, 8, gain=1.0)
    _conv(sd, seed, "fvae.encoder.pre_net.0", Hd, N_MEL, 8)
    _wn(sd, seed, "fvae.encoder.wn", Hd, sh["fvae_kernel_size"], sh["fvae_enc_n_layers"], h)
    _conv(sd, seed, "fvae.encoder.out_proj", 2 * Z, Hd, 1)
    for f in range(0, 2 * sh["prior_glow_n_blocks"], 2):
        p = f"fvae.prior_flow.flows.{f}"
        _conv(sd, seed, p + ".pre", Hf, Z // 2, 1, gain=1.0)
        _wn(sd, seed, p + ".enc", Hf, sh["glow_kernel_size"], 4, h)
        _conv(sd, seed, p + ".post", Z // 2, Hf, 1, gain=0.5)
    _conv(sd, seed, "fvae.decoder.pre_net.0", Hd, Z, 4, gain=1.0, transposed=True)
    # ConvTranspose1d keeps a [cout] bias
    _wn(sd, seed, "fvae.decoder.wn", Hd, sh["fvae_kernel_size"], sh["fvae_dec_n_layers"], h)
    _conv(sd, seed, "fvae.decoder.out_proj", N_MEL, Hd, 1, gain=1.5)
    sd["fvae.decoder.out_proj.bias"] = (sd["fvae.decoder.out_proj.bias"] - 2.5).astype(np.float32)  # log-mel range
    # dictionary encoder (modules/dict_tts/layers/dict_encoder.py:69-128)
    p = "dict_encoder.S2PA_module"
    sd[p + ".emb.weight"] = randn(seed, p + ".emb", (n_phone, h), h ** -0.5)
    sd[p + ".word_emb.weight"] = randn(seed, p + ".word_emb", (word_size, h), h ** -0.5)
    sd[p + ".emb.weight"][0] = 0
    sd[p + ".word_emb.weight"][0] = 0
    _rel_encoder(sd, seed, p + ".semantic_encoder", h=h, f=4 * h, k=sh["enc_ffn_kernel_size"])
    a = p + ".s2pa_attention"
    _linear(sd, seed, a + ".q_transform", h, h, gain=6.0)
    _linear(sd, seed, a + ".k_transform", h, GLOSS_DIM, gain=6.0)
    _linear(sd, seed, a + ".v_transform", h, GLOSS_DIM, gain=2.0)
    _linear(sd, seed, a + ".output_transform", h, h)
    sd[a + ".pinyin_embedding.weight"] = randn(seed, a + ".pinyin", (N_PINYIN, h), 1.0)
    sd[a + ".pinyin_embedding.weight"][0] = 0
    _rel_encoder(sd, seed, p + ".linguistic_encoder", h=h, f=4 * h, k=sh["enc_ffn_kernel_size"])
    if speaker is not None:
        sd.update(speaker_state_dict(seed, speaker, num_spk, hidden=h))
    return sd


def fft_blocks_state_dict(seed=1234, hidden=HIDDEN, layers=4, kernel_size=9, use_pos_embed=True, use_last_norm=True):
    """numpy state dict of the reference's ``FFTBlocks`` (modules/fastspeech/tts_modules.py:458-493): per layer
    ``layers.i.op.{layer_norm1, self_attn.in_proj_weight, self_attn.out_proj, layer_norm2, ffn.ffn_1, ffn.ffn_2}``"""
    sd = {}
    for i in range(layers):
        p = f"layers.{i}.op"
        _ln(sd, seed, f"fft.{p}.layer_norm1", hidden, "weight", "bias")
        sd[f"{p}.layer_norm1.weight"], sd[f"{p}.layer_norm1.bias"] = sd.pop(f"fft.{p}.layer_norm1.weight"), sd.pop(f"fft.{p}.layer_norm1.bias")
        sd[f"{p}.self_attn.in_proj_weight"] = randn(seed, f"fft.{p}.in_proj", (3 * hidden, hidden), 1.0 / np.sqrt(hidden))
        sd[f"{p}.self_attn.out_proj.weight"] = randn(seed, f"fft.{p}.out_proj", (hidden, hidden), 0.7 / np.sqrt(hidden))
        _ln(sd, seed, f"fft.{p}.layer_norm2", hidden, "weight", "bias")
        sd[f"{p}.layer_norm2.weight"], sd[f"{p}.layer_norm2.bias"] = sd.pop(f"fft.{p}.layer_norm2.weight"), sd.pop(f"fft.{p}.layer_norm2.bias")
        sd[f"{p}.ffn.ffn_1.weight"] = randn(seed, f"fft.{p}.ffn_1.w", (4 * hidden, hidden, kernel_size), 1.6 / np.sqrt(hidden * kernel_size) * np.sqrt(kernel_size))
        sd[f"{p}.ffn.ffn_1.bias"] = randn(seed, f"fft.{p}.ffn_1.b", (4 * hidden,), 0.05)
        sd[f"{p}.ffn.ffn_2.weight"] = randn(seed, f"fft.{p}.ffn_2.w", (hidden, 4 * hidden), 0.7 / np.sqrt(4 * hidden))
        sd[f"{p}.ffn.ffn_2.bias"] = randn(seed, f"fft.{p}.ffn_2.b", (hidden,), 0.05)
    if use_last_norm:
        _ln(sd, seed, "fft.layer_norm", hidden, "weight", "bias")
        sd["layer_norm.weight"], sd["layer_norm.bias"] = sd.pop("fft.layer_norm.weight"), sd.pop("fft.layer_norm.bias")
    if use_pos_embed:
        sd["pos_embed_alpha"] = np.array([0.8], np.float32)
        sd["embed_positions._float_tensor"] = np.zeros(1, np.float32)
    return sd


def hifigan_config():
    """egs/egs_bases/tts/vocoder/hifigan.yaml:3-10"""
    return {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
            "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
            "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


def hifigan_config_v3():
    """the light "V3" generator of the original HifiGAN release (config_v3.json): ``resblock: "2"`` (ResBlock2,
    modules/hifigan/hifigan.py:61-89), three upsamplers (hop 256), stage widths 128 / 64 / 32"""
    return {"resblock": "2", "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8],
            "upsample_initial_channel": 256, "resblock_kernel_sizes": [3, 5, 7],
            "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]]}


def hifigan_config_v2():
    """the small "V2" generator of the original HifiGAN release (config_v2.json): ResBlock1 like V1 with
    ``upsample_initial_channel`` 128, i.e. stage widths 64 / 32 / 16 / 8 (hop 256)"""
    return {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
            "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 7, 11],
            "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


def hifigan_state_dict(seed=1234, weight_norm=True, cfg=None):
    """numpy state dict of ``HifiGanGenerator`` (``state_dict.model_gen``), weight-norm form by default."""
    cfg = cfg or hifigan_config()
    sd = {}
    c0 = cfg["upsample_initial_channel"]
    _conv(sd, seed, "conv_pre", c0, N_MEL, 7, gain=0.35, wn=weight_norm)
    ch = c0
    for i, (u, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        ch = c0 // (2 ** (i + 1))
        _conv(sd, seed, f"ups.{i}", ch, 2 * ch, k, gain=1.4, wn=weight_norm, transposed=True)
        # fan-in of a stride-u transposed conv is cin*k/u
        for key in (f"ups.{i}.weight_v", f"ups.{i}.weight"):
            if key in sd:
                sd[key] = (sd[key] * np.float32(np.sqrt(max(1, k // 2) / (k / u)))).astype(np.float32)
        if weight_norm:
            v = sd[f"ups.{i}.weight_v"]
            nrm = np.sqrt((v.reshape(v.shape[0], -1) ** 2).sum(1)).reshape(-1, 1, 1)
            sd[f"ups.{i}.weight_g"] = (nrm / 1.7 * (1.0 + 0.1 * randn(seed, f"ups.{i}.g", (v.shape[0], 1, 1)))
                                        ).astype(np.float32)
        nk = len(cfg["resblock_kernel_sizes"])
        for j, kk in enumerate(cfg["resblock_kernel_sizes"]):
            r = f"resblocks.{i * nk + j}"
            if str(cfg.get("resblock", "1")) == "2":   # ResBlock2 (modules/hifigan/hifigan.py:62-66): convs.{0,1}
                for m in range(len(cfg["resblock_dilation_sizes"][j])):
                    _conv(sd, seed, f"{r}.convs.{m}", ch, ch, kk, gain=1.0, wn=weight_norm)
                continue
            for m in range(3):
                _conv(sd, seed, f"{r}.convs1.{m}", ch, ch, kk, gain=1.0, wn=weight_norm)
                _conv(sd, seed, f"{r}.convs2.{m}", ch, ch, kk, gain=0.6, wn=weight_norm)
    _conv(sd, seed, "conv_post", 1, ch, 7, gain=0.25, wn=weight_norm)
    return sd


# MultiPeriodDiscriminator / MultiScaleDiscriminator (modules/hifigan/hifigan.py:154-298): (C_out, C_in, k, stride, groups) per convolution
DISC_PERIODS = (2, 3, 5, 7, 11)
DISC_MPD_CONVS = ((32, 1, 5, 3, 1), (128, 32, 5, 3, 1), (512, 128, 5, 3, 1), (1024, 512, 5, 3, 1), (1024, 1024, 5, 1, 1))
DISC_MSD_CONVS = ((128, 1, 15, 1, 1), (128, 128, 41, 2, 4), (256, 128, 41, 2, 16), (512, 256, 41, 4, 16), (1024, 512, 41, 4, 16),
                  (1024, 1024, 41, 1, 16), (1024, 1024, 5, 1, 1))
DISC_POST = (1, 1024, 3, 1, 1)


def _disc_conv(sd, seed, name, spec, conv2d, norm, gain):
    """one discriminator convolution in the checkpoint's form: weight_norm -> weight_g / weight_v, spectral_norm -> weight_orig /
    weight_u / weight_v (u, v from power iterations on the matrix, so that u . (W v) IS its spectral norm, as after training)."""
    cout, cin, k, _, groups = spec
    shape = (cout, cin // groups, k, 1) if conv2d else (cout, cin // groups, k)
    fan_in = (cin // groups) * k
    w = randn(seed, name + ".w", shape, gain * np.sqrt(2.0 / fan_in))
    ones = (1,) * (len(shape) - 1)
    if norm == "weight":
        nrm = np.sqrt((w.reshape(cout, -1).astype(np.float64) ** 2).sum(1)).reshape((cout,) + ones)
        sd[name + ".weight_g"] = (nrm * (1.0 + 0.1 * randn(seed, name + ".g", (cout,) + ones))).astype(np.float32)
        sd[name + ".weight_v"] = (w * np.float32(1.7)).astype(np.float32)
    else:
        m = w.reshape(cout, -1).astype(np.float64)
        v = _rng(seed, name + ".v").standard_normal(m.shape[1])
        for _ in range(8):
            u = m @ v
            u /= np.linalg.norm(u) + 1e-12
            v = m.T @ u
            v /= np.linalg.norm(v) + 1e-12
        sd[name + ".weight_orig"] = w
        sd[name + ".weight_u"] = u.astype(np.float32)
        sd[name + ".weight_v"] = v.astype(np.float32)
    sd[name + ".bias"] = randn(seed, name + ".b", (cout,), 0.05)


def hifigan_disc_state_dict(seed=1234):
    """numpy state dict of the vocoder task's ``model_disc`` (``state_dict.model_disc`` of a HifiGAN checkpoint with use_cond_disc and
    use_spec_disc off): ``mpd.discriminators.<i>`` (weight norm) and ``msd.discriminators.<i>`` (the first under spectral norm, the others
    under weight norm), He-scaled per layer.  A spectrally normalised layer has gain 1 whatever its stored scale, so the first scale
    discriminator's outputs are driven by its biases; the others keep the input's scale."""
    sd = {}
    for i in range(len(DISC_PERIODS)):
        p = f"mpd.discriminators.{i}"
        for j, spec in enumerate(DISC_MPD_CONVS):
            _disc_conv(sd, seed, f"{p}.convs.{j}", spec, True, "weight", 1.0)
        _disc_conv(sd, seed, f"{p}.conv_post", DISC_POST, True, "weight", 0.7)
    for i in range(3):
        p = f"msd.discriminators.{i}"
        norm = "spectral" if i == 0 else "weight"
        for j, spec in enumerate(DISC_MSD_CONVS):
            _disc_conv(sd, seed, f"{p}.convs.{j}", spec, False, norm, 1.0)
        _disc_conv(sd, seed, f"{p}.conv_post", DISC_POST, False, norm, 0.7)
    return sd


def voice_encoder_state_dict(seed=1234, scale=1.0):
    """numpy state dict of Resemblyzer's VoiceEncoder (``lstm = nn.LSTM(40, 256, 3, batch_first=True)``, ``linear = nn.Linear(256, 256)``)
    with torch's default initialisation, U(-1/16, 1/16) for every tensor (1 / sqrt(hidden) = 1 / sqrt(in_features)), times ``scale``"""
    sd = {}
    u = lambda name, shape: (_rng(seed, "spkenc." + name).uniform(-1.0 / 16, 1.0 / 16, size=shape) * scale).astype(np.float32)
    for k in range(3):
        sd[f"lstm.weight_ih_l{k}"] = u(f"wih{k}", (1024, 40 if k == 0 else 256))
        sd[f"lstm.weight_hh_l{k}"] = u(f"whh{k}", (1024, 256))
        sd[f"lstm.bias_ih_l{k}"] = u(f"bih{k}", (1024,))
        sd[f"lstm.bias_hh_l{k}"] = u(f"bhh{k}", (1024,))
    sd["linear.weight"] = u("lw", (256, 256))
    sd["linear.bias"] = u("lb", (256,))
    return sd


def mel_disc_state_dict(seed=1234, norm="in", hidden=128, win_num=3, reduction="stack"):
    """numpy state dict of the Dict-TTS task's ``mel_disc`` (``state_dict.mel_disc``; modules/fastspeech/multi_window_disc.py::Discriminator
    without cond_disc): per window ``discriminator.conv_layers.<w>.model.<l>.0`` (the Conv2d; under ``sn`` as weight_orig / weight_u /
    weight_v with u, v from power iterations, so that u . (W v) IS the spectral norm), ``model.<l>.3`` (l = 1, 2: InstanceNorm2d's affine
    under ``in``; BatchNorm2d's affine and running statistics under ``bn``) and ``adv_layer``.  He-scaled; affine scales lie around 1, so
    that no channel is dead."""
    if norm not in ("in", "bn", "sn"):
        raise ValueError(f"norm = {norm!r} (supported: 'in', 'bn', 'sn')")
    if reduction not in ("stack", "sum", "none"):
        raise ValueError(f"reduction = {reduction!r} (supported: 'stack', 'sum', 'none')")
    H = int(hidden)
    sd = {}
    for w, win in enumerate((32, 64, 128)[:win_num]):
        base = f"discriminator.conv_layers.{w}"
        for l in range(3):
            name = f"{base}.model.{l}.0"
            cin = H if l else 1
            wt = randn(seed, name + ".w", (H, cin, 3, 3), np.sqrt(2.0 / (cin * 9)))
            if norm == "sn":
                m = wt.reshape(H, -1).astype(np.float64)
                v = _rng(seed, name + ".v").standard_normal(m.shape[1])
                for _ in range(8):
                    u = m @ v
                    u /= np.linalg.norm(u) + 1e-12
                    v = m.T @ u
                    v /= np.linalg.norm(v) + 1e-12
                sd[name + ".weight_orig"] = wt
                sd[name + ".weight_u"] = u.astype(np.float32)
                sd[name + ".weight_v"] = v.astype(np.float32)
            else:
                sd[name + ".weight"] = wt
            sd[name + ".bias"] = randn(seed, name + ".b", (H,), 0.05)
            if l and norm in ("in", "bn"):
                n = f"{base}.model.{l}.3"
                sd[n + ".weight"] = (1.0 + 0.1 * randn(seed, n + ".g", (H,))).astype(np.float32)
                sd[n + ".bias"] = randn(seed, n + ".beta", (H,), 0.05)
                if norm == "bn":
                    sd[n + ".running_mean"] = randn(seed, n + ".rm", (H,), 0.1)
                    sd[n + ".running_var"] = (0.5 + _rng(seed, n + ".rv").random(H)).astype(np.float32)
                    sd[n + ".num_batches_tracked"] = np.array(1000, np.int64)
        n_in = H * 10 * (1 if reduction == "none" else win // 8)
        sd[f"{base}.adv_layer.weight"] = randn(seed, base + ".adv.w", (1, n_in), 1.0 / np.sqrt(n_in))
        sd[f"{base}.adv_layer.bias"] = randn(seed, base + ".adv.b", (1,), 0.05)
    return sd


# ----------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------
_STRUCT = None


def biaobei_struct():
    global _STRUCT
    if _STRUCT is None:
        with open(os.path.join(_DATA, "biaobei_struct.json")) as f:
            d = json.load(f)
        d["entries"] = {int(k): v for k, v in d["entries"].items()}
        _STRUCT = d
    return _STRUCT


_FULL = None


def zh_dict_struct():
    """sense structure of ALL 7,030 zh-dict.json characters (oracle/make_biaobei_struct.py:write_full_dictionary):
    {'n_entries', 'entries': word id (3 + rank) -> [[gloss_tokens, pinyin_initial_id, pinyin_final_id], ...]} — the table
    of BASELINE.json configs[4] ("word_size=8000, full zh-dict.json entry set in HBM")"""
    global _FULL
    if _FULL is None:
        with open(os.path.join(_DATA, "zh_dict_struct.json")) as f:
            d = json.load(f)
        d["entries"] = {int(k): v for k, v in d["entries"].items()}
        _FULL = d
    return _FULL


BOS_ID, EOS_ID = 1203, 1204  # any ids >= 3 outside the char range; '<BOS>'/'<EOS>' are ordinary vocabulary words


def config5_sentences(n=128, seed=55, entries=None):
    """BASELINE.json configs[4] / SURVEY §8d 'Config 5': n mixed-length utterances, T_w ~ U{6..60} characters drawn from the WHOLE
    dictionary with the heteronyms (>= 2 pronunciations) over-sampled x5; the first / last table rows appear.  -> list of id lists"""
    ent = entries if entries is not None else zh_dict_struct()["entries"]
    rng = np.random.default_rng(seed)
    ids = np.array(sorted(ent))
    wts = np.array([5.0 if len(ent[i]) > 1 else 1.0 for i in ids])
    wts /= wts.sum()
    sents = [rng.choice(ids, size=int(rng.integers(6, 61)), p=wts).tolist() for _ in range(n)]
    sents[0][0], sents[1][-1] = int(ids[0]), int(ids[-1])
    return sents


def dict_entry(word_id, seed=1234, entries=None):
    """One ``dict_embed`` item (binarizer_zh.py:301-309): key/value [L,768] (same content), key_map [L],
    pinyin [P], pinyin_map [P]."""
    entries = biaobei_struct()["entries"] if entries is None else entries
    senses = entries[word_id]
    if senses[0][2] < 0:  # char absent from the dictionary: zero entry (binarizer_zh.py:250-259)
        return (np.zeros((3, GLOSS_DIM), np.float32), np.array([0, 1, 0], np.float32),
                np.array([0], np.int64), np.array([1], np.int64))
    L = sum(s[0] for s in senses)
    emb = randn(seed, f"gloss.{word_id}", (L, GLOSS_DIM), 0.5)
    key_map, pinyin, pinyin_map = [], [], []
    for i, (n, ini, fin) in enumerate(senses):
        key_map += [0] + [i + 1] * (n - 2) + [0]
        pinyin += [ini, fin]
        pinyin_map += [i + 1, i + 1]
    return emb, np.array(key_map, np.float32), np.array(pinyin, np.int64), np.array(pinyin_map, np.int64)


def make_batch(sentences, seed=1234, entries=None, pron_every=7):
    """Collate sentences (lists of word ids, without BOS/EOS) the way DictTTSDataset.collater does
    (tasks/tts/dataset_utils.py:264-302).  Returns a dict of numpy arrays:
    word_tokens [B,T_w] i64, keys/values [B,T_w,L_k,768] f32, key_map [B,T_w,L_k] f32, pinyin [B,T_w,P] i64,
    pinyin_map [B,T_w,P] i64, pron_modified [B,T_w] i64."""
    B = len(sentences)
    items = [[dict_entry(w, seed, entries) for w in s] for s in sentences]
    Tw = max(len(s) for s in sentences) + 2
    Lk = max(e[0].shape[0] for it in items for e in it)
    P = max(e[2].shape[0] for it in items for e in it)
    word_tokens = np.zeros((B, Tw), np.int64)
    keys = np.zeros((B, Tw, Lk, GLOSS_DIM), np.float32)
    key_map = np.zeros((B, Tw, Lk), np.float32)
    pinyin = np.zeros((B, Tw, P), np.int64)
    pinyin_map = np.zeros((B, Tw, P), np.int64)
    pron_modified = np.zeros((B, Tw), np.int64)
    n_multi = 0
    for b, (s, it) in enumerate(zip(sentences, items)):
        word_tokens[b, :len(s) + 2] = [BOS_ID] + list(s) + [EOS_ID]
        for t, (emb, km, py, pm) in enumerate(it):
            keys[b, t + 1, :emb.shape[0]] = emb
            key_map[b, t + 1, :km.shape[0]] = km
            pinyin[b, t + 1, :py.shape[0]] = py
            pinyin_map[b, t + 1, :pm.shape[0]] = pm
            if pm.max() >= 2:
                n_multi += 1
                if pron_every and n_multi % pron_every == 0:
                    pron_modified[b, t + 1] = 2  # sandhi-forced sense (sandhi_processor.py:447-483)
    # F.pad(..., value=1) on the word axis: first and LAST row of the padded batch (dataset_utils.py:288-300)
    key_map[:, 0, :] = 1
    key_map[:, -1, :] = 1
    pinyin_map[:, 0, :] = 1
    pinyin_map[:, -1, :] = 1
    return {"word_tokens": word_tokens, "keys": keys, "values": keys.copy(), "key_map": key_map, "pinyin": pinyin,
            "pinyin_map": pinyin_map, "pron_modified": pron_modified}


def biaobei_batch(first=0, count=60, seed=1234):
    st = biaobei_struct()
    return make_batch(st["sentences"][first:first + count], seed)


def teacher_mel2word(word_tokens, frames_per_char=22, frames_edge=11):
    """Teacher-forced mel2word: 22 frames / char, 11 for BOS/EOS; [B,T] i64, 0 = padding."""
    rows = []
    for wt in word_tokens:
        n = int((wt > 0).sum())
        d = [frames_edge] + [frames_per_char] * (n - 2) + [frames_edge]
        rows.append(np.repeat(np.arange(1, n + 1), d))
    T = max(len(r) for r in rows)
    out = np.zeros((len(rows), T), np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def noise(seed, B, T4, name="z_p"):
    """prior sample z_p [B,16,T_mel/4] (fvae_semantics.py:110-111), injected explicitly."""
    return randn(seed, name, (B, 16, T4))


def random_mel(seed, T, name="mel"):
    """a log-mel-like [T,80] array in roughly [-6, 1.5] (base.yaml:59-60)"""
    m = randn(seed, name, (T, N_MEL), 1.2) - 3.0
    # smooth along time so that it resembles a spectrogram rather than white noise
    m[1:] = 0.6 * m[1:] + 0.4 * m[:-1]
    return np.clip(m, -6.0, 1.5).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------
# resident dictionary table: the ragged form of the reference's ``dict_embed`` indexed dataset
# ----------------------------------------------------------------------------------------------------------
def dict_table(seed=1234, entries=None):
    """-> dict(ids, tok_off, keys, key_map, pin_off, pinyin, pinyin_map, L, P): every entry of the structure file, in
    ascending word-id order; ``ids[word_id]`` is the table row of a word."""
    entries = biaobei_struct()["entries"] if entries is None else entries
    order = sorted(entries)
    ids = {w: i for i, w in enumerate(order)}
    items = [dict_entry(w, seed, entries) for w in order]
    tok_off = np.zeros(len(order) + 1, np.int32)
    pin_off = np.zeros(len(order) + 1, np.int32)
    for i, (emb, km, py, pm) in enumerate(items):
        tok_off[i + 1] = tok_off[i] + emb.shape[0]
        pin_off[i + 1] = pin_off[i] + py.shape[0]
    return {"ids": ids, "tok_off": tok_off, "pin_off": pin_off,
            "keys": np.concatenate([it[0] for it in items]), "key_map": np.concatenate([it[1] for it in items]),
            "pinyin": np.concatenate([it[2] for it in items]), "pinyin_map": np.concatenate([it[3] for it in items]),
            "L": np.diff(tok_off), "P": np.diff(pin_off)}


def make_id_batch(sentences, table, pron_every=7):
    """the id-only form of make_batch(): word_tokens [B,T_w] i64, entry_ids [B,T_w] i32 (-1 BOS / last row, -2 batch
    padding), pron_modified [B,T_w] i64 and the batch maxima L_k, P the collated tensors would have"""
    B = len(sentences)
    Tw = max(len(s) for s in sentences) + 2
    word_tokens = np.zeros((B, Tw), np.int64)
    entry = np.full((B, Tw), -2, np.int32)
    pron_modified = np.zeros((B, Tw), np.int64)
    L_k, P, n_multi = 1, 1, 0
    for b, s in enumerate(sentences):
        word_tokens[b, :len(s) + 2] = [BOS_ID] + list(s) + [EOS_ID]
        for t, w in enumerate(s):
            e = table["ids"][w]
            entry[b, t + 1] = e
            L_k, P = max(L_k, int(table["L"][e])), max(P, int(table["P"][e]))
            if table["pinyin_map"][table["pin_off"][e]:table["pin_off"][e + 1]].max() >= 2:
                n_multi += 1
                if pron_every and n_multi % pron_every == 0:
                    pron_modified[b, t + 1] = 2
    entry[:, 0] = -1
    entry[:, -1] = -1
    return {"word_tokens": word_tokens, "entry_ids": entry, "pron_modified": pron_modified, "L_k": L_k, "P": P}


# ----------------------------------------------------------------------------------------------------------
# the PortaSpeech baseline (modules/portaspeech/model.py::PortaSpeech, dur_level: word)
# ----------------------------------------------------------------------------------------------------------
PS_N_PHONE = 64      # rows of the phoneme embedding (len(dictionary)); row 0 is padding
PS_WINDOW = 4        # TextEncoder's window_size (model.py:79)


def portaspeech_state_dict(seed=1234, n_phone=PS_N_PHONE, acoustic=None, word_enc_layers=4, enc_layers=4, window=PS_WINDOW):
    """numpy state dict with the key names / shapes of the baseline's ``state_dict['model']``.  acoustic: ACOUSTIC_SHAPE keys, as for
    dict_tts_state_dict.  The prenet's ``proj`` is NON-zero (the reference initialises it to zero, which would hide the prenet), and the
    duration head is scaled so that a word of 1 .. 3 phonemes gets roughly 0 .. 30 frames (the per-phoneme durations are summed per word
    BEFORE exp(.) - 1)."""
    sh = acoustic_shape(acoustic)
    sd = {}
    h, heads = sh["hidden_size"], sh["num_heads"]
    Hd, Z, Hf = sh["fvae_enc_dec_hidden"], sh["latent_size"], sh["prior_glow_hidden"]
    p = "ph_encoder"
    sd[p + ".emb.weight"] = randn(seed, "ps.emb", (n_phone, h), h ** -0.5)
    sd[p + ".emb.weight"][0] = 0
    for i in range(3):
        _conv(sd, seed, f"{p}.pre.conv_layers.{i}", h, h, 5, gain=1.2)
        _ln(sd, seed, f"{p}.pre.norm_layers.{i}", h)
    _conv(sd, seed, f"{p}.pre.proj", h, h, 1, gain=0.5)
    dk = h // heads
    for i in range(enc_layers):
        for n in "qkvo":
            _conv(sd, seed, f"{p}.encoder.attn_layers.{i}.conv_{n}", h, h, 1, gain=1.0 if n in "qk" else 0.7)
        sd[f"{p}.encoder.attn_layers.{i}.emb_rel_k"] = randn(seed, f"ps.rel_k.{i}", (1, 2 * window + 1, dk), 2.0 * dk ** -0.5)
        sd[f"{p}.encoder.attn_layers.{i}.emb_rel_v"] = randn(seed, f"ps.rel_v.{i}", (1, 2 * window + 1, dk), 2.0 * dk ** -0.5)
        _ln(sd, seed, f"{p}.encoder.norm_layers_1.{i}", h)
        _conv(sd, seed, f"{p}.encoder.ffn_layers.{i}.conv_1", 4 * h, h, sh["enc_ffn_kernel_size"], gain=1.2)
        _conv(sd, seed, f"{p}.encoder.ffn_layers.{i}.conv_2", h, 4 * h, 1, gain=0.7)
        _ln(sd, seed, f"{p}.encoder.norm_layers_2.{i}", h)
    for k, v in fft_blocks_state_dict(seed + 1, hidden=h, layers=word_enc_layers, kernel_size=1).items():
        sd["word_encoder." + k] = v
    for n in ("enc_pos_proj", "dec_query_proj", "dec_res_proj"):
        _linear(sd, seed, "ps." + n, h, 2 * h, gain=1.4, bias=0.02)
        sd[n + ".weight"], sd[n + ".bias"] = sd.pop(f"ps.{n}.weight"), sd.pop(f"ps.{n}.bias")
    sd["attn.in_proj_weight"] = randn(seed, "ps.attn.in_proj_weight", (3 * h, h), 2.0 * h ** -0.5)
    sd["attn.out_proj.weight"] = randn(seed, "ps.attn.out_proj", (h, h), h ** -0.5)
    for i in range(sh["dur_predictor_layers"]):
        _conv(sd, seed, f"dur_predictor.conv.{i}.1", 128, h if i == 0 else 128, sh["dur_predictor_kernel"], gain=1.3)
        _ln(sd, seed, f"dur_predictor.conv.{i}.3", 128, "weight", "bias")
    sd["dur_predictor.linear.0.weight"] = randn(seed, "ps.dur.lin.w", (1, 128), 0.5 / np.sqrt(128))
    sd["dur_predictor.linear.0.bias"] = np.array([0.35], np.float32)   # softplus ~ 0.9 per phoneme: exp(0.9 n) - 1 frames for n phonemes
    _conv(sd, seed, "fvae.g_pre_net.0", h, h, 8, gain=1.0)
    _conv(sd, seed, "fvae.encoder.pre_net.0", Hd, N_MEL, 8)
    _wn(sd, seed, "fvae.encoder.wn", Hd, sh["fvae_kernel_size"], sh["fvae_enc_n_layers"], h)
    _conv(sd, seed, "fvae.encoder.out_proj", 2 * Z, Hd, 1)
    for f in range(0, 2 * sh["prior_glow_n_blocks"], 2):
        q = f"fvae.prior_flow.flows.{f}"
        _conv(sd, seed, q + ".pre", Hf, Z // 2, 1, gain=1.0)
        _wn(sd, seed, q + ".enc", Hf, sh["glow_kernel_size"], 4, h)
        _conv(sd, seed, q + ".post", Z // 2, Hf, 1, gain=0.5)
    _conv(sd, seed, "fvae.decoder.pre_net.0", Hd, Z, 4, gain=1.0, transposed=True)
    _wn(sd, seed, "fvae.decoder.wn", Hd, sh["fvae_kernel_size"], sh["fvae_dec_n_layers"], h)
    _conv(sd, seed, "fvae.decoder.out_proj", N_MEL, Hd, 1, gain=1.5)
    sd["fvae.decoder.out_proj.bias"] = (sd["fvae.decoder.out_proj.bias"] - 2.5).astype(np.float32)
    return sd


def portaspeech_batch(words, seed=1234, n_phone=PS_N_PHONE, T_ph=None, T_w=None):
    """words: per utterance the list of phonemes per word (each >= 1), e.g. [[2, 1, 3], [1]] -> the collated inputs of the baseline:
    txt_tokens [B, T_ph] i64 in [1, n_phone) (0 = padding), ph2word [B, T_ph] i64 (1-based, 0 = padding), word_len [B] i64.
    T_ph / T_w: pad the phoneme axis / report a wider word axis (the same utterance inside a wider batch)."""
    B = len(words)
    n_ph = [int(sum(w)) for w in words]
    T_ph = max(n_ph) if T_ph is None else int(T_ph)
    assert T_ph >= max(n_ph) and all(min(w) >= 1 for w in words)
    txt = np.zeros((B, T_ph), np.int64)
    ph2word = np.zeros((B, T_ph), np.int64)
    for b, w in enumerate(words):
        txt[b, :n_ph[b]] = _rng(seed, f"ps.tokens.{b}.{n_ph[b]}").integers(1, n_phone, size=n_ph[b])
        ph2word[b, :n_ph[b]] = np.repeat(np.arange(1, len(w) + 1), w)
    word_len = np.array([len(w) for w in words], np.int64)
    assert T_w is None or T_w >= word_len.max()
    return {"txt_tokens": txt, "ph2word": ph2word, "word_len": word_len, "T_w": int(word_len.max() if T_w is None else T_w)}


def portaspeech_words(first=0, count=60, seed=1234, max_ph=3):
    """phonemes per word for ``count`` Biaobei sentences from ``first``: every word (BOS / EOS included) gets 1 .. max_ph phonemes, seeded"""
    st = biaobei_struct()
    out = []
    for i, s in enumerate(st["sentences"][first:first + count]):
        out.append(_rng(seed, f"ps.words.{first + i}").integers(1, max_ph + 1, size=len(s) + 2).tolist())
    return out


def ps_spread_mel2word(words, frames):
    """teacher-forced mel2word giving utterance b exactly frames[b] frames spread as evenly as possible over its words (the first words
    take the remainder; frames[b] < its word count leaves the last words without frames): [B, max(frames)] int64, 0 = padding"""
    rows = []
    for w, n_f in zip(words, frames):
        n = len(w)
        d = np.full(n, n_f // n)
        d[:n_f % n] += 1
        rows.append(np.repeat(np.arange(1, n + 1), d))
    out = np.zeros((len(rows), max(len(r) for r in rows)), np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out
