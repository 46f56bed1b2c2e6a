"""Configuration for the MI355X path: reads the SAME YAML chains / checkpoint config the reference reads.

Mirrors the subset of ``utils/hparams.py:25-126`` the inference path needs: ``base_config`` inheritance (a
string or a list; entries starting with '.' are relative to the including file, others to the working
directory), the saved ``checkpoints/<exp>/config.yaml`` layered on top, and ``--hparams=k=v,...`` overrides
with the reference's typing rule.  ``hparams`` is a module-level dict, as in the reference, so the vocoder
plugin can be constructed with no arguments (vocoders/base_vocoder.py:15-23).
"""
import os

import yaml

hparams = {}


def _override(old, new):
    for k, v in new.items():
        if isinstance(v, dict) and isinstance(old.get(k), dict):
            _override(old[k], v)
        else:
            old[k] = v


def load_config_chain(config_fn, _seen=None):
    seen = set() if _seen is None else _seen
    if not os.path.exists(config_fn):
        return {}
    with open(config_fn) as f:
        cur = yaml.safe_load(f) or {}
    seen.add(config_fn)
    out = {}
    bases = cur.get("base_config", [])
    if not isinstance(bases, list):
        bases = [bases]
    for c in bases:
        if c.startswith("."):
            c = os.path.normpath(os.path.join(os.path.dirname(config_fn), c))
        if c not in seen:
            _override(out, load_config_chain(c, seen))
    _override(out, cur)
    return out


def apply_overrides(hp, hparams_str):
    """--hparams="a=1,b.c=2,d=[1 1 1]" (utils/hparams.py:85-99)"""
    if not hparams_str:
        return hp
    for item in hparams_str.split(","):
        k, v = item.split("=")
        v = v.strip("'\" ")
        node = hp
        for part in k.split(".")[:-1]:
            node = node[part]
        k = k.split(".")[-1]
        old = node.get(k)
        if v in ("True", "False") or isinstance(old, (bool, list, dict)):
            if isinstance(old, list):
                v = v.replace(" ", ",")
            node[k] = eval(v, {"__builtins__": {}}, {})  # literals only
        elif old is None:
            node[k] = yaml.safe_load(v)
        else:
            node[k] = type(old)(v)
    return hp


def set_hparams(config="", exp_name="", hparams_str="", global_hparams=True, work_root="checkpoints"):
    hp = {}
    if config:
        hp.update(load_config_chain(config))
    work_dir = os.path.join(work_root, exp_name) if exp_name else ""
    if work_dir and os.path.exists(os.path.join(work_dir, "config.yaml")):
        with open(os.path.join(work_dir, "config.yaml")) as f:
            hp.update(yaml.safe_load(f) or {})
    hp["work_dir"] = work_dir
    apply_overrides(hp, hparams_str)
    hp["exp_name"] = exp_name
    hp["infer"] = True
    if global_hparams:
        hparams.clear()
        hparams.update(hp)
    return hp


# resolved defaults of egs/datasets/audio/biaobei/dict_tts.yaml (+ use_word_input/word_size/use_dict from the README
# command line), SURVEY.md §5 "Config / flags"; used when no YAML is at hand (synthetic runs)
BIAOBEI_DEFAULTS = {
    "hidden_size": 192, "num_heads": 2, "enc_ffn_kernel_size": 5, "word_size": 8000, "value_embedding_size": 185,
    "audio_num_mel_bins": 80, "latent_size": 16, "fvae_enc_dec_hidden": 192, "fvae_kernel_size": 5,
    "fvae_dec_n_layers": 4, "fvae_enc_n_layers": 8, "prior_glow_hidden": 64, "glow_kernel_size": 3,
    "prior_glow_n_blocks": 4, "dur_predictor_layers": 3, "dur_predictor_kernel": 5, "frames_multiple": 4,
    "language": "zh", "use_post_glow": False, "use_prior_glow": True, "dur_scale": "log", "dur_level": "word",
    "audio_sample_rate": 22050, "hop_size": 256, "fft_size": 1024, "win_size": 1024, "fmin": 80, "fmax": 7600,   # egs/egs_bases/tts/base.yaml:49-54
    "loud_norm": False, "min_level_db": -100, "use_spk_embed": False, "use_spk_id": False, "num_spk": 1,
    "vocoder": "dict_tts_amd.vocoder.HifiGAN", "vocoder_ckpt": "", "use_word_input": True, "use_dict": True,
}

# the light "V3" generator of the original HifiGAN release (config_v3.json): ResBlock2, three upsamplers, hop 256
HIFIGAN_V3 = {
    "resblock": "2", "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8],
    "upsample_initial_channel": 256, "resblock_kernel_sizes": [3, 5, 7],
    "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]],
}

# the small "V2" generator of the original HifiGAN release (config_v2.json): ResBlock1, upsample_initial_channel 128 (widths 64 / 32 / 16 / 8)
HIFIGAN_V2 = {
    "resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
    "upsample_initial_channel": 128, "resblock_kernel_sizes": [3, 7, 11],
    "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
}

HIFIGAN_DEFAULTS = {
    "resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
    "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
    "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
}


def speaker_kind(hp):
    """None (single speaker), "id" (use_spk_id: Embedding(num_spk, hidden)) or "embed" (use_spk_embed: Linear(256, hidden)).
    The reference builds spk_embed_proj only when num_spk > 1 (modules/portaspeech/model.py:159-163) and then crashes in forward
    (modules/dict_tts/model.py:45) when use_spk_* is set with num_spk = 1, the value egs/egs_bases/tts/base.yaml:58 ships: refused here."""
    hp = {**BIAOBEI_DEFAULTS, **(hp or {})}
    if not (hp.get("use_spk_embed") or hp.get("use_spk_id")):
        return None
    num_spk = int(hp.get("num_spk", 1) or 1)
    if num_spk <= 1:
        which = "use_spk_id" if hp.get("use_spk_id") else "use_spk_embed"
        raise ValueError(f"{which}=True needs num_spk > 1, but num_spk={num_spk}: the reference builds no spk_embed_proj then and fails in "
                         f"forward.  Override it with the checkpoint's speaker count, e.g. --hparams num_spk=N")
    return "id" if hp.get("use_spk_id") else "embed"   # use_spk_id wins (modules/portaspeech/model.py:160-163, tasks/tts/dict_tts.py:182)


# what the PortaSpeech baseline (modules/portaspeech/model.py::PortaSpeech) reads beyond BIAOBEI_DEFAULTS, with the values of
# egs/egs_bases/tts/ps.yaml; window_size is TextEncoder's default (model.py:79), not an hparam of the reference
PORTASPEECH_DEFAULTS = {"enc_layers": 4, "word_enc_layers": 4, "ps_window_size": 4}


def is_baseline(hp):
    """True when the hparams' task is the PortaSpeech baseline (``task_cls: tasks.tts.ps_adv.PortaSpeechAdvTask`` / ``tasks.tts.ps.*``),
    False for the Dict-TTS task or when no task is named"""
    task = str((hp or {}).get("task_cls", ""))
    return task.startswith(("tasks.tts.ps_adv.", "tasks.tts.ps.", "tasks.tts.ps_flow."))


def fill_abi_config(cfg, hp=None, voc=None, n_phone=None, vocoder_precision=None, baseline=False):
    """copy reference hparams into a DttsConfig (abi.DttsConfig); unsupported settings fail loudly.  baseline: the config of the
    PortaSpeech baseline (dict_tts_amd.model.PortaSpeech), which also reads enc_layers and refuses what that class does not run"""
    hp = {**BIAOBEI_DEFAULTS, **(hp or {})}
    if hp.get("use_post_glow"):
        raise NotImplementedError("use_post_glow=True is outside the Dict-TTS path (egs/egs_bases/tts/dict_tts.yaml:4)")
    if baseline:
        hp = {**PORTASPEECH_DEFAULTS, **hp}
        if hp.get("use_spk_embed") or hp.get("use_spk_id"):
            which = "use_spk_id" if hp.get("use_spk_id") else "use_spk_embed"
            raise NotImplementedError(f"{which}=True: speakers are not implemented for the PortaSpeech baseline (they are added to ph_encoder_out "
                                      f"including its padded rows, which changes what the duration predictor sees as padding)")
        if hp.get("dur_level", "word") != "word":
            raise NotImplementedError(f"dur_level={hp.get('dur_level')!r}: the PortaSpeech baseline is implemented for dur_level: word only")
        cfg.enc_layers = int(hp["enc_layers"])
    speaker_kind(hp)   # use_spk_embed / use_spk_id need num_spk > 1; nothing of it goes into the config struct (the weights carry the form)
    if not hp.get("use_prior_glow", True) or hp.get("dur_scale", "log") != "log":
        raise NotImplementedError("only use_prior_glow=True / dur_scale=log are implemented")
    for k in ("hidden_size", "num_heads", "enc_ffn_kernel_size", "word_size", "value_embedding_size",
              "audio_num_mel_bins", "latent_size", "fvae_enc_dec_hidden", "fvae_kernel_size", "fvae_dec_n_layers",
              "fvae_enc_n_layers", "prior_glow_hidden", "glow_kernel_size", "prior_glow_n_blocks",
              "dur_predictor_layers", "dur_predictor_kernel", "frames_multiple"):
        setattr(cfg, k, int(hp[k]))
    cfg.language_zh = 1 if hp.get("language", "zh") == "zh" else 0
    if n_phone is not None:
        cfg.n_phone = int(n_phone)
    if voc is not None:
        # modules/hifigan/hifigan.py:109: ResBlock1 if h['resblock'] == '1' else ResBlock2 (YAML / JSON deliver a string or an int)
        resblock = str(voc.get("resblock", "1")).strip()
        if resblock not in ("1", "2"):
            raise NotImplementedError(f"resblock={voc.get('resblock')!r}: the generator's 'resblock' is '1' (ResBlock1) or '2' (ResBlock2)")
        n_dil = 3 if resblock == "1" else 2
        ur, uk = list(voc["upsample_rates"]), list(voc["upsample_kernel_sizes"])
        rk, rd = list(voc["resblock_kernel_sizes"]), [list(d) for d in voc["resblock_dilation_sizes"]]
        cfg.upsample_initial_channel = int(voc["upsample_initial_channel"])
        cfg.n_upsamples = len(ur)
        for i in range(len(ur)):
            cfg.upsample_rates[i] = int(ur[i])
            cfg.upsample_kernel_sizes[i] = int(uk[i])
        cfg.n_resblock_kernels = len(rk)
        for i in range(len(rk)):
            cfg.resblock_kernel_sizes[i] = int(rk[i])
            if len(rd[i]) != n_dil:
                raise NotImplementedError(f"resblock_dilation_sizes[{i}] = {rd[i]}: resblock '{resblock}' (ResBlock{resblock}) expects exactly "
                                          f"{n_dil} dilations per kernel size")
            if any(int(d) < 1 for d in rd[i]):
                raise ValueError(f"resblock_dilation_sizes[{i}] = {rd[i]}: dilations must be >= 1")
            # the struct has no block-type field: a row whose third entry is 0 is a two-dilation (ResBlock2) row (include/dicttts_hip.h)
            for j in range(3):
                cfg.resblock_dilation_sizes[i][j] = int(rd[i][j]) if j < n_dil else 0
    if vocoder_precision is not None:
        cfg.vocoder_precision = int(vocoder_precision)
    # A/B switches of tuning experiments (include/dicttts_hip.h: dtts_config.tune_flags; 0 = the measured defaults).  An explicit
    # key of the hparams / vocoder config, never the process environment.
    cfg.tune_flags = int((hp or {}).get("dtts_tune_flags", 0)) | int((voc or {}).get("dtts_tune_flags", 0))
    rz = (hp or {}).get("dtts_debug_redzone") or (voc or {}).get("dtts_debug_redzone")
    cfg.debug_redzone = (2 if rz is not True and rz == 2 else 1) if rz else 0   # (2: + the launcher's pack-order self-test, include/dicttts_hip.h)
    return cfg
