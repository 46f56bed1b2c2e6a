"""Drop-in for the reference acoustic model ``modules.dict_tts.model.PortaSpeech_dict`` at inference
(modules/dict_tts/model.py:14-121): same ``forward`` signature and return keys, ``load_state_dict`` with the
reference's key names, every tensor op executed by libdicttts_hip.so.

What the reference ignores at inference is accepted and ignored here too: ``ph_tokens`` (txt_tokens[1]),
``key_value_map``, ``ph2word``, ``word_len``, ``mel2ph``, ``tgt_mels``.

``infer=False`` with ``tgt_mels`` and gradients disabled runs the teacher-forced posterior pass the reference's validation_step runs
(modules/dict_tts/fvae_semantics.py:84-108; dtts_text2mel_fetch(DTTS_OUT_POSTERIOR)): it adds ``kl``, ``z_p``, ``m_q``, ``logs_q`` and returns the
reconstruction through the posterior latent as ``mel_out``.  One extra keyword, ``eps`` ([B, latent, T_mel/4]): the posterior sample's
noise (torch.randn_like in the reference); when omitted it is drawn on the device.  Training (gradients) is not implemented.

Speakers (modules/dict_tts/model.py:44-45,94-96): with ``use_spk_embed`` (``spk_embed`` = fp32 [B, 256] utterance embeddings) or
``use_spk_id`` (``spk_embed`` = int64 [B] speaker ids; use_spk_id wins if both are set) and ``num_spk > 1``, ``load_state_dict``
uploads ``spk_embed_proj.*`` and every forward projects the batch's speakers on the GPU and adds them to the word encoder output
(dtts_text2mel_speakers).  Without those hparams ``spk_embed`` is ignored and ``spk_embed_proj.*`` is accepted and not uploaded,
as before; with them, a forward without ``spk_embed`` raises (the reference crashes there).
One extra keyword, ``z_p`` ([B, latent, T_mel/4]): the prior sample, which the reference draws from the CPU
global RNG (modules/dict_tts/fvae_semantics.py:110-111); when omitted it is drawn the same way here.
"""
import numpy as np
import torch

from . import abi
from . import hparams as hparams_mod
from .hparams import fill_abi_config

# state-dict groups that exist in a Dict-TTS checkpoint but are never used by PortaSpeech_dict at inference
# (SURVEY.md §8a "Parameter inventory"): accepted by load_state_dict, not uploaded
UNUSED_PREFIXES = ("attn.", "enc_pos_proj.", "dec_query_proj.", "dec_res_proj.",
                   "dict_encoder.S2PA_module.emb.", "spk_embed_proj.", "post_flow.", "sin_pos.")
SPEAKER_PREFIX = "spk_embed_proj."   # used (uploaded) when the hparams ask for speakers, unused otherwise


def load_checkpoint_state(work_dir, child="model"):
    """newest ``model_ckpt_steps_*.ckpt`` under work_dir -> state_dict[child]
    (utils/ckpt_utils.py:8-25, utils/trainer.py:348-376, 436-449)"""
    import glob
    import re
    paths = sorted(glob.glob(f"{work_dir}/model_ckpt_steps_*.ckpt"),
                   key=lambda x: -int(re.findall(r".*steps\_(\d+)\.ckpt", x)[0]))
    if not paths:
        raise FileNotFoundError(f"no model_ckpt_steps_*.ckpt under {work_dir}")
    ckpt = torch.load(paths[0], map_location="cpu", weights_only=False)
    return ckpt["state_dict"][child], paths[0]


class PortaSpeech_dict(torch.nn.Module):
    def __init__(self, dictionary=None, out_dims=None, hparams=None, ctx=None):
        """dictionary: anything with __len__ (the phoneme TokenTextEncoder of the reference); only its length
        matters (rows of the unused phoneme embedding)."""
        super().__init__()
        if not torch.cuda.is_available():
            raise abi.DttsError("dict_tts_amd.model.PortaSpeech_dict needs a ROCm GPU: the HIP path has no CPU fallback")
        if hparams is None:   # the global hparams, looked up at call time (the INTEGRATION.md hook may rebind them late)
            if not hparams_mod.hparams:
                raise RuntimeError("PortaSpeech_dict(hparams=None) needs the global hparams: call dict_tts_amd.hparams.set_hparams(...) "
                                   "or alias the reference's (INTEGRATION.md), or pass hparams={} for the Biaobei defaults")
            hparams = hparams_mod.hparams
        hp = dict(hparams)
        self.hparams = hp
        self.spk_kind = hparams_mod.speaker_kind(hp)   # None | "embed" | "id"; raises for use_spk_* with num_spk <= 1
        n_phone = len(dictionary) if dictionary is not None else None
        if ctx is None:
            ctx = abi.Context(fill_abi_config(abi.default_config(), hp, None, n_phone=n_phone))
        self.ctx = ctx
        self.cfg = ctx.cfg
        self._state = {}
        self._ready = False
        self.device = torch.device("cuda", torch.cuda.current_device())

    # -- checkpoint compatibility --------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        unexpected = []
        for k in state_dict:
            if k.endswith((".weight", ".bias", ".weight_g", ".weight_v", ".gamma", ".beta", ".in_proj_weight")):
                continue
            unexpected.append(k)
        if strict and unexpected:
            raise RuntimeError(f"Unexpected key(s) in state_dict: {unexpected[:5]}")
        unused = UNUSED_PREFIXES if self.spk_kind is None else tuple(p for p in UNUSED_PREFIXES if p != SPEAKER_PREFIX)
        used = {k: v for k, v in state_dict.items() if not k.startswith(unused)}
        if self.spk_kind is not None:
            want = ["spk_embed_proj.weight"] + (["spk_embed_proj.bias"] if self.spk_kind == "embed" else [])
            missing = [k for k in want if k not in state_dict]
            if missing and strict:
                raise RuntimeError(f"Error(s) in loading state_dict for PortaSpeech_dict: missing key(s) {missing} "
                                   f"(use_spk_{'id' if self.spk_kind == 'id' else 'embed'}=True, num_spk={self.hparams.get('num_spk')})")
        self._state = dict(state_dict)
        self.ctx.load_state_dict("model", used)
        try:
            self.ctx.finalize(abi.PART_ACOUSTIC)   # names the first missing tensor (strict)
        except abi.DttsError as e:
            raise RuntimeError(f"Error(s) in loading state_dict for PortaSpeech_dict: {e}") from e
        self._ready = True
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def state_dict(self, *args, **kwargs):
        return dict(self._state)

    # -- inference -----------------------------------------------------------------------------------------
    def forward(self, txt_tokens, pron_modified, key_value_map, ph2word, word_len, dict_msg, mel2word=None, mel2ph=None,
                spk_embed=None, infer=False, tgt_mels=None, forward_post_glow=True, two_stage=True, z_p=None, eps=None):
        if not infer:
            if tgt_mels is None:
                raise NotImplementedError("the MI355X path implements inference (infer=True) and the teacher-forced posterior pass "
                                          "(infer=False with tgt_mels, gradients disabled)")
            if torch.is_grad_enabled():
                raise NotImplementedError("infer=False with gradients enabled: gradients (training) are not implemented on the MI355X path; "
                                          "run validation under torch.no_grad()")
        if not self._ready:
            raise RuntimeError("load_state_dict() must be called first")
        dev = self.device
        i64 = lambda t: None if t is None else t.to(device=dev, dtype=torch.int64).contiguous()
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        word_tokens = i64(txt_tokens[0])
        keys, values, key_map = f32(dict_msg[0]), f32(dict_msg[1]), f32(dict_msg[2])
        pinyin, pinyin_map = i64(dict_msg[3]), i64(dict_msg[4])
        pron_modified = i64(pron_modified)
        mel2word = i64(mel2word)
        B, T_w = word_tokens.shape
        L_k, P = keys.shape[2], pinyin.shape[2]
        assert keys.shape == (B, T_w, L_k, self.cfg.gloss_dim) and values.shape == keys.shape
        assert key_map.shape == (B, T_w, L_k) and pinyin.shape == pinyin_map.shape == (B, T_w, P)
        stream = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        if not infer:
            tgt_mels = f32(torch.as_tensor(tgt_mels))
            if tgt_mels.dim() != 3 or tgt_mels.shape[0] != B or tgt_mels.shape[2] != self.cfg.audio_num_mel_bins:
                raise ValueError(f"tgt_mels must be [B, T, {self.cfg.audio_num_mel_bins}] with B = {B}, got {tuple(tgt_mels.shape)}")
            if mel2word is not None:   # the length is known before the encode: refuse before any work is enqueued
                fm = self.cfg.frames_multiple
                T_mel = mel2word.shape[1] + (-mel2word.shape[1]) % fm
                if tgt_mels.shape[1] != T_mel:
                    raise ValueError(f"tgt_mels has {tgt_mels.shape[1]} frames, mel2word gives T_mel = {T_mel} (its length {mel2word.shape[1]} "
                                     f"padded to a multiple of frames_multiple = {fm})")
        spk = self._arm_speakers(spk_embed, B, stream)   # noqa: F841  (kept alive until the projection has read it)
        T_mel = self.ctx.text2mel_encode(ptr(word_tokens), ptr(keys), ptr(values), ptr(key_map), ptr(pinyin), ptr(pinyin_map),
                                         ptr(pron_modified), (ptr(mel2word), mel2word.shape[1]) if mel2word is not None else None, B, T_w,
                                         L_k, P, stream)
        if not infer:
            return self._posterior(T_mel, tgt_mels, eps, B, T_w, L_k, P)
        return self._finish(T_mel, z_p, B, T_w, L_k, P)

    def upload_dict_table(self, table):
        """make the dictionary resident in HBM (dict_tts_amd/synth.py:dict_table layout = the reference's dict_embed items)"""
        self.ctx.dict_table_upload(table["tok_off"], table["keys"], table.get("values"), table["key_map"], table["pin_off"],
                                   table["pinyin"], table["pinyin_map"])

    def edit_dict_table(self, replace=None, append=None, pinyin_encoder=None):
        """change the resident dictionary in place (dtts_text2mel_fetch(DTTS_DICT_EDIT)): ``replace`` {entry id: item}, ``append`` [item, ...]
        -> the ids of the appended entries.  Afterwards the table is, bit for bit, what ``upload_dict_table`` of the edited dictionary would
        hold; other entries keep their ids (to delete a word, replace it with the '<UNK>' item).  An item is the binariser's ``dict_embed``
        item: ``key`` [L, gloss_dim], optional ``value`` (= key), ``key_map`` [L], ``pinyin`` [P] (ids, or tokens of ``pinyin_encoder`` as
        ``dict_embed.table_from_items`` takes them), ``pinyin_map`` [P]; ``key`` / ``value`` may be numpy arrays, CPU tensors or CUDA
        tensors.  When every row of the call is a CUDA tensor the rows are concatenated on the device and never touch the host
        (``GlossEncoder.build_items(device=True)``); otherwise they go through the host.  An administrative call: synchronous, with one
        device synchronisation; not for every batch."""
        from . import dict_embed
        replace, append = dict(replace or {}), list(append or [])
        n_old = self.dict_entries()
        ids = sorted(int(e) for e in replace)
        for e in ids:
            if not 0 <= e < n_old:
                raise ValueError(f"edit_dict_table: replace names entry {e}, the table holds {n_old} entries")
        new_ids = list(range(n_old, n_old + len(append)))
        items = [replace[e] for e in ids] + append
        rows = [r for it in items for r in (it["key"], it.get("value")) if r is not None]
        on_device = bool(rows) and all(isinstance(r, torch.Tensor) and r.is_cuda for r in rows)
        p = dict_embed.pack_items(items, pinyin_encoder, rows=not on_device)
        if p["D"] is not None and p["D"] != self.cfg.gloss_dim:
            raise ValueError(f"edit_dict_table: the items' rows are {p['D']} wide, gloss_dim = {self.cfg.gloss_dim}")
        stream = torch.cuda.current_stream().cuda_stream
        if on_device:
            f32 = lambda t: t.to(device=self.device, dtype=torch.float32)
            keys = torch.cat([f32(it["key"]) for it in items]).contiguous()
            separate = any(it.get("value") is not None and it["value"] is not it["key"] for it in items)
            values = torch.cat([f32(it["value"] if it.get("value") is not None else it["key"]) for it in items]).contiguous() if separate else None
            kp, vp = keys.data_ptr(), None if values is None else values.data_ptr()   # (alive until the call, which synchronises, returns)
        else:
            kp = np.concatenate(p["keys"]) if items else np.zeros((0, self.cfg.gloss_dim), np.float32)
            vp = None if p["same"] else np.concatenate(p["values"])
        self.ctx.dict_table_edit(ids + new_ids, p["tok_off"], p["pin_off"], p["key_map"], p["pinyin"], p["pinyin_map"], kp, vp, stream,
                                 rows_on_device=on_device)
        return new_ids

    def dict_entries(self):
        """entries of the resident table (0 before ``upload_dict_table``)"""
        return self.ctx.dict_table_entry(-1, torch.cuda.current_stream().cuda_stream)[0]

    def dict_entry(self, e):
        """what the resident table holds for entry ``e`` (dtts_text2mel_fetch(DTTS_DICT_ENTRY)): device tensors ``K`` / ``V`` [L, hidden] (the
        PROJECTED rows), ``key_map`` [L], ``pinyin`` / ``pinyin_map`` [P], and the ints ``L``, ``P``"""
        stream = torch.cuda.current_stream().cuda_stream
        _, L, P = self.ctx.dict_table_entry(int(e), stream)
        out = lambda shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device=self.device)
        r = {"K": out((L, self.cfg.hidden_size)), "V": out((L, self.cfg.hidden_size)), "key_map": out((L,)),
             "pinyin": out((P,), torch.int64), "pinyin_map": out((P,), torch.int64)}
        self.ctx.dict_table_entry(int(e), stream, k=r["K"].data_ptr(), v=r["V"].data_ptr(), key_map=r["key_map"].data_ptr(),
                                  pinyin=r["pinyin"].data_ptr(), pinyin_map=r["pinyin_map"].data_ptr())
        r.update(L=L, P=P)
        return r

    def _arm_speakers(self, spk_embed, B, stream):
        """project the batch's speakers and arm the next encode (modules/dict_tts/model.py:44-45; tasks/tts/dict_tts.py:182 passes
        sample['spk_ids'] with use_spk_id, sample['spk_embed'] otherwise); returns the device tensor the projection reads"""
        if self.spk_kind is None:
            return None
        if spk_embed is None:
            raise abi.DttsError(f"use_spk_{self.spk_kind}=True: forward needs spk_embed (" +
                             ("int64 speaker ids [B]" if self.spk_kind == "id" else "fp32 speaker embeddings [B, 256]") +
                             "); the reference crashes in spk_embed_proj(None) here")
        if self.spk_kind == "id":
            t = torch.as_tensor(spk_embed).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
            if t.shape[0] != B:
                raise ValueError(f"spk_ids has {t.shape[0]} entries for a batch of {B}")
            self.ctx.text2mel_speakers(abi.SPK_ID, t.data_ptr(), B, stream)
        else:
            t = torch.as_tensor(spk_embed).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(t.shape) != (B, 256):
                raise ValueError(f"spk_embed must be [B, 256] = [{B}, 256], got {tuple(t.shape)}")
            self.ctx.text2mel_speakers(abi.SPK_EMBED, t.data_ptr(), B, stream)
        return t

    def forward_ids(self, word_tokens, entry_ids, pron_modified, L_k, P, mel2word=None, z_p=None, spk_embed=None):
        """forward(infer=True) with the dictionary tensors replaced by ids into the resident table"""
        dev = self.device
        word_tokens = word_tokens.to(device=dev, dtype=torch.int64).contiguous()
        entry_ids = entry_ids.to(device=dev, dtype=torch.int32).contiguous()
        pron_modified = None if pron_modified is None else pron_modified.to(device=dev, dtype=torch.int64).contiguous()
        mel2word = None if mel2word is None else mel2word.to(device=dev, dtype=torch.int64).contiguous()
        B, T_w = word_tokens.shape
        stream = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        spk = self._arm_speakers(spk_embed, B, stream)   # noqa: F841
        T_mel = self.ctx.text2mel_encode_ids(ptr(word_tokens), ptr(entry_ids), ptr(pron_modified),
                                             (ptr(mel2word), mel2word.shape[1]) if mel2word is not None else None, B, T_w,
                                             int(L_k), int(P), stream)
        return self._finish(T_mel, z_p, B, T_w, int(L_k), int(P))

    def _posterior(self, T_mel, tgt_mels, eps, B, T_w, L_k, P):
        """the teacher-forced FVAE posterior pass (fvae_semantics.py:84-108) after the encode; returns forward(infer=False)'s keys"""
        dev = self.device
        stream = torch.cuda.current_stream().cuda_stream
        if tgt_mels.shape[1] != T_mel:   # predicted durations: T_mel is known after the encode (the reference fails on the shapes here)
            raise ValueError(f"tgt_mels has {tgt_mels.shape[1]} frames, the durations give T_mel = {T_mel}")
        Z, T4 = self.cfg.latent_size, T_mel // 4
        if eps is not None:
            eps = eps.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(eps.shape) != (B, Z, T4):
                raise ValueError(f"eps must be [B, {Z}, T_mel/4] = {(B, Z, T4)}, got {tuple(eps.shape)}")
        out = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        mel = out(B, T_mel, self.cfg.audio_num_mel_bins)
        m_q, logs_q, z_p, kl = out(B, Z, T4), out(B, Z, T4), out(B, Z, T4), out(())
        self.ctx.text2mel_posterior(tgt_mels.data_ptr(), T_mel, None if eps is None else eps.data_ptr(), T4, mel.data_ptr(), T_mel,
                                    m_q.data_ptr(), logs_q.data_ptr(), z_p.data_ptr(), kl.data_ptr(), stream)
        ret = self._fetch_encoder(B, T_w, L_k, P, T_mel)
        ret["mel_out"] = ret["mel_out_fvae"] = mel
        ret.update(kl=kl, z_p=z_p, m_q=m_q, logs_q=logs_q)
        ret["rel"] = ret["dp_attn"] = None
        return ret

    def _finish(self, T_mel, z_p, B, T_w, L_k, P):
        dev = self.device
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        stream = torch.cuda.current_stream().cuda_stream
        Z = self.cfg.latent_size
        if z_p is None:
            z_p = torch.distributions.Normal(0, 1).sample([B, Z, T_mel // 4])  # fvae_semantics.py:110
        z_p = f32(z_p)
        assert tuple(z_p.shape) == (B, Z, T_mel // 4), (tuple(z_p.shape), (B, Z, T_mel // 4))
        n_mel = self.cfg.audio_num_mel_bins
        mel = torch.empty(B, T_mel, n_mel, dtype=torch.float32, device=dev)
        self.ctx.text2mel_decode(z_p.data_ptr(), mel.data_ptr(), stream)
        ret = self._fetch_encoder(B, T_w, L_k, P, T_mel)
        ret["mel_out"] = ret["mel_out_fvae"] = mel
        ret["rel"] = ret["dp_attn"] = None
        ret["z_p_in"] = z_p
        return ret

    def _fetch_encoder(self, B, T_w, L_k, P, T_mel):
        dev = self.device
        stream = torch.cuda.current_stream().cuda_stream
        H = self.cfg.hidden_size
        ret = {}
        out = lambda shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device=dev)
        ret["pron_attn"] = out((B, T_w, P))
        ret["dur"] = out((B, T_w))
        ret["dict_attn"] = out((B, 1, L_k, T_w))
        ret["word_encoder_out"] = out((B, T_w, H))
        ret["x_mask"] = out((B, T_mel, 1))
        ret["mel2word"] = out((B, T_mel), torch.int64)
        ret["mel_lens"] = out((B,), torch.int32)
        for key, what in (("pron_attn", abi.OUT_PRON_ATTN), ("dur", abi.OUT_DUR), ("dict_attn", abi.OUT_DICT_ATTN),
                          ("word_encoder_out", abi.OUT_WORD_ENCODER_OUT), ("x_mask", abi.OUT_X_MASK),
                          ("mel2word", abi.OUT_MEL2WORD), ("mel_lens", abi.OUT_MEL_LENS)):
            self.ctx.fetch(what, ret[key].data_ptr(), stream)
        return ret


# state-dict groups of a baseline checkpoint that the PortaSpeech class accepts and does not upload
PS_UNUSED_PREFIXES = ("post_flow.", "g_proj.", "sin_pos.", "spk_embed_proj.")
PS_USED_PREFIXES = ("ph_encoder.", "word_encoder.", "enc_pos_proj.", "dec_query_proj.", "dec_res_proj.", "attn.", "dur_predictor.", "fvae.")


class PortaSpeech(torch.nn.Module):
    """Drop-in for the reference's phoneme-input baseline ``modules.portaspeech.model.PortaSpeech`` at inference (model.py:133-367;
    ``task_cls: tasks.tts.ps_adv.PortaSpeechAdvTask``, ``dur_level: word``, ``use_post_glow: false``): the same ``forward`` signature and
    return keys, ``load_state_dict`` with the reference's key names, every tensor op executed by libdicttts_hip.so
    (dtts_text2mel_fetch(DTTS_PS_ENCODE) + dtts_text2mel_decode).  Extra keyword ``z_p`` ([B, latent, T_mel/4]): the prior sample, drawn as
    the reference draws it when omitted.  Refused by name: ``infer=False`` (the baseline's posterior pass is not implemented),
    ``dur_level: ph``, ``use_post_glow``, ``use_spk_embed`` / ``use_spk_id``.  ``ret['attn']`` rows of frames with mel2word = 0 are zeros
    (the reference leaves meaningless softmax rows there; they never reach decoder_inp)."""

    def __init__(self, dictionary=None, out_dims=None, hparams=None, ctx=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise abi.DttsError("dict_tts_amd.model.PortaSpeech needs a ROCm GPU: the HIP path has no CPU fallback")
        if hparams is None:
            if not hparams_mod.hparams:
                raise RuntimeError("PortaSpeech(hparams=None) needs the global hparams: call dict_tts_amd.hparams.set_hparams(...) "
                                   "or alias the reference's (INTEGRATION.md), or pass hparams={} for the ps_adv.yaml defaults")
            hparams = hparams_mod.hparams
        hp = {**hparams_mod.PORTASPEECH_DEFAULTS, **dict(hparams)}
        self.hparams = hp
        if out_dims is not None and int(out_dims) != int(hp.get("audio_num_mel_bins", 80)):
            raise NotImplementedError(f"out_dims={out_dims} differs from audio_num_mel_bins={hp.get('audio_num_mel_bins', 80)}")
        n_phone = len(dictionary) if dictionary is not None else hp.get("ps_n_phone")
        if n_phone is None:
            raise ValueError("PortaSpeech needs the phoneme dictionary (its length gives the rows of ph_encoder.emb)")
        if ctx is None:
            ctx = abi.Context(fill_abi_config(abi.default_config(), hp, None, n_phone=n_phone, baseline=True))
        self.ctx = ctx
        self.cfg = ctx.cfg
        self._state = {}
        self._ready = False
        self.device = torch.device("cuda", torch.cuda.current_device())

    def load_state_dict(self, state_dict, strict=True):
        unexpected = [k for k in state_dict if not k.startswith(PS_USED_PREFIXES + PS_UNUSED_PREFIXES)]
        if strict and unexpected:
            raise RuntimeError(f"Unexpected key(s) in state_dict: {unexpected[:5]}")
        used = {k: v for k, v in state_dict.items() if k.startswith(PS_USED_PREFIXES) and not k.endswith("embed_positions._float_tensor")}
        from .fft import DEFAULT_MAX_TARGET_POSITIONS, sinusoid_table
        H = self.cfg.hidden_size
        used["config"] = np.array([self.hparams["ps_window_size"], self.hparams["word_enc_layers"]], np.float32)
        used["word_encoder.pos_table"] = sinusoid_table(DEFAULT_MAX_TARGET_POSITIONS, H, 0)   # SinusoidalPositionalEmbedding.weights
        self._state = dict(state_dict)
        self.ctx.load_state_dict("ps", used)
        try:
            self.ctx.finalize(abi.PART_PORTASPEECH)   # names the first missing tensor (strict)
        except abi.DttsError as e:
            raise RuntimeError(f"Error(s) in loading state_dict for PortaSpeech: {e}") from e
        self._ready = True
        return torch.nn.modules.module._IncompatibleKeys([], [])

    def state_dict(self, *args, **kwargs):
        return dict(self._state)

    def forward(self, txt_tokens, ph2word, word_len, mel2word=None, mel2ph=None, spk_embed=None, infer=False, tgt_mels=None,
                forward_post_glow=True, two_stage=True, z_p=None):
        if not infer:
            raise NotImplementedError("PortaSpeech.forward(infer=False): the posterior pass of the baseline is not implemented on the MI355X "
                                      "path; only inference (infer=True) is")
        if not self._ready:
            raise RuntimeError("load_state_dict() must be called first")
        dev = self.device
        i64 = lambda t: None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous()
        txt_tokens, ph2word, mel2word = i64(txt_tokens), i64(ph2word), i64(mel2word)
        B, T_ph = txt_tokens.shape
        if tuple(ph2word.shape) != (B, T_ph):
            raise ValueError(f"ph2word must be [B, T_ph] = {(B, T_ph)}, got {tuple(ph2word.shape)}")
        T_w = int(torch.as_tensor(word_len).max())     # the reference: torch.arange(word_len) / word_len.max() + 1 (model.py:240,316)
        stream = torch.cuda.current_stream().cuda_stream
        status = torch.zeros(4, dtype=torch.int64, device=dev)
        T_mel = self.ctx.ps_encode(B, T_ph, T_w, txt_tokens.data_ptr(), ph2word.data_ptr(), status.data_ptr(), stream,
                                   mel2word=(mel2word.data_ptr(), mel2word.shape[1]) if mel2word is not None else None, want_attn=True)
        bad = abi.ps_status_error(status.cpu().tolist())   # (the frames' checks, and all of them with a teacher-forced mel2word)
        if bad:
            raise abi.DttsError(f"dtts_text2mel_fetch(DTTS_PS_ENCODE): {bad}")
        H, Z, n_mel = self.cfg.hidden_size, self.cfg.latent_size, self.cfg.audio_num_mel_bins
        if z_p is None:
            z_p = torch.distributions.Normal(0, 1).sample([B, Z, T_mel // 4])   # fvae.py: prior_dist.sample
        z_p = z_p.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(z_p.shape) == (B, Z, T_mel // 4), (tuple(z_p.shape), (B, Z, T_mel // 4))
        mel = torch.empty(B, T_mel, n_mel, dtype=torch.float32, device=dev)
        self.ctx.text2mel_decode(z_p.data_ptr(), mel.data_ptr(), stream)
        out = lambda shape, dt=torch.float32: torch.empty(*shape, dtype=dt, device=dev)
        ret = {"ph_encoder_out": out((B, T_ph, H)), "dur": out((B, T_w)), "attn": out((B, T_mel, T_ph)), "word_encoder_out": out((B, T_w, H)),
               "x_mask": out((B, T_mel, 1)), "decoder_inp": out((B, T_mel, H)), "mel2word": out((B, T_mel), torch.int64),
               "mel_lens": out((B,), torch.int32)}
        for key, what in (("ph_encoder_out", abi.PS_PH_ENCODER_OUT), ("dur", abi.OUT_DUR), ("attn", abi.PS_ATTN),
                          ("word_encoder_out", abi.OUT_WORD_ENCODER_OUT), ("x_mask", abi.OUT_X_MASK), ("decoder_inp", abi.PS_DECODER_INP),
                          ("mel2word", abi.OUT_MEL2WORD), ("mel_lens", abi.OUT_MEL_LENS)):
            self.ctx.fetch(what, ret[key].data_ptr(), stream)
        ret["mel_out"] = ret["mel_out_fvae"] = mel
        ret["z_p_in"] = z_p
        return ret


def model_cls(hp):
    """the acoustic model class of the hparams' task: PortaSpeech for ``task_cls: tasks.tts.ps_adv.*`` (the baseline), else PortaSpeech_dict"""
    return PortaSpeech if hparams_mod.is_baseline(hp) else PortaSpeech_dict


def decode_pinyin_ids(pron_attn, pinyin):
    """after_infer's pinyin decode for ONE utterance (tasks/tts/dict_tts.py:294-304): pron_attn [T_w,P],
    pinyin [T_w,P] -> list of pinyin-token ids, two per inner word"""
    pron_attn = torch.as_tensor(np.asarray(pron_attn.detach().cpu() if hasattr(pron_attn, "detach") else pron_attn))
    pinyin = torch.as_tensor(np.asarray(pinyin.detach().cpu() if hasattr(pinyin, "detach") else pinyin))
    _, max_idx = pron_attn.max(dim=-1)
    ids = []
    for i in range(1, pinyin.shape[0] - 1):
        ids += pinyin[i][max_idx[i]:max_idx[i] + 2].tolist()
    return ids
