"""Gloss embeddings on the device: the RoFormer encoder behind the reference's ``dict_embed`` — ``data_gen/tts/binarizer_zh.py`` runs
``pretrained/roformer-chinese-base`` on every dictionary gloss and keeps, per token, the mean of the word embedding and the first eight
hidden states (``get_encodings``); ``gen_dict_embeddings`` concatenates a word's glosses into one item.  dict_tts_amd/csrc/gloss.hip
(dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)) computes the same on a ragged batch of glosses; the arithmetic is specified in include/dicttts_hip.h and restated in
float64 by tests/gloss_ref.py.

Tokenisation (RoFormer's jieba pre-tokeniser), ``preprocess_text`` and pypinyin stay with the caller: ``encode`` takes token ids,
``[CLS]`` and ``[SEP]`` included.  Neither the checkpoint nor its tokenizer was available here: see INTEGRATION.md ("Gloss encoder").
"""
import json
import os

import numpy as np
import torch

from . import abi, dict_embed
from .unit import DeviceUnit

HEAD = 64
UNK_PINYIN = "<UNK>"


def check_config(config, n_hidden=8):
    """the refusals that need no device: a configuration the kernels do not implement is named (ValueError)"""
    H, heads = int(config["hidden_size"]), int(config["num_attention_heads"])
    if H % HEAD or heads < 1 or H % heads or H // heads != HEAD:
        raise ValueError(f"hidden_size = {H} with num_attention_heads = {heads}: the gloss encoder supports heads of {HEAD} channels and a hidden "
                         f"size that is a multiple of {HEAD}")
    E = int(config.get("embedding_size", H))
    if E != H:
        raise ValueError(f"embedding_size = {E} differs from hidden_size = {H} (the reference's feature buffer assumes they are equal)")
    F = int(config["intermediate_size"])
    if not 4 <= F <= 65536 or F % 4:
        raise ValueError(f"intermediate_size = {F}: the gloss encoder supports a multiple of 4 up to 65536 (the feed-forward rows are read in "
                         f"16-byte pieces)")
    if config.get("rotary_value", False):
        raise ValueError("rotary_value = true is not supported (the reference's checkpoint rotates q and k only)")
    if config.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act = {config.get('hidden_act')!r}: only the erf GELU ('gelu') is supported")
    if not 2 <= int(n_hidden) <= int(config["num_hidden_layers"]) + 1:
        raise ValueError(f"n_hidden = {n_hidden} hidden states (supported: 2 .. num_hidden_layers + 1 = {int(config['num_hidden_layers']) + 1})")


def layer_keys(l):
    p = f"encoder.layer.{l}."
    names = [f"attention.self.{n}" for n in ("query", "key", "value")] + ["attention.output.dense", "attention.output.LayerNorm", "intermediate.dense",
                                                                         "output.dense", "output.LayerNorm"]
    return [p + n + s for n in names for s in (".weight", ".bias")]


def select_state(state, config, n_hidden=8):
    """-> {key without 'roformer.': float32 array} of exactly the tensors the first n_hidden hidden states need (layers 0 .. n_hidden - 2);
    a missing one is refused by name (KeyError).  The MLM head, the later layers and ``embed_positions`` are not taken"""
    st = {(k[len("roformer."):] if k.startswith("roformer.") else k): v for k, v in state.items()}
    keys = ["embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for l in range(int(n_hidden) - 1):
        keys += layer_keys(l)
    out = {}
    for k in keys:
        if k not in st:
            raise KeyError(f"the gloss encoder's state dict lacks {k}")
        v = st[k]
        out[k] = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), np.float32)
    E = out["embeddings.word_embeddings.weight"].shape
    if len(E) != 2 or E[1] != int(config["hidden_size"]):
        raise ValueError(f"embeddings.word_embeddings.weight is {list(E)}; the encoder's is [vocab, {int(config['hidden_size'])}] "
                         f"(embedding_size must equal hidden_size)")
    return out


class GlossEncoder(DeviceUnit):
    """``GlossEncoder.from_pretrained("pretrained/roformer-chinese-base").encode(id_sequences)``.

    ctx: an existing ``abi.Context`` or None for one of its own; it is created, and the weights loaded, on the first device call, so that
    argument and configuration errors surface without a GPU.  row_budget: token rows per library call (the workspace is
    ``rows * (3 hidden + max(4 hidden, ffn))`` floats: 21.5 KB per row at 768 / 3072)."""

    PREFIX, PART = "gloss", abi.PART_GLOSS

    def __init__(self, ctx=None, row_budget=16384):
        if int(row_budget) < abi.GLOSS_MAX_L:
            raise ValueError(f"row_budget = {row_budget} (must hold one gloss of {abi.GLOSS_MAX_L} tokens)")
        self.ctx = ctx
        self.row_budget = int(row_budget)
        self.weights = None
        self.config = None
        self.n_hidden = None

    # ---- weights
    def load_state_dict(self, state, config, n_hidden=8):
        if self._loaded:
            raise abi.DttsError("GlossEncoder.load_state_dict: this encoder's weights are already on the device (a context builds the part once)")
        check_config(config, n_hidden)
        self.weights = select_state(state, config, n_hidden)
        self.config, self.n_hidden = dict(config), int(n_hidden)
        self.hidden = int(config["hidden_size"])
        self.vocab = int(self.weights["embeddings.word_embeddings.weight"].shape[0])
        return self

    @classmethod
    def from_pretrained(cls, dir_or_state, config=None, n_hidden=8, ctx=None, row_budget=16384):
        """a Hugging Face model directory (``config.json`` + ``pytorch_model.bin``), or a state dict with ``config`` (a dict of the same
        names); keys with or without the ``roformer.`` prefix.  Keeps layers 0 .. n_hidden - 2"""
        if isinstance(dir_or_state, (str, bytes)) or hasattr(dir_or_state, "__fspath__"):
            d = os.fspath(dir_or_state)
            with open(os.path.join(d, "config.json")) as f:
                config = json.load(f)
            check_config(config, n_hidden)   # before the (large) checkpoint is read
            dir_or_state = torch.load(os.path.join(d, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        elif config is None:
            raise ValueError("GlossEncoder.from_pretrained: a state dict needs its config (the dict of config.json)")
        return cls(ctx=ctx, row_budget=row_budget).load_state_dict(dir_or_state, config, n_hidden)

    def _state(self):
        if self.weights is None:
            raise abi.DttsError("GlossEncoder: no weights (load_state_dict / from_pretrained first)")
        w = dict(self.weights)
        w["config"] = np.array([self.config["num_attention_heads"], self.config.get("layer_norm_eps", 1e-12),
                                1.0 if self.config.get("rotary_value", False) else 0.0, 0.0 if self.config.get("hidden_act", "gelu") == "gelu" else 1.0],
                               np.float32)
        return w

    # ---- device calls
    def encode(self, id_sequences):
        """id_sequences: token-id sequences of 1 .. 64 ids each, [CLS] and [SEP] included -> one float32 device tensor [L, hidden] per
        gloss, the reference's ``feat``.  A gloss's result does not depend on the others or on ``row_budget``.  An id outside the
        vocabulary raises (DttsError naming the gloss, the position and the id) after the batch has run."""
        seqs = [np.asarray(s, np.int64).reshape(-1) for s in id_sequences]
        for g, s in enumerate(seqs):
            if not 1 <= len(s) <= abi.GLOSS_MAX_L:
                raise ValueError(f"gloss {g} has L = {len(s)} tokens (supported: 1 .. {abi.GLOSS_MAX_L})")
        ctx = self._context()
        if not seqs:
            return []
        dev, stream = self.device, torch.cuda.current_stream().cuda_stream
        chunks, start, rows = [], 0, 0
        for g, s in enumerate(seqs):   # consecutive glosses while their rows fit the budget
            if rows + len(s) > self.row_budget:
                chunks.append((start, g))
                start, rows = g, 0
            rows += len(s)
        chunks.append((start, len(seqs)))
        status = torch.zeros(len(chunks), 2, dtype=torch.int64, device=dev)
        outs = []
        for c, (g0, g1) in enumerate(chunks):
            lens = np.array([len(s) for s in seqs[g0:g1]], np.int64)
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            ids = torch.from_numpy(np.concatenate(seqs[g0:g1])).to(dev)
            tok_off = torch.from_numpy(off).to(dev)
            out = torch.empty(int(off[-1]), self.hidden, dtype=torch.float32, device=dev)
            ctx.gloss_encode(g1 - g0, stream, ids=ids.data_ptr(), tok_off=tok_off.data_ptr(), sum_L=int(off[-1]), L_max=int(lens.max()),
                             out=out.data_ptr(), status=status[c].data_ptr())
            outs += [out[off[i]:off[i + 1]] for i in range(g1 - g0)]
        bad = status.cpu().numpy()
        for c, (g0, g1) in enumerate(chunks):
            if bad[c, 0]:
                row, g = int(bad[c, 0]) - 1, g0
                while row >= len(seqs[g]):
                    row -= len(seqs[g])
                    g += 1
                raise abi.DttsError(f"GlossEncoder.encode: gloss {g}, position {row}: token id {int(bad[c, 1])} is outside the vocabulary "
                                    f"of {self.vocab} (row {int(bad[c, 0]) - 1} of its call; its embedding was taken as zero)")
        return outs

    __call__ = encode

    def build_items(self, entries, n_words, device=False):
        """entries: {word id: [((initial, final_tone3), ids), ...]} — per word the glosses of its pronunciations in dictionary order, each
        with its pinyin pair and its token ids.  -> the ``n_words`` items of the binariser's ``dict_embed`` in word-id order (CPU tensors):
        key = value = the glosses' features concatenated, key_map ``[0] + [g + 1] * (L_g - 2) + [0]`` per gloss, pinyin the pairs
        concatenated, pinyin_map ``[g + 1] * 2``; a word without an entry gets the binariser's ``<UNK>`` item.  ``tokens_gloss`` holds the
        token ids (the caller has the tokenizer that names them).  device=True keeps ``key`` / ``value`` on the device (the '<UNK>' items'
        zero rows too): gloss ids -> embeddings -> ``PortaSpeech_dict.edit_dict_table`` then never touches the host"""
        order = [w for w in range(int(n_words)) if w in entries and len(entries[w])]
        for w in entries:
            if not 0 <= int(w) < int(n_words):
                raise ValueError(f"entries holds word id {w}; the dictionary has {n_words} words")
        feats = iter(self.encode([ids for w in order for _, ids in entries[w]]))
        items = []
        for w in range(int(n_words)):
            if w not in entries or not len(entries[w]):
                z = torch.zeros(3, self.hidden, device=self.device if device else None)
                items.append({"tokens_gloss": ["O"], "key": z, "key_map": [0, 1, 0], "value": z.clone(), "pinyin": [UNK_PINYIN], "pinyin_map": [1]})
                continue
            key, key_map, pinyin, pinyin_map, tokens = [], [], [], [], []
            for g, (pair, ids) in enumerate(entries[w]):
                f = next(feats) if device else next(feats).cpu()
                key.append(f)
                key_map += [0] + [g + 1] * (f.shape[0] - 2) + [0]
                pinyin += list(pair)
                pinyin_map += [g + 1] * len(pair)
                tokens += [int(i) for i in ids]
            feat = torch.cat(key)
            items.append({"tokens_gloss": tokens, "key": feat, "key_map": key_map, "value": feat, "pinyin": pinyin, "pinyin_map": pinyin_map})
        return items

    def build_table(self, entries, n_words, pinyin_encoder=None):
        """-> the ragged arrays ``dtts_dict_table_upload`` takes (dict_embed.table_from_items) of ``build_items``, + ``pinyin_encoder``:
        the given list, or the one the binariser builds (``['<UNK>']``, then every initial / final in order of first appearance)"""
        items = self.build_items(entries, n_words)
        if pinyin_encoder is None:
            pinyin_encoder = [UNK_PINYIN]
            for it in items:
                for p in it["pinyin"]:
                    if p not in pinyin_encoder:
                        pinyin_encoder.append(p)
        table = dict_embed.table_from_items(items, pinyin_encoder)
        table["pinyin_encoder"] = list(pinyin_encoder)
        return table
