"""The gloss encoder restated: what ``data_gen/tts/binarizer_zh.py::get_encodings`` takes from ``RoFormerForMaskedLM`` — the mean of the word
embeddings and the first ``n_hidden`` hidden states — written out in torch at a chosen dtype, one gloss at a time as the reference runs them
(batch size 1, no padding).  float64 is the definition the GPU is measured against, float32 the yardstick of its error.  Needs no
``transformers``; tests/test_gloss_cpu.py compares it with the Hugging Face model where that is importable.

state: Hugging Face keys (numpy or torch), with or without the ``roformer.`` prefix.  cfg: the names of ``config.json``."""
import numpy as np
import torch
import torch.nn.functional as F

HEAD = 64


def strip(state):
    """-> {key without 'roformer.': value}; the MLM head (cls.*) and the stored position table are dropped"""
    out = {}
    for k, v in state.items():
        k = k[len("roformer."):] if k.startswith("roformer.") else k
        if k.startswith("cls.") or k.endswith("embed_positions.weight"):
            continue
        out[k] = v
    return out


def rotary_table(n_pos, d=HEAD):
    """(sin, cos) [n_pos, d // 2] as RoFormerSinusoidalPositionalEmbedding holds them: computed in float64, rounded to float32"""
    ang = np.array([[pos / np.power(10000, 2 * j / d) for j in range(d // 2)] for pos in range(n_pos)], np.float64)
    return np.sin(ang).astype(np.float32), np.cos(ang).astype(np.float32)


def _t(state, key, dtype, device):
    v = state[key]
    v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    return torch.from_numpy(np.ascontiguousarray(v)).to(device=device, dtype=dtype)


def layers_of(state):
    return 1 + max(int(k.split(".")[2]) for k in strip(state) if k.startswith("encoder.layer."))


def rotate(t, sin, cos):
    """t [heads, L, d]; sin / cos [L, d // 2]: t cos_pos + rot(t) sin_pos with rot(t)[2j] = -t[2j + 1], rot(t)[2j + 1] = t[2j]"""
    sin_pos = torch.repeat_interleave(sin, 2, dim=-1)
    cos_pos = torch.repeat_interleave(cos, 2, dim=-1)
    rot = torch.stack([-t[..., 1::2], t[..., 0::2]], dim=-1).reshape(t.shape)
    return t * cos_pos + rot * sin_pos


def hidden_states(state, cfg, ids, dtype=torch.float64, device="cpu", n_hidden=8):
    """one gloss: ids [L] -> [E, h_0, .., h_(n_hidden - 1)], each [L, H]"""
    st = strip(state)
    g = lambda k: _t(st, k, dtype, device)
    eps, heads = float(cfg.get("layer_norm_eps", 1e-12)), int(cfg["num_attention_heads"])
    ids = torch.as_tensor(np.asarray(ids, np.int64), device=device)
    L = ids.shape[0]
    E = g("embeddings.word_embeddings.weight")[ids]
    H = E.shape[1]
    x = F.layer_norm(E + g("embeddings.token_type_embeddings.weight")[0], (H,), g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), eps)
    sin, cos = (torch.from_numpy(a).to(device=device, dtype=dtype) for a in rotary_table(L, H // heads))
    out = [E, x]
    for l in range(n_hidden - 1):
        p = f"encoder.layer.{l}."
        lin = lambda t, name: F.linear(t, g(p + name + ".weight"), g(p + name + ".bias"))
        split = lambda t: t.reshape(L, heads, H // heads).transpose(0, 1)
        q, k, v = (split(lin(x, "attention.self." + n)) for n in ("query", "key", "value"))
        q, k = rotate(q, sin, cos), rotate(k, sin, cos)
        scores = q @ k.transpose(-1, -2) / np.sqrt(H // heads)
        ctx = (torch.softmax(scores, dim=-1) @ v).transpose(0, 1).reshape(L, H)
        a = F.layer_norm(lin(ctx, "attention.output.dense") + x, (H,), g(p + "attention.output.LayerNorm.weight"), g(p + "attention.output.LayerNorm.bias"), eps)
        f = F.gelu(lin(a, "intermediate.dense"))
        x = F.layer_norm(lin(f, "output.dense") + a, (H,), g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"), eps)
        out.append(x)
    return out


def encode(state, cfg, id_seqs, dtype=torch.float64, device="cpu", n_hidden=8):
    """-> list of feat [L, H] = mean(stack([E, h_0, .., h_(n_hidden - 1)]), 0), one per gloss, each run alone"""
    with torch.no_grad():
        return [torch.stack(hidden_states(state, cfg, ids, dtype, device, n_hidden)).mean(dim=0) for ids in id_seqs]


def encode_np(state, cfg, id_seqs, dtype=torch.float64, n_hidden=8):
    """the same, concatenated: float64 numpy [sum_L, H]"""
    return np.concatenate([f.double().cpu().numpy() for f in encode(state, cfg, id_seqs, dtype, "cpu", n_hidden)])
