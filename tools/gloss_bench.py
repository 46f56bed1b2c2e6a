#!/usr/bin/env python3
"""Time the gloss encoder on the device (dtts_text2mel_fetch(DTTS_GLOSS_ENCODE)) against float32 torch on the same device in the same run: the restatement
gloss by gloss (tests/gloss_ref.py: how the reference's binariser runs the model, batch size 1), the same arithmetic on ONE padded batch
with a key mask (torch at its best), and Hugging Face's RoFormerForMaskedLM on the padded batch when ``transformers`` is importable.  Warm,
the sides ALTERNATE call by call; wall time around a synchronised call (encode synchronises once itself), median of --reps after --warmup.

Two workloads at hidden 768 / 12 heads / FFN 3072, 7 layers (seeded weights): one 32-token gloss; 1024 glosses of mixed lengths 3 .. 32.

    python tools/gloss_bench.py [--reps 5] [--warmup 2] [--workload one|dict]

No gate: figures for LABNOTES.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F


def padded_forward(st, cfg, ids, mask, n_hidden):
    """tests/gloss_ref.py on a padded batch: ids [N, T], mask [N, T] bool (keys past a gloss's end get -inf) -> feat [N, T, H]"""
    import gloss_ref as R
    H, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    N, T = ids.shape
    E = st["embeddings.word_embeddings.weight"][ids]
    x = F.layer_norm(E + st["embeddings.token_type_embeddings.weight"][0], (H,), st["embeddings.LayerNorm.weight"], st["embeddings.LayerNorm.bias"], eps)
    sin, cos = (torch.from_numpy(a).to(x) for a in R.rotary_table(T, H // heads))
    bias = torch.zeros(N, 1, 1, T, device=x.device).masked_fill(~mask[:, None, None, :], float("-inf"))
    acc = E + x
    for l in range(n_hidden - 1):
        p = f"encoder.layer.{l}."
        lin = lambda t, name: F.linear(t, st[p + name + ".weight"], st[p + name + ".bias"])
        split = lambda t: t.reshape(N, T, heads, H // heads).transpose(1, 2)
        q, k, v = (split(lin(x, "attention.self." + n)) for n in ("query", "key", "value"))
        q, k = R.rotate(q, sin, cos), R.rotate(k, sin, cos)
        ctx = (torch.softmax(q @ k.transpose(-1, -2) / 8.0 + bias, dim=-1) @ v).transpose(1, 2).reshape(N, T, H)
        a = F.layer_norm(lin(ctx, "attention.output.dense") + x, (H,), st[p + "attention.output.LayerNorm.weight"], st[p + "attention.output.LayerNorm.bias"], eps)
        x = F.layer_norm(lin(F.gelu(lin(a, "intermediate.dense")), "output.dense") + a, (H,), st[p + "output.LayerNorm.weight"], st[p + "output.LayerNorm.bias"], eps)
        acc = acc + x
    return acc / (n_hidden + 1)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", choices=("one", "dict"), default=None)
    ap.add_argument("--no-per-gloss", action="store_true", help="skip the gloss-by-gloss torch form (1024 x 7 layers of small launches)")
    a = ap.parse_args()
    import gloss_ref as R
    import gloss_shapes as S
    from dict_tts_amd import gloss_encoder as G

    cfg, n_hidden = S.config(768, 12, 3072, 7), 8
    st = S.seeded_state(cfg)
    enc = G.GlossEncoder.from_pretrained(st, cfg, n_hidden=n_hidden)
    dst = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    hf = None
    try:
        hf = S.hf_model(cfg, st, torch.float32).cuda()
    except ImportError:
        pass
    rng = np.random.default_rng(5)
    workloads = {"one": [32], "dict": [int(v) for v in rng.integers(3, 33, size=1024)]}
    for name in ([a.workload] if a.workload else ["one", "dict"]):
        lengths = workloads[name]
        seqs = S.id_sets(lengths, seed=11)
        N, Tm = len(seqs), max(lengths)
        ids = torch.zeros(N, Tm, dtype=torch.int64)
        mask = torch.zeros(N, Tm, dtype=torch.bool)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.from_numpy(s)
            mask[i, :len(s)] = True
        ids, mask = ids.cuda(), mask.cuda()

        def padded():
            with torch.no_grad():
                return padded_forward(dst, cfg, ids, mask, n_hidden)

        def hf_padded():
            with torch.no_grad():
                hs = hf(input_ids=ids, attention_mask=mask.long(), output_hidden_states=True, return_dict=True)["hidden_states"]
                return torch.stack([hf.get_input_embeddings()(ids)] + list(hs[0:n_hidden])).mean(dim=0)

        fns = {"unit (encode)": lambda: enc.encode(seqs), "torch float32, one padded batch": padded}
        if not a.no_per_gloss:
            fns["torch float32, gloss by gloss"] = lambda: R.encode(dst, cfg, seqs, torch.float32, "cuda", n_hidden)
        if hf is not None:
            fns["transformers float32, one padded batch"] = hf_padded
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        got, want = enc.encode(seqs), padded()
        diff = max(float((g - want[i, :len(g)]).abs().max()) for i, g in enumerate(got))
        print(json.dumps({"workload": name, "glosses": N, "rows": int(sum(lengths)), "padded_rows": N * Tm, "reps": a.reps,
                          "median_ms (min_ms)": {k: f"{np.median(v):.3f} ({np.min(v):.3f})" for k, v in ms.items()},
                          "max |unit - torch float32|": diff}), flush=True)


if __name__ == "__main__":
    main()
