"""Configurations, id sets and seeded weights of the gloss-encoder tests (tests/test_gloss_cpu.py, tests/test_gloss_gpu.py,
tools/make_golden_gloss.py, tools/gloss_bench.py).  Weights are seeded, never a real checkpoint."""
import numpy as np

SEED = 1806
VOCAB = 97


def config(hidden, heads, ffn, layers, vocab=VOCAB):
    """the fields of a RoFormer ``config.json`` the encoder reads (and the ones RoFormerConfig needs to build the model)"""
    return {"vocab_size": vocab, "embedding_size": hidden, "hidden_size": hidden, "num_hidden_layers": layers, "num_attention_heads": heads,
            "intermediate_size": ffn, "hidden_act": "gelu", "layer_norm_eps": 1e-12, "rotary_value": False, "type_vocab_size": 2,
            "max_position_embeddings": 128, "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0}


# name -> (config, n_hidden): the accuracy shapes (the mean runs over layers + 2 terms, n_hidden = layers + 1 hidden states)
CFGS = {"h128x7": (config(128, 2, 256, 7), 8), "h768x1": (config(768, 12, 3072, 1), 2), "h384x2": (config(384, 6, 1536, 2), 3)}
# name -> (config, n_hidden): each named after the dispatch branch it forces (conv1d.hip: launch_engine<ENG_F32>, gloss.hip: the head
# groups of gloss_attn_kernel, the shared workspace row W = max(4 hidden, ffn))
EDGE_CFGS = {
    # a head group of ONE head (nh = 1); ffn > 4 hidden: the workspace row is the feed-forward's, not q | k | v | ctx
    "h64_nh1_wideffn": (config(64, 1, 320, 2), 3),
    # nh = 3; ffn = 200: C_out_pad = 224 of intermediate.dense and C_in_pad = 256 of output.dense are padded, ffn % 32 != 0
    "h192_nh3_pad": (config(192, 3, 200, 2), 3),
    # the first width whose 32-row tile of three bf16 planes (32 x (2 x 832 + 16) x 3 = 161,280 B) exceeds the short kernel's 150 KB:
    # q | k | v, the output projection and the GELU layer on conv1d_cl_kernel<ENG_F32>; head groups 4 + 4 + 4 + 1; output.dense
    # (C_in = 256) on the short kernel
    "h832_generic": (config(832, 13, 256, 1), 2),
    # the generic kernel on all four contractions
    "h1024_generic": (config(1024, 16, 4096, 1), 2),
}
ALL_CFGS = {**CFGS, **EDGE_CFGS}
GOLDEN_CFG = config(128, 2, 256, 8)     # eight layers in the checkpoint, seven used: what the reference does with its twelve
GOLDEN_LENGTHS = (1, 2, 3, 5, 31, 64)

# every path of the attention kernel and the GEMM row seams in one call: sum = 229, no multiple of 32 or 128
MIXED_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64)

# row totals that END on a tile: 32 (the short kernel's and the generic kernel's small tile), 64 / 65 (the generic kernel's switch from
# 32 t x 128 co to 128 t x 64 co), 128 and 256 (its large tile); then calls whose longest gloss, which sizes the attention kernel's LDS
# tiles, has 2 and 33 tokens
SEAM_LENGTHS = ((32,), (64,), (64, 1), (64, 64), (63, 64, 64, 64, 1), (2, 1, 2), (33, 1, 32))


def id_sets(lengths, seed=SEED, vocab=VOCAB):
    """one id sequence per length; ids in [0, vocab)"""
    rng = np.random.default_rng([seed, 7])
    return [rng.integers(0, vocab, size=int(L)).astype(np.int64) for L in lengths]


def seeded_state(cfg, seed=SEED):
    """Hugging Face keyed float32 numpy weights of ``roformer.*`` (without the prefix) for cfg.  The projections keep the activations at
    O(1); the query / key weights have std 0.3 at hidden 128 (0.3 sqrt(128 / hidden) elsewhere: scores of std ~ 10), so that the softmax is
    far from uniform.  ``encoder.embed_positions.weight`` is NOT produced: it is the rotary table, not a weight to seed."""
    rng = np.random.default_rng([seed, cfg["hidden_size"], cfg["num_hidden_layers"]])
    H, Fi, E = cfg["hidden_size"], cfg["intermediate_size"], cfg["embedding_size"]
    n = lambda std, *shape: (rng.standard_normal(shape) * std).astype(np.float32)
    st = {"embeddings.word_embeddings.weight": n(0.15, cfg["vocab_size"], E),
          "embeddings.token_type_embeddings.weight": n(0.15, cfg["type_vocab_size"], E),
          "embeddings.LayerNorm.weight": 1 + n(0.1, H), "embeddings.LayerNorm.bias": n(0.05, H)}
    qk = 0.3 * np.sqrt(128.0 / H)
    for l in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{l}."
        for name, std in (("query", qk), ("key", qk), ("value", H ** -0.5)):
            st[p + f"attention.self.{name}.weight"] = n(std, H, H)
            st[p + f"attention.self.{name}.bias"] = n(0.1, H)
        st[p + "attention.output.dense.weight"] = n(H ** -0.5, H, H)
        st[p + "attention.output.dense.bias"] = n(0.1, H)
        st[p + "attention.output.LayerNorm.weight"] = 1 + n(0.1, H)
        st[p + "attention.output.LayerNorm.bias"] = n(0.05, H)
        st[p + "intermediate.dense.weight"] = n(H ** -0.5, Fi, H)
        st[p + "intermediate.dense.bias"] = n(0.1, Fi)
        st[p + "output.dense.weight"] = n(Fi ** -0.5, H, Fi)
        st[p + "output.dense.bias"] = n(0.1, H)
        st[p + "output.LayerNorm.weight"] = 1 + n(0.1, H)
        st[p + "output.LayerNorm.bias"] = n(0.05, H)
    return st


def hf_model(cfg, state, dtype):
    """RoFormerForMaskedLM of cfg with ``state`` under ``roformer.`` (needs transformers).  The MLM head keeps its initialisation (it is
    never computed into a hidden state) and the rotary table is left as the model made it."""
    import torch
    from transformers import RoFormerConfig, RoFormerForMaskedLM
    model = RoFormerForMaskedLM(RoFormerConfig(**cfg)).eval()
    params = dict(model.named_parameters())
    with torch.no_grad():
        for k, v in state.items():
            params["roformer." + k].copy_(torch.from_numpy(v))
    return model.to(dtype)


def hf_feat(model, ids, n_hidden=8):
    """the reference's get_encodings on one id sequence -> [L, H]"""
    import torch
    with torch.no_grad():
        inp = torch.as_tensor(np.asarray(ids, np.int64))[None]
        hs = model(input_ids=inp, output_hidden_states=True, return_dict=True)["hidden_states"]
        shallow = model.get_input_embeddings()(inp)[0]
        return torch.stack([shallow] + [h[0] for h in hs[0:n_hidden]]).mean(dim=0)
