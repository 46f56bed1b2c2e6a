"""tests/golden/g18_gloss.npz: the reference's ``get_encodings`` on seeded weights, from Hugging Face's ``RoFormerForMaskedLM`` in float64
(needs ``transformers``).  Inputs are regenerated from tests/gloss_shapes.py; the file stores the ids, their offsets and the expected
``feat`` only.

    python tools/make_golden_gloss.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gloss_shapes as S  # noqa: E402


def main():
    import transformers
    cfg = S.GOLDEN_CFG
    model = S.hf_model(cfg, S.seeded_state(cfg), torch.float64)
    ids = S.id_sets(S.GOLDEN_LENGTHS)
    feat = np.concatenate([S.hf_feat(model, i, 8).numpy() for i in ids])
    off = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "g18_gloss.npz")
    np.savez_compressed(out, ids=np.concatenate(ids), tok_off=off, feat=feat, seed=np.int64(S.SEED), transformers=np.array(transformers.__version__))
    print(f"{out}: {feat.shape} float64, {os.path.getsize(out)} bytes (transformers {transformers.__version__})")


if __name__ == "__main__":
    main()
