"""The teacher-forced FVAE posterior pass, the parts that need no GPU: the CPU restatement (tests/posterior_ref.py) against the
reference's own outputs (tests/golden/g12_posterior.npz, both cases) and the C ABI surface of the pass: the DTTS_OUT_POSTERIOR item of
dtts_text2mel_fetch and its host argument block."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import posterior_ref as pr
from dict_tts_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture
def eight_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", ["plain", "id"])
def test_restatement_matches_reference_golden_g12(golden_dir, eight_threads, case):
    from oracle import hifigan_ref as href
    g = np.load(os.path.join(golden_dir, "g12_posterior.npz"))
    b = {k: T(v) for k, v in pr.g12_batch().items()}
    assert np.array_equal(b["word_tokens"].numpy(), g["word_tokens"])
    m2w = pr.g12_mel2word(b["word_tokens"].numpy())
    assert np.array_equal(m2w, g["mel2word_in"]) and m2w.shape[1] % 4 != 0
    mels = pr.tgt_mels_for(m2w)
    assert np.allclose(pr.mels_fingerprint(mels), g["tgt_mels_fingerprint"], rtol=1e-12, atol=0)
    assert (m2w[pr.G12_HOLE[0], pr.G12_HOLE[1]:pr.G12_HOLE[2]] == 0).all()
    spk = pr.g12_speakers(case)
    if spk is not None:
        assert np.array_equal(spk, g[case + ".spk"])
    sd = href.fold_weight_norm({k: T(v) for k, v in pr.g12_state_dict(case).items()})
    r = pr.forward_posterior(sd, b["word_tokens"], (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]),
                             b["pron_modified"], T(mels), T(m2w), T(g[case + ".eps"]), form=pr.CASES[case]["form"],
                             spk=None if spk is None else T(spk))
    assert np.array_equal(r["x_mask"].numpy(), g[case + ".x_mask"])
    for k in ("mel_out", "z_p", "m_q", "logs_q", "dur"):
        want = g[case + "." + k]
        assert r[k].shape == want.shape, k
        err = np.abs(r[k].numpy() - want).max()
        # 1e-5 max-abs on unit-scale arrays; z_p of the synthetic flow reaches |57| (fp32 ulp 3.8e-6 there): the bound scales with it
        assert err <= 1e-5 * max(1.0, float(np.abs(want).max())), (k, err)
    kl, want = float(r["kl"]), float(g[case + ".kl"])
    assert abs(kl - want) <= 1e-6 * abs(want), (kl, want)


def test_posterior_on_a_null_handle_is_invalid():
    lib = abi.load_library()
    args = abi.PosteriorArgs(C.sizeof(abi.PosteriorArgs))
    assert lib.dtts_text2mel_fetch(None, abi.OUT_POSTERIOR, C.byref(args), None) == -22   # DTTS_E_INVAL


def test_posterior_argument_block_matches_the_header():
    """the pass is an item of dtts_text2mel_fetch (the ABI keeps its entry points); its argument block is declared in the header and
    mirrored field for field by abi.PosteriorArgs"""
    hdr = open(os.path.join(ROOT, "include", "dicttts_hip.h")).read()
    assert int(re.search(r"#define DTTS_OUT_POSTERIOR (\d+)", hdr).group(1)) == abi.OUT_POSTERIOR == 9
    body = re.search(r"typedef struct dtts_posterior_args \{(.*?)\} dtts_posterior_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?([a-z_0-9]+)$", r"\1", part.strip()) for part in decl.split(",")]
    assert names == [f[0] for f in abi.PosteriorArgs._fields_], names
    assert C.sizeof(abi.PosteriorArgs) == 4 * 4 + 7 * C.sizeof(C.c_void_p)
    assert "dtts_text2mel_posterior" not in abi.EXPORTS


def test_training_still_refused_before_the_gpu_is_touched():
    """infer=False without tgt_mels keeps the old refusal; the message now names what does run"""
    src = open(os.path.join(ROOT, "dict_tts_amd", "model.py")).read()
    assert "gradients (training) are not implemented" in src
