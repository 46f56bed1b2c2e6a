"""ResBlock2 generators (``resblock: "2"``, the V3 family) on the CPU: the configuration encoding, the float64 reference against the
golden taken from the reference implementation (tests/golden/g13_hifigan_rb2.npz, tools/make_golden_rb2.py), the synthetic state dict,
and the rounding emulator with planted defects against the bounds the GPU test applies."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import rb2x_shapes
import resblock2_ref as r2
from dict_tts_amd import abi, hparams as hp, synth, vocoder
from oracle import hifigan_ref as href
from resblock2_emul import BOUNDS_RB2, Emulator2
from vocoder_emul import BOUNDS, Emulator, seam_check

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
rms = lambda a: float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))
V3 = synth.hifigan_config_v3()


@pytest.fixture(scope="module")
def gen():
    return V3, href.fold_weight_norm({k: T(v) for k, v in synth.hifigan_state_dict(gc.SEED, cfg=V3).items()})


# ------------------------------------------------------------------------------------------------ configuration
def test_v3_config_is_the_released_one():
    assert V3 == hp.HIFIGAN_V3 == {"resblock": "2", "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8],
                                   "upsample_initial_channel": 256, "resblock_kernel_sizes": [3, 5, 7],
                                   "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]]}


@pytest.mark.parametrize("resblock", ["2", 2])
def test_fill_abi_config_encodes_resblock2_rows(resblock):
    cfg = hp.fill_abi_config(abi.default_config(), None, {**V3, "resblock": resblock})
    assert cfg.n_upsamples == 3 and list(cfg.upsample_rates)[:3] == [8, 8, 4] and list(cfg.upsample_kernel_sizes)[:3] == [16, 16, 8]
    assert cfg.upsample_initial_channel == 256 and cfg.n_resblock_kernels == 3 and list(cfg.resblock_kernel_sizes)[:3] == [3, 5, 7]
    assert [list(r) for r in cfg.resblock_dilation_sizes][:3] == [[1, 2, 0], [2, 6, 0], [3, 12, 0]]   # third entry 0 = a two-dilation row
    assert abi.C.sizeof(abi.DttsConfig) == abi.load_library().dtts_config_sizeof()


def test_fill_abi_config_resblock1_is_unchanged():
    want = abi.default_config()
    for voc in (synth.hifigan_config(), hp.HIFIGAN_DEFAULTS, {**synth.hifigan_config(), "resblock": 1}):
        got = hp.fill_abi_config(abi.default_config(), None, voc)
        assert bytes(got) == bytes(want)


def test_fill_abi_config_names_the_key_in_its_errors():
    with pytest.raises(NotImplementedError, match="resblock_dilation_sizes.*exactly 2"):
        hp.fill_abi_config(abi.default_config(), None, {**V3, "resblock_dilation_sizes": [[1, 2, 3]] * 3})
    with pytest.raises(NotImplementedError, match="resblock_dilation_sizes.*exactly 3"):
        hp.fill_abi_config(abi.default_config(), None, {**synth.hifigan_config(), "resblock_dilation_sizes": [[1, 2]] * 3})
    with pytest.raises(NotImplementedError, match="resblock"):
        hp.fill_abi_config(abi.default_config(), None, {**V3, "resblock": "3"})


def test_dtts_create_checks_the_rows_before_it_looks_for_a_device():
    lib = abi.load_library()

    def create(cfg):
        h = abi.C.c_void_p()
        rc = lib.dtts_create(abi.C.byref(cfg), abi.C.byref(h))
        msg = lib.dtts_last_error(None).decode()
        if rc == 0:
            lib.dtts_destroy(h)
        return rc, msg
    mixed = hp.fill_abi_config(abi.default_config(), None, V3)
    mixed.resblock_dilation_sizes[1][2] = 5
    rc, msg = create(mixed)
    assert rc == -22 and "resblock_dilation_sizes" in msg, (rc, msg)
    bad = hp.fill_abi_config(abi.default_config(), None, V3)
    bad.resblock_dilation_sizes[0][1] = 0
    rc, msg = create(bad)
    assert rc == -22 and "resblock_dilation_sizes" in msg, (rc, msg)
    for cfg in (hp.fill_abi_config(abi.default_config(), None, V3), abi.default_config()):   # past that check: created, or no device
        rc, msg = create(cfg)
        assert rc != -22, (rc, msg)
        if not torch.cuda.is_available():
            assert "no HIP device" in msg


def test_config_json_generator_v1_layout_with_a_resblock2_config(tmp_path):
    """vocoders/hifigan.py:19-25: the original HifiGAN layout, config.json + generator_v1 with the state under the key generator"""
    sd = {k: T(v) for k, v in synth.hifigan_state_dict(gc.SEED, cfg=V3).items()}
    (tmp_path / "config.json").write_text(json.dumps({**V3, "num_mels": 80, "sampling_rate": 22050}))
    torch.save({"generator": sd}, str(tmp_path / "generator_v1"))
    config, state = vocoder.find_vocoder_checkpoint(str(tmp_path))
    assert sorted(state) == sorted(sd) and all(torch.equal(state[k], sd[k]) for k in sd)
    cfg = hp.fill_abi_config(abi.default_config(), None, {**hp.HIFIGAN_DEFAULTS, **config})
    assert [list(r) for r in cfg.resblock_dilation_sizes][:3] == [[1, 2, 0], [2, 6, 0], [3, 12, 0]] and cfg.n_upsamples == 3


# ------------------------------------------------------------------------------------------------ weights
RB1_SHA = {
    "conv_post.bias": "7763332acc", "conv_post.weight_g": "0c1be985b7", "conv_post.weight_v": "9200675ca5", "conv_pre.bias": "915e3daafd",
    "conv_pre.weight_g": "596ced918d", "conv_pre.weight_v": "72e9e8cf3e", "resblocks.0.convs1.0.bias": "d961fb3d33", "resblocks.0.convs1.0.weight_g":
    "92097a7e83", "resblocks.0.convs1.0.weight_v": "bb2b07a749", "resblocks.0.convs1.1.bias": "ad01931096", "resblocks.0.convs1.1.weight_g":
    "b33685351f", "resblocks.0.convs1.1.weight_v": "597a99846f", "resblocks.0.convs1.2.bias": "82d8d1d04d", "resblocks.0.convs1.2.weight_g":
    "b9693674db", "resblocks.0.convs1.2.weight_v": "aff10753b5", "resblocks.0.convs2.0.bias": "64340f4f92", "resblocks.0.convs2.0.weight_g":
    "38f43a534d", "resblocks.0.convs2.0.weight_v": "bbfdcf8e3d", "resblocks.0.convs2.1.bias": "03604d1440", "resblocks.0.convs2.1.weight_g":
    "df30072b39", "resblocks.0.convs2.1.weight_v": "bd4ee7d458", "resblocks.0.convs2.2.bias": "67a5a9503f", "resblocks.0.convs2.2.weight_g":
    "bf2005f386", "resblocks.0.convs2.2.weight_v": "24297281ab", "resblocks.1.convs1.0.bias": "1bcec33332", "resblocks.1.convs1.0.weight_g":
    "2a6c86dd7c", "resblocks.1.convs1.0.weight_v": "fb2df79443", "resblocks.1.convs1.1.bias": "4248eca114", "resblocks.1.convs1.1.weight_g":
    "43f6374e67", "resblocks.1.convs1.1.weight_v": "749e1b7ac7", "resblocks.1.convs1.2.bias": "2816bd2396", "resblocks.1.convs1.2.weight_g":
    "9e4b7e4b8a", "resblocks.1.convs1.2.weight_v": "d06f30ea2c", "resblocks.1.convs2.0.bias": "b7c0ecd3cf", "resblocks.1.convs2.0.weight_g":
    "d5a4ce4fd8", "resblocks.1.convs2.0.weight_v": "24cf8b89ff", "resblocks.1.convs2.1.bias": "e088f90589", "resblocks.1.convs2.1.weight_g":
    "909e72ddda", "resblocks.1.convs2.1.weight_v": "984b5cb7f3", "resblocks.1.convs2.2.bias": "bae9250e4a", "resblocks.1.convs2.2.weight_g":
    "7ab2d09b0e", "resblocks.1.convs2.2.weight_v": "de45480be5", "resblocks.10.convs1.0.bias": "75be32700f", "resblocks.10.convs1.0.weight_g":
    "4f7eafaa69", "resblocks.10.convs1.0.weight_v": "e9ae1499d6", "resblocks.10.convs1.1.bias": "571b51c04a", "resblocks.10.convs1.1.weight_g":
    "7d42ff7e62", "resblocks.10.convs1.1.weight_v": "92adfad13d", "resblocks.10.convs1.2.bias": "a19f035b2c", "resblocks.10.convs1.2.weight_g":
    "5294d88321", "resblocks.10.convs1.2.weight_v": "b015b2c187", "resblocks.10.convs2.0.bias": "99785aedf9", "resblocks.10.convs2.0.weight_g":
    "a73f7503cc", "resblocks.10.convs2.0.weight_v": "9eabc08073", "resblocks.10.convs2.1.bias": "4a518e201c", "resblocks.10.convs2.1.weight_g":
    "daf66f3775", "resblocks.10.convs2.1.weight_v": "426b993a77", "resblocks.10.convs2.2.bias": "6341479eee", "resblocks.10.convs2.2.weight_g":
    "717834e079", "resblocks.10.convs2.2.weight_v": "d0b184af86", "resblocks.11.convs1.0.bias": "020c610bc0", "resblocks.11.convs1.0.weight_g":
    "1bc721a5b9", "resblocks.11.convs1.0.weight_v": "ba4acc1656", "resblocks.11.convs1.1.bias": "ea8f8b776b", "resblocks.11.convs1.1.weight_g":
    "e134184420", "resblocks.11.convs1.1.weight_v": "ac00496421", "resblocks.11.convs1.2.bias": "505beb375b", "resblocks.11.convs1.2.weight_g":
    "92b1b28060", "resblocks.11.convs1.2.weight_v": "8d5fb23d06", "resblocks.11.convs2.0.bias": "836a1aba15", "resblocks.11.convs2.0.weight_g":
    "909e4a556f", "resblocks.11.convs2.0.weight_v": "ec29b416a4", "resblocks.11.convs2.1.bias": "04ea7d2c23", "resblocks.11.convs2.1.weight_g":
    "5ac4564186", "resblocks.11.convs2.1.weight_v": "d36b6ddb72", "resblocks.11.convs2.2.bias": "0f3a2cdf25", "resblocks.11.convs2.2.weight_g":
    "549366f04e", "resblocks.11.convs2.2.weight_v": "f1e961ea10", "resblocks.2.convs1.0.bias": "dd2e34bd6b", "resblocks.2.convs1.0.weight_g":
    "02617b33c5", "resblocks.2.convs1.0.weight_v": "72ba0c5142", "resblocks.2.convs1.1.bias": "44487c7509", "resblocks.2.convs1.1.weight_g":
    "33d3584c1a", "resblocks.2.convs1.1.weight_v": "a570192b11", "resblocks.2.convs1.2.bias": "0ee5d3dd35", "resblocks.2.convs1.2.weight_g":
    "81e239f877", "resblocks.2.convs1.2.weight_v": "f4b62a39d0", "resblocks.2.convs2.0.bias": "201cca5540", "resblocks.2.convs2.0.weight_g":
    "ff2865a143", "resblocks.2.convs2.0.weight_v": "02ea5d62ad", "resblocks.2.convs2.1.bias": "9e875ec37e", "resblocks.2.convs2.1.weight_g":
    "eb3a122019", "resblocks.2.convs2.1.weight_v": "e0b7121bcd", "resblocks.2.convs2.2.bias": "91644c747a", "resblocks.2.convs2.2.weight_g":
    "188dc3a199", "resblocks.2.convs2.2.weight_v": "1aa99d03a5", "resblocks.3.convs1.0.bias": "313a61658c", "resblocks.3.convs1.0.weight_g":
    "927312ec22", "resblocks.3.convs1.0.weight_v": "8843f9b9c7", "resblocks.3.convs1.1.bias": "dcc4a6760f", "resblocks.3.convs1.1.weight_g":
    "298d35386f", "resblocks.3.convs1.1.weight_v": "bf538c6e4a", "resblocks.3.convs1.2.bias": "c79f400576", "resblocks.3.convs1.2.weight_g":
    "531a791113", "resblocks.3.convs1.2.weight_v": "150f1a07ee", "resblocks.3.convs2.0.bias": "c93a6399a9", "resblocks.3.convs2.0.weight_g":
    "e60688a339", "resblocks.3.convs2.0.weight_v": "9dd2053eea", "resblocks.3.convs2.1.bias": "8dcc7f6a91", "resblocks.3.convs2.1.weight_g":
    "02aa6c84d8", "resblocks.3.convs2.1.weight_v": "07824798ea", "resblocks.3.convs2.2.bias": "345445a327", "resblocks.3.convs2.2.weight_g":
    "81d0a07f49", "resblocks.3.convs2.2.weight_v": "6ee52df311", "resblocks.4.convs1.0.bias": "d8c102e1b7", "resblocks.4.convs1.0.weight_g":
    "1e050fc16f", "resblocks.4.convs1.0.weight_v": "9c7ad5e043", "resblocks.4.convs1.1.bias": "d1234580d0", "resblocks.4.convs1.1.weight_g":
    "6ec0603660", "resblocks.4.convs1.1.weight_v": "f59a4d9a14", "resblocks.4.convs1.2.bias": "7ee199eb0c", "resblocks.4.convs1.2.weight_g":
    "0edf41c063", "resblocks.4.convs1.2.weight_v": "5742061d8c", "resblocks.4.convs2.0.bias": "3361543215", "resblocks.4.convs2.0.weight_g":
    "586fd40af2", "resblocks.4.convs2.0.weight_v": "993b16977a", "resblocks.4.convs2.1.bias": "7470f6be54", "resblocks.4.convs2.1.weight_g":
    "11e5381c5b", "resblocks.4.convs2.1.weight_v": "33d2c5acf7", "resblocks.4.convs2.2.bias": "6827d1558d", "resblocks.4.convs2.2.weight_g":
    "2279ff387e", "resblocks.4.convs2.2.weight_v": "396135e22d", "resblocks.5.convs1.0.bias": "f15525a620", "resblocks.5.convs1.0.weight_g":
    "3ad032980a", "resblocks.5.convs1.0.weight_v": "50223b5a46", "resblocks.5.convs1.1.bias": "133dbfcce2", "resblocks.5.convs1.1.weight_g":
    "7a1f0ca3a5", "resblocks.5.convs1.1.weight_v": "c06adaeee4", "resblocks.5.convs1.2.bias": "0be251c04d", "resblocks.5.convs1.2.weight_g":
    "54a01119c0", "resblocks.5.convs1.2.weight_v": "70efd8ea6b", "resblocks.5.convs2.0.bias": "3fbe74257d", "resblocks.5.convs2.0.weight_g":
    "05eba86343", "resblocks.5.convs2.0.weight_v": "3a837e9669", "resblocks.5.convs2.1.bias": "6a6984367c", "resblocks.5.convs2.1.weight_g":
    "e84a839538", "resblocks.5.convs2.1.weight_v": "ea7d0d18c4", "resblocks.5.convs2.2.bias": "96ebaef28d", "resblocks.5.convs2.2.weight_g":
    "77cfbbda35", "resblocks.5.convs2.2.weight_v": "7098bfba61", "resblocks.6.convs1.0.bias": "a8ab0c610d", "resblocks.6.convs1.0.weight_g":
    "4e24edd756", "resblocks.6.convs1.0.weight_v": "cb9d587ee2", "resblocks.6.convs1.1.bias": "fff73b78c7", "resblocks.6.convs1.1.weight_g":
    "ba580e8e92", "resblocks.6.convs1.1.weight_v": "076d4ce9be", "resblocks.6.convs1.2.bias": "cffea6ddf4", "resblocks.6.convs1.2.weight_g":
    "49ac418eb6", "resblocks.6.convs1.2.weight_v": "ae8a2d08e6", "resblocks.6.convs2.0.bias": "9f27868a0d", "resblocks.6.convs2.0.weight_g":
    "5675f27db1", "resblocks.6.convs2.0.weight_v": "95fcb3b6cd", "resblocks.6.convs2.1.bias": "be2cc1f25e", "resblocks.6.convs2.1.weight_g":
    "b49c25f924", "resblocks.6.convs2.1.weight_v": "da1b7cc573", "resblocks.6.convs2.2.bias": "e9cf2c1365", "resblocks.6.convs2.2.weight_g":
    "20852142a7", "resblocks.6.convs2.2.weight_v": "f449319f5a", "resblocks.7.convs1.0.bias": "ad876bed7c", "resblocks.7.convs1.0.weight_g":
    "e34c92c398", "resblocks.7.convs1.0.weight_v": "7e660861aa", "resblocks.7.convs1.1.bias": "e9dc5489f4", "resblocks.7.convs1.1.weight_g":
    "6a9246235c", "resblocks.7.convs1.1.weight_v": "2572b86772", "resblocks.7.convs1.2.bias": "3d955ea056", "resblocks.7.convs1.2.weight_g":
    "748923206f", "resblocks.7.convs1.2.weight_v": "789c4556c4", "resblocks.7.convs2.0.bias": "3104adb746", "resblocks.7.convs2.0.weight_g":
    "cf7859d4d1", "resblocks.7.convs2.0.weight_v": "add7fe608b", "resblocks.7.convs2.1.bias": "4269121b3c", "resblocks.7.convs2.1.weight_g":
    "1a2a0c45de", "resblocks.7.convs2.1.weight_v": "4b66679f9b", "resblocks.7.convs2.2.bias": "911d54ed6b", "resblocks.7.convs2.2.weight_g":
    "d2a1a9668f", "resblocks.7.convs2.2.weight_v": "ac6c274010", "resblocks.8.convs1.0.bias": "476de4dc09", "resblocks.8.convs1.0.weight_g":
    "7beccaec82", "resblocks.8.convs1.0.weight_v": "1cc74b4f52", "resblocks.8.convs1.1.bias": "4682e67bb9", "resblocks.8.convs1.1.weight_g":
    "72cf1070cf", "resblocks.8.convs1.1.weight_v": "39899d36ea", "resblocks.8.convs1.2.bias": "220f2e1114", "resblocks.8.convs1.2.weight_g":
    "6fb5c00025", "resblocks.8.convs1.2.weight_v": "2381be959c", "resblocks.8.convs2.0.bias": "5cef2d1584", "resblocks.8.convs2.0.weight_g":
    "27116fea29", "resblocks.8.convs2.0.weight_v": "c7a655db5b", "resblocks.8.convs2.1.bias": "60f8f8d849", "resblocks.8.convs2.1.weight_g":
    "7ed64335e6", "resblocks.8.convs2.1.weight_v": "02db0b2c3c", "resblocks.8.convs2.2.bias": "89b838b972", "resblocks.8.convs2.2.weight_g":
    "de86ce2f41", "resblocks.8.convs2.2.weight_v": "9e86ff295e", "resblocks.9.convs1.0.bias": "01c0e7c7c9", "resblocks.9.convs1.0.weight_g":
    "88febbfa94", "resblocks.9.convs1.0.weight_v": "4f10555e81", "resblocks.9.convs1.1.bias": "660592ecf1", "resblocks.9.convs1.1.weight_g":
    "b875755c69", "resblocks.9.convs1.1.weight_v": "9c907a44a3", "resblocks.9.convs1.2.bias": "9d402939e5", "resblocks.9.convs1.2.weight_g":
    "415193cd9c", "resblocks.9.convs1.2.weight_v": "1c2e51c962", "resblocks.9.convs2.0.bias": "82ec6823c2", "resblocks.9.convs2.0.weight_g":
    "78531a9363", "resblocks.9.convs2.0.weight_v": "bf9b5c28ae", "resblocks.9.convs2.1.bias": "f71d712001", "resblocks.9.convs2.1.weight_g":
    "7f3c572a45", "resblocks.9.convs2.1.weight_v": "a2247fdb05", "resblocks.9.convs2.2.bias": "2f30126897", "resblocks.9.convs2.2.weight_g":
    "f0f8d750ea", "resblocks.9.convs2.2.weight_v": "9c610ed4ed", "ups.0.bias": "04831d89ed", "ups.0.weight_g": "b8e189cb7b", "ups.0.weight_v":
    "493fbe34cb", "ups.1.bias": "03de4c2574", "ups.1.weight_g": "ef8c6ce285", "ups.1.weight_v": "7a649952d8", "ups.2.bias": "45bab72ab5",
    "ups.2.weight_g": "a4fb62aeee", "ups.2.weight_v": "3e856bac94", "ups.3.bias": "a1e6a9e546", "ups.3.weight_g": "c611ca11c9", "ups.3.weight_v":
    "9bba7475e9"
}   # sha256(tensor bytes)[:10] of synth.hifigan_state_dict(1234) on the parent of the commit that added ResBlock2


def test_synthetic_state_dict_names_and_unchanged_resblock1_tensors(golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_hifigan_rb2.npz"))
    assert sorted(synth.hifigan_state_dict(gc.SEED, cfg=V3)) == [str(n) for n in g["state_dict_names"]]
    sd = synth.hifigan_state_dict(1234)
    assert sorted(sd) == sorted(RB1_SHA)
    for k, v in sd.items():
        assert hashlib.sha256(v.tobytes()).hexdigest()[:10] == RB1_SHA[k], k


# ------------------------------------------------------------------------------------------------ the float64 reference
def test_float64_reference_reproduces_g13(gen, golden_dir):
    """the tolerances of tests/test_oracle_golden.py::test_g6_hifigan: 2e-5 on waveform and stage heads, 1e-6 on folded weights"""
    cfg, fsd = gen
    g = np.load(os.path.join(golden_dir, "g13_hifigan_rb2.npz"))
    close = lambda a, b, tol: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) <= tol
    for name in ("conv_pre.weight", "ups.0.weight", "resblocks.0.convs.0.weight", "resblocks.8.convs.1.weight"):
        assert close(fsd[name][:8], g[f"folded.{name}.head"], 1e-6), name
    mel = gc.g6_mel()
    with torch.no_grad():
        wav, stages = r2.generator_forward(fsd, cfg, T(mel).unsqueeze(0).transpose(2, 1), return_stages=True)
    for name in [f"ups.{i}" for i in range(3)] + [f"rb.{n}" for n in range(9)] + ["post"]:
        assert close(stages[name][0, :, :64], g[name + ".head"], 2e-5), name
        assert abs(float(stages[name].pow(2).mean().sqrt()) - float(g[name + ".rms"])) <= 2e-5, name
    assert close(wav.view(-1), g["wav"], 2e-5) and wav.shape[-1] == 32 * 256
    assert close(r2.spec2wav(fsd, cfg, mel), g["wav"], 2e-5)
    assert float(np.mean(np.abs(g["wav"]) > 0.9)) == 0.0   # the reference alone stays inside the GPU test's saturation cap


# ------------------------------------------------------------------------------------------------ the emulator
ISO = {"resblock": "2", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": 128,
       "resblock_kernel_sizes": [3, 5, 7], "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]]}


@pytest.mark.parametrize("which", ["v3", "iso"])
def test_emulator_without_rounding_is_the_float64_reference(gen, which):
    cfg, fsd = gen
    if which == "iso":
        cfg = ISO
        fsd = href.fold_weight_norm({k: T(v) for k, v in synth.hifigan_state_dict(gc.SEED, cfg=cfg).items()})
    mel = T(gc.g6_mel()).T.unsqueeze(0).double()
    with torch.no_grad():
        want = r2.generator_forward(fsd, cfg, mel)
    got = Emulator2(fsd, cfg, rounding=False).forward(mel)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-12


def test_emulator_waveform_error_is_inside_the_gate(gen):
    """BASELINE.json north_star: RMS(gpu - ref) <= 1e-4 in the f16 mode.  Emulated on the synthetic V3 weights: 9.4e-5 / 9.6e-5 / 9.7e-5
    on three mels — NOT a third of ResBlock1's 6.0-6.9e-5 although the chain is a third as deep.  Where it comes from (each source
    switched on alone): the serial convolutions' split operands 0.0e-5; fp16 operands of the LAST stage's three ResBlocks alone 6.0e-5
    (every rounding there reaches conv_post directly, x has RMS 2.1-2.4); fp16 activations of all stages with exact weights 6.9e-5, the
    fp16 weights the rest.  The error is set by the last stage, not by the depth; the synthetic ResBlock2 convolutions have gain 1.0
    where ResBlock1's second convolutions have 0.6."""
    cfg, fsd = gen
    for mel in (gc.g6_mel(), synth.random_mel(31, 72, "s16_0")):
        ref = r2.spec2wav(fsd, cfg, mel)
        w16 = Emulator2(fsd, cfg).spec2wav(mel)
        e16, eb = rms(w16 - ref), rms(Emulator2(fsd, cfg, mode="bf16").spec2wav(mel) - ref)
        print(f"emulated waveform error: f16 {e16:.3e}  bf16 {eb:.3e}")
        assert e16 <= 1e-4 and abs(rms(w16) - rms(ref)) <= 1e-4 and 1e-4 < eb < 5e-3


@pytest.mark.parametrize("mode", ["f16", "bf16"])
@pytest.mark.parametrize("defect", ["halo", "stale", "no_res0", "rb1_order"])
def test_planted_defects_exceed_the_gpu_bounds(gen, mode, defect):
    """each restatement error a fused ResBlock2 kernel could make moves the waveform beyond the bounds the GPU test applies against this
    emulator — on the full V3 generator (group full_*) and on a one-stage isolating generator (group f16 / bf16).  If one does not, the
    bounds are too loose."""
    cfg, fsd = gen
    mel = synth.random_mel(77, 24, "defect")
    for name, c, s, group in (("v3", cfg, fsd, "full_" + mode),
                              ("iso", ISO, href.fold_weight_norm({k: T(v) for k, v in synth.hifigan_state_dict(gc.SEED, cfg=ISO).items()}), mode)):
        clean = Emulator2(s, c, mode=mode).spec2wav(mel)
        # the halo defect sits at the seams of the kernel's own tiles: a seam must fall inside the utterance
        tile = 32 if name == "iso" else 1024
        broken = Emulator2(s, c, mode=mode, defect=defect, tile=tile).spec2wav(mel)
        vals, fails = seam_check(broken, clean, BOUNDS_RB2[group])
        print(f"{name} {mode} {defect}: {vals}")
        assert fails, f"{name} / {mode} / {defect}: {vals} stays inside {BOUNDS_RB2[group]}: the bounds are too loose"


def test_bounds_do_not_exceed_resblock1s():
    for g, b in BOUNDS_RB2.items():
        assert all(b[k] <= BOUNDS[g][k] for k in b), g


# ------------------------------------------------------------------------------------------------ the tile rule
def test_tile_rule_of_the_v3_kernels():
    """halo = (K - 1) / 2 * (d0 + d1): 3, 16 and 45 rows for V3's three kernels; every V3 (C, K, d0, d1) is admitted at all four widths"""
    assert [rb2x_shapes.halo(k, *d) for k, d in zip(V3["resblock_kernel_sizes"], V3["resblock_dilation_sizes"])] == [3, 16, 45]
    for C in (32, 64, 128, 256):
        for k, d in zip(V3["resblock_kernel_sizes"], V3["resblock_dilation_sizes"]):
            assert rb2x_shapes.supported(C, k, *d)
    assert not rb2x_shapes.supported(64, 4, 1, 1) and not rb2x_shapes.supported(48, 3, 1, 1) and not rb2x_shapes.supported(256, 11, 3, 12)
    text = open(os.path.join(os.path.dirname(__file__), "..", "dict_tts_amd", "csrc", "rb2x.h")).read()
    assert "(K - 1) / 2 * (d0 + d1)" in text and "(K + 1) / 2 * (d0 > d1 ? d0 : d1)" in text
