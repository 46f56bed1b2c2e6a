"""The FFT-block shapes the tests run, each named after the branch it forces, the launch rules of libdicttts_hip.so restated in Python
(which kernel a layer of the stack runs at a given (B, T)), and the inputs of the seam cases (test infrastructure).

Rules restated (the constants are READ from the sources, so a change there moves this table and tests/test_fft_blocks_cpu.py fails):
  * conv1d.hip launch_engine / launch_short_policy: every FFT convolution is packed ENG_F32 with its three bf16 pieces beside it.  A layer
    runs conv1d_short_kernel on the three-piece engine ("short_x6") whenever its 32-row tile (31 + K rows x (C_in_pad * 2 + 16) B x 3
    planes) fits SHORT_LDS_KB; else conv1d_short_kernel on fp32 MFMA ("short_f32") when the fp32 tile (31 + K rows x (C_in_pad * 4 + 16) B)
    fits AND the batch has at most SHORT_TILES tiles of 32 rows (B * ceil(T / 32)); else the generic conv1d_cl_kernel ("generic").
  * ops.hip mha_launch: dk == MHX_DK -> mha_mfma_kernel ("mfma"), or mha_mfma_split_kernel ("mfma_split") when T > MHA_SPLIT_T; any other
    dk <= MHA_DK_MAX -> the scalar mha_kernel ("scalar").
"""
import os
import re

import numpy as np

from dict_tts_amd import synth

SEED = 4321
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dict_tts_amd", "csrc")


def _grab(text, pattern, what):
    m = re.search(pattern, text)
    if not m:
        raise AssertionError(f"tests/fft_shapes.py no longer finds {what} (pattern {pattern!r}): the launch rule changed, restate it here")
    return int(m.group(1))


_CONST = None


def constants():
    """the numbers of the launch rules, read from conv1d.hip and ops.hip"""
    global _CONST
    if _CONST is None:
        conv = open(os.path.join(CSRC, "conv1d.hip")).read()
        ops = open(os.path.join(CSRC, "ops.hip")).read()
        pol = conv[conv.index("static bool launch_short_policy"):conv.index("static hipError_t launch_engine")]
        mha = ops[ops.index("hipError_t mha_launch("):]
        mha = mha[:mha.index("\n}\n")]
        _CONST = {
            "SHORT_LDS_KB": _grab(pol, r"if \(lds > (\d+) \* 1024 \|\|", "the LDS limit of launch_short_policy"),
            "SHORT_TILES": _grab(pol, r"ENGINE != ENG_BF16X6 && \(long long\)p\.B \* \(\(p\.T_out \+ 31\) / 32\) > (\d+)\)\) return false",
                                 "the tile limit of launch_short_policy"),
            "MHX_DK": _grab(ops, r"constexpr int MHX_DK = (\d+),", "MHX_DK"),
            "MHA_DK_MAX": _grab(ops, r"MHA_DK_MAX = (\d+);", "MHA_DK_MAX"),
            "MHA_SPLIT_T": _grab(mha, r"if \(T > (\d+)\) \{", "the T switch of mha_launch"),
        }
        # the order of the rule itself: three-piece short kernel first, then the fp32 short kernel, then the generic one
        eng = conv[conv.index("static hipError_t launch_engine"):conv.index("hipError_t conv1d_launch")]
        a, b, c = (eng.find(s) for s in ("launch_short_policy<ENG_BF16X6>", "launch_short_policy<ENG_F32>", "launch_cfg<ENGINE"))
        if not 0 <= a < b < c:
            raise AssertionError("tests/fft_shapes.py: launch_engine no longer tries x6 short, f32 short, generic in that order")
        if "if (dk == MHX_DK) {" not in mha or "if (dk > MHA_DK_MAX) return hipErrorInvalidValue;" not in mha:
            raise AssertionError("tests/fft_shapes.py: mha_launch no longer dispatches on dk == MHX_DK / dk <= MHA_DK_MAX")
    return _CONST


def conv_kernel(C_in, K, B, T):
    """the kernel a stride-1 ENG_F32 convolution of C_in input channels and K taps runs at (B, T): 'short_x6' | 'short_f32' | 'generic'"""
    c = constants()
    C_in_pad = (C_in + 63) // 64 * 64 if C_in > 32 else 32          # pack_conv: CK = 64 above 32 channels
    rows = 31 + (K - 1) + 1
    if rows * (C_in_pad * 2 + 16) * 3 <= c["SHORT_LDS_KB"] * 1024:   # C_in_pad % 16 == 0 always: the three pieces are always packed
        return "short_x6"
    if rows * (C_in_pad * 4 + 16) <= c["SHORT_LDS_KB"] * 1024 and B * ((T + 31) // 32) <= c["SHORT_TILES"]:
        return "short_f32"
    return "generic"


def mha_kernel(hidden, heads, T):
    c = constants()
    dk = hidden // heads
    if dk == c["MHX_DK"]:
        return "mfma_split" if T > c["MHA_SPLIT_T"] else "mfma"
    assert dk <= c["MHA_DK_MAX"]
    return "scalar"


def kernels(shape, B, T):
    """{'qkv', 'o', 'ffn1', 'ffn2', 'mha'} -> the kernel each launch of one layer of `shape` runs at (B, T)"""
    C, K = shape["hidden"], shape["k"]
    return {"qkv": conv_kernel(C, 1, B, T), "o": conv_kernel(C, 1, B, T), "ffn1": conv_kernel(C, K, B, T),
            "ffn2": conv_kernel(4 * C, 1, B, T), "mha": mha_kernel(C, shape["heads"], T)}


# name -> model shape, the ragged utterances of its end-to-end case (padded to T; lengths around the 32-row tile and the 128-query
# tile), `repeat`: the same utterances that many times over in a second batch (the other side of the 256-tile limit for the two-sided
# entries, the bit-identity batch at hidden 192), and `expect`: the kernels the name promises, {launch: kernel} at B = len(lens) and,
# under 'big', at B = len(lens) * repeat
SHAPES = {
    "h192_heads2": dict(hidden=192, heads=2, k=9, layers=2, T=161, lens=(161, 129, 128, 97, 33, 1), repeat=15,
                        expect={"ffn1": "short_x6", "ffn2": "short_x6", "mha": "mfma_split"},
                        big={"ffn1": "short_x6", "ffn2": "short_x6", "qkv": "short_x6", "o": "short_x6"}),
    "h192_heads4-mha_dk48": dict(hidden=192, heads=4, k=9, layers=2, T=100, lens=(100, 65, 64, 31, 2), repeat=0,
                                 expect={"mha": "scalar", "ffn2": "short_x6"}),
    "h128_heads2-mha_dk64": dict(hidden=128, heads=2, k=9, layers=2, T=129, lens=(129, 128, 63, 17), repeat=0,
                                 expect={"mha": "scalar", "ffn2": "short_x6"}),
    "h256_heads4-mha_dk64-ffn2_f32_short_or_generic": dict(hidden=256, heads=4, k=9, layers=2, T=161, lens=(161, 160, 129, 128, 127, 96, 65, 33, 1),
                                                           repeat=5, expect={"mha": "scalar", "ffn1": "short_x6", "ffn2": "short_f32"},
                                                           big={"ffn1": "short_x6", "ffn2": "generic"}),
    "h384_heads4-mfma_c384-ffn2_generic": dict(hidden=384, heads=4, k=9, layers=2, T=100, lens=(100, 97, 64, 33, 7), repeat=0,
                                               expect={"mha": "mfma", "ffn1": "short_x6", "ffn2": "generic"}),
    "h768_heads8-ffn1_generic_gelu": dict(hidden=768, heads=8, k=9, layers=1, T=128, lens=(128, 127, 100, 97, 96, 65, 64, 63, 33, 32, 31, 2, 1),
                                          repeat=5, expect={"mha": "mfma", "qkv": "short_x6", "ffn1": "short_f32", "ffn2": "generic"},
                                          big={"ffn1": "generic", "ffn2": "generic"}),
    "h192_k1": dict(hidden=192, heads=2, k=1, layers=1, T=70, lens=(70, 64, 33, 1), repeat=0, expect={"ffn1": "short_x6"}),
    "h192_k3": dict(hidden=192, heads=2, k=3, layers=1, T=70, lens=(70, 64, 33, 1), repeat=0, expect={"ffn1": "short_x6"}),
    "h192_k13": dict(hidden=192, heads=2, k=13, layers=1, T=70, lens=(70, 64, 33, 5), repeat=0, expect={"ffn1": "short_x6"}),
}


def state_np(shape, seed=SEED, **kw):
    """the numpy state dict of a shape (synth.fft_blocks_state_dict), without the reference's dtype marker"""
    sd = synth.fft_blocks_state_dict(seed, shape["hidden"], layers=shape["layers"], kernel_size=shape["k"], **kw)
    sd.pop("embed_positions._float_tensor", None)
    return sd


def ragged(name, B_T_C, lens, scale=1.0):
    """fp32 [B, T, C] standard-normal input whose utterance b has lens[b] non-zero frames"""
    x = synth.randn(SEED, "fft." + name, B_T_C, scale)
    for b, n in enumerate(lens):
        x[b, n:] = 0
    return x


def shape_input(name):
    s = SHAPES[name]
    return ragged(name, (len(s["lens"]), s["T"], s["hidden"]), s["lens"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# The position seams (default shape, 1 layer, B = 3, T = 513): fft_positions_kernel scans an utterance in chunks of 256 frames (4 waves
# of 64 lanes) with a carry.
SEAM_SHAPE = dict(hidden=192, heads=2, k=9, layers=1)
SEAM_T = 513
SEAM_LENS = (513, 257, 256)
SEAM_ZERO = ((0, 0), (0, 63), (0, 64), (0, 255), (0, 256), (0, 511), (0, 512), (1, 256))   # (utterance, frame): first channel exactly 0
SEAM_EXTENT = (513, 300, 290)     # the explicit-mask case: non-zero extent of x, LONGER than the mask's lengths SEAM_LENS


def seam_input(explicit):
    """-> (x fp32 [3, 513, 192], lens or None): value-derived padding (lens None) or an explicit mask of lengths SEAM_LENS over an x whose
    non-zero frames go on to SEAM_EXTENT (the positions count them whatever the mask says)"""
    x = ragged("seam", (3, SEAM_T, 192), SEAM_EXTENT if explicit else SEAM_LENS)
    for b, t in SEAM_ZERO:
        x[b, t, 0] = 0.0
    if explicit:
        x[2, 270, 0] = 0.0            # a first-channel-zero frame BEHIND the mask's end and behind the chunk boundary
    return x, (np.array(SEAM_LENS, np.int64) if explicit else None)


def quiet_input():
    """the LayerNorm-eps case (no positional embedding, 1 layer): a few valid rows of amplitude 2e-3, whose variance (4e-6) is of the size of
    torch's eps 1e-5 — the only rows on which the eps is visible above the bounds"""
    lens = (70, 33)
    x = ragged("quiet", (2, 70, 192), lens)
    for b, t in ((0, 0), (0, 31), (0, 32), (0, 69), (1, 32)):
        x[b, t] *= np.float32(2e-3)
    return x, lens
