"""The polyphase upsamplers of the vocoder: the forms the library accepts, the case table of tests/test_upsampler_forms_{cpu,gpu}.py, and the
rules that decide how an upsampler runs, restated from dict_tts_amd/csrc/pack.hip (pack_transposed) and vconv.hip (vconv_launch) for the tests
that build shapes from them.

A ConvTranspose1d(2 ch -> ch, kernel k, stride u, padding (k - u) / 2) is packed as an ordinary convolution with u * ch output channels
(phase-major) over the input offsets delta in {-1, 0, +1}:   out[u q + r][co] = b[co] + sum_delta sum_ci x[q + delta][ci] w[ci][co][r + p - u delta].
Accepted: u <= k <= 2 u with k - u even (exactly T * u output rows).  Three forms:
  single   k == u (p = 0): one tap, K = 1, pad = 0
  half     k == 2 u, 2 p == u and (u ch / 2) % wave_ch == 0: three taps of which every wave skips one (vconv.hip poly_half)
  general  everything else: all three taps contracted, the weight taken where r + p - u delta lies in [0, k)
"""
import torch

RB_KERNELS = [3, 7, 11]
RB_DILATIONS = [[1, 3, 5]] * 3


# ------------------------------------------------------------------------------------------------ pack.hip pack_transposed
def accepted(u, k):
    """pack.hip pack_transposed: what dtts_finalize_weights accepts (every precision)"""
    return u >= 1 and u <= k <= 2 * u and (k - u) % 2 == 0


def polyphase_form(u, k, c_out):
    assert accepted(u, k), (u, k)
    p = (k - u) // 2
    if k == u and p == 0:
        return "single"
    cop = u * c_out
    wave_ch = 64 if cop % 256 == 0 else 32   # channels per wave of the vconv configuration the layer gets
    if k == 2 * u and 2 * p == u and (cop // 2) % wave_ch == 0:
        return "half"
    return "general"


def pad32(c):
    return (c + 31) // 32 * 32   # pack.hip pack_conv: C_in_pad / C_out_pad


# ------------------------------------------------------------------------------------------------ vconv.hip vconv_launch
# every instantiation vconv_launch can return, (MT, NT, WT, WC, CK, X3); `vlaunch<..>` in the source stands for both values of X3
ALL_BRANCHES = {
    (2, 2, 1, 4, 64, True), (2, 2, 1, 4, 128, True),
    (4, 2, 1, 4, 128, True), (4, 2, 1, 4, 128, False), (4, 2, 1, 4, 64, True), (4, 2, 1, 4, 64, False), (4, 2, 1, 4, 32, True), (4, 2, 1, 4, 32, False),
    (2, 1, 1, 4, 64, True), (2, 1, 1, 4, 128, True), (2, 1, 2, 2, 64, True), (2, 1, 2, 2, 128, True),
    (4, 1, 1, 4, 128, True), (4, 1, 1, 4, 128, False), (4, 1, 1, 4, 64, True), (4, 1, 1, 4, 64, False), (4, 1, 1, 4, 32, True), (4, 1, 1, 4, 32, False),
    (4, 1, 2, 2, 64, True), (4, 1, 2, 2, 64, False), (4, 1, 2, 2, 32, True), (4, 1, 2, 2, 32, False),
    (4, 1, 4, 1, 64, True), (4, 1, 4, 1, 64, False), (4, 1, 4, 1, 32, True), (4, 1, 4, 1, 32, False),
}
# the instantiations no upsampler of a generator with upsample_initial_channel in {16 .. 512} and u <= 8 reaches, and why
NOT_AN_UPSAMPLER = {
    (2, 2, 1, 4, 64, True): "text-to-mel: the prior flow's conditioning convolution, ci == 192",
    (2, 1, 1, 4, 64, True): "text-to-mel: the decoder WaveNet layers, gate_H / split",
    (2, 1, 2, 2, 128, True): "text-to-mel: the strided g_pre_net, in_half",
    (4, 2, 1, 4, 32, True): "co % 256 == 0 over ci == 32: a 32-channel input means <= 16 output channels per phase, 8 * 16 = 128 at most",
    (4, 2, 1, 4, 32, False): "co % 256 == 0 over ci == 32: a 32-channel input means <= 16 output channels per phase, 8 * 16 = 128 at most",
    (4, 1, 1, 4, 128, True): "split operands on 128-row tiles: the upsamplers of DTTS_VOC_F16 set small_tiles and take the 64-row form (conv_pre runs here)",
    (4, 1, 2, 2, 64, True): "split operands on 256-row tiles: the upsamplers of DTTS_VOC_F16 set small_tiles and take the 128-row form",
}


def vconv_config(c_out_pad, c_in_pad, exact, small_tiles):
    """vconv_launch for an upsampler's call (no gate_H / split / in_half / h2): -> ((MT, NT, WT, WC, CK, X3), TT) with TT = 32 MT WT the input
    rows per tile.  exact: DTTS_VOC_F16 (fp32 input, split operands: the X3 instantiations); small_tiles: VConvParams::small_tiles"""
    co, ci, x3 = c_out_pad, c_in_pad, bool(exact)
    assert co % 32 == 0 and ci % 32 == 0
    ck = lambda: 128 if ci % 128 == 0 else (64 if ci % 64 == 0 else 32)

    def out(mt, nt, wt, wc, c, x=x3):
        return (mt, nt, wt, wc, c, x), 32 * mt * wt
    if x3 and not small_tiles and co % 256 == 0 and ci == 192:
        return out(2, 2, 1, 4, 64)
    if co % 256 == 0:
        if x3 and small_tiles and ci == 256:
            return out(2, 2, 1, 4, 128)
        return out(4, 2, 1, 4, ck())
    if x3 and small_tiles and co % 128 == 0 and ci % 128 == 0:
        return out(2, 1, 1, 4, 128)
    if x3 and small_tiles and co % 64 == 0 and co % 128 and ci % 64 == 0:
        return out(2, 1, 2, 2, 64)
    if co % 128 == 0:
        return out(4, 1, 1, 4, ck())
    if co % 64 == 0:
        return out(4, 1, 2, 2, 64 if ci % 64 == 0 else 32)
    return out(4, 1, 4, 1, 64 if ci % 64 == 0 else 32)


def reachable_branches(exact):
    """the instantiations an upsampler (2 ch -> u ch channels) of a generator with upsample_initial_channel in {16 .. 512} and u <= 8 reaches"""
    return {vconv_config(pad32(u * c_in // 2), pad32(c_in), exact, exact)[0] for c_in in (16, 32, 64, 128, 256, 512) for u in range(1, 9)}


# ------------------------------------------------------------------------------------------------ the case table
def iso(c0, u, k):
    """an isolating generator: ONE upsampler, so that its rows are the ResBlocks' input directly and stage rows are waveform samples; the
    ResBlock side is what tests/test_vocoder_kernels_gpu.py and tests/test_hifigan_v2_gpu.py already run"""
    return {"resblock": "1", "upsample_rates": [u], "upsample_kernel_sizes": [k], "upsample_initial_channel": c0,
            "resblock_kernel_sizes": list(RB_KERNELS), "resblock_dilation_sizes": [list(d) for d in RB_DILATIONS]}


FORMS_AT_64 = [("single", 4, 4), ("single", 3, 3), ("half", 6, 12), ("general", 4, 6), ("general", 8, 12), ("general", 3, 5), ("general", 5, 7),
               ("general", 5, 9), ("general", 6, 10), ("half", 2, 4)]   # (2, 4): the control, what the rest of the suite runs
WIDE_AND_NARROW = [("general", 3, 5), ("general", 5, 9), ("single", 4, 4)]
# beyond the issue's table: the launcher branch no row above reaches (ci == 32 under 128 packed channels, 8 x 16), and k = 2u where the packed
# channels do not split into whole waves (6 x 8 = 48 under a pack of 64: the general form), which the bf16x3 / per-convolution tests run
EXTRA = [("general", 8, 12, 32), ("general", 6, 12, 16)]


def case_name(u, k, c0):
    return f"u{u}k{k}_c{c0}"


CASES = {}   # name -> {"u", "k", "c0", "form", "cfg"}
for _form, _u, _k in FORMS_AT_64:
    CASES[case_name(_u, _k, 64)] = {"u": _u, "k": _k, "c0": 64, "form": _form}
for _c0 in (512, 256, 128, 32, 16):
    for _form, _u, _k in WIDE_AND_NARROW:
        CASES[case_name(_u, _k, _c0)] = {"u": _u, "k": _k, "c0": _c0, "form": _form}
for _form, _u, _k, _c0 in EXTRA:
    CASES[case_name(_u, _k, _c0)] = {"u": _u, "k": _k, "c0": _c0, "form": _form}
for _c in CASES.values():
    _c["cfg"] = iso(_c["c0"], _c["u"], _c["k"])
CONTROL = case_name(2, 4, 64)

# one generator with a different form per stage (single, general, general) whose ragged stage lengths are multiples of 4, 20 and 60
MIXED = {"resblock": "1", "upsample_rates": [4, 5, 3], "upsample_kernel_sizes": [4, 9, 5], "upsample_initial_channel": 256,
         "resblock_kernel_sizes": list(RB_KERNELS), "resblock_dilation_sizes": [list(d) for d in RB_DILATIONS]}

# refused by name at dtts_finalize_weights, in every precision
REFUSED = [(3, 6), (5, 10), (4, 7),   # odd k - u: ConvTranspose1d yields T u + 1 rows
           (4, 2), (4, 3),            # k < u: the reference's padding would be negative
           (5, 11), (2, 6)]           # k > 2 u: more than three taps


def width(case):
    """the stage width (channels of the upsampler's output and of the ResBlocks)"""
    return CASES[case]["c0"] // 2


def narrow(case):
    return width(case) in (16, 8)


def launch_of(case, mode):
    """((MT, NT, WT, WC, CK, X3), TT) of the case's upsampler in a mode of the GPU tests ('f16', 'f16_release': DTTS_VOC_F16; 'bf16')"""
    c = CASES[case]
    exact = mode != "bf16"
    return vconv_config(pad32(c["u"] * c["c0"] // 2), pad32(c["c0"]), exact, exact)   # (vocoder.hip: p.small_tiles = exact)


def tile_lengths(case, mode):
    """input frames around the upsampler's tile seams: TT - 1, TT, TT + 1, 2 TT + 1, and the longer utterance (3 TT + 5) of the ragged batch"""
    tt = launch_of(case, mode)[1]
    return [tt - 1, tt, tt + 1, 2 * tt + 1], 3 * tt + 5


# ------------------------------------------------------------------------------------------------ the polyphase sum, restated
def polyphase(a, w, b, u, k, defect=None, at=None):
    """conv_transpose1d(a, w, b, stride=u, padding=(k - u) / 2) of a [B, C_in, T] as the polyphase sum above (torch, the dtype of `a`).
    defect plants what a kernel could get wrong; `at` is the input row it concerns:
      'plus_tap_at_end'    the delta = +1 tap of the last input row reads a non-zero row (row T / 2) instead of zero
      'minus_tap_at_start' the delta = -1 tap of row 0 reads a non-zero row (row T / 2) instead of zero
      'phase_rotated'      output phase r is written where phase r + 1 belongs
      'pad_off_by_one'     p + 1 instead of p
      'seam_tap_dropped'   the delta = +1 tap of input row `at` (the last row of a tile: t0 + TT - 1) is not added
      'pad_channel_store'  the value of the first padding channel of row `at` (packed channel u C_out: zero weights, zero bias = 0) lands on
                           channel 0, phase 0 of row at + 1 (a 16-byte store past C_out at a row pitch of u C_out)"""
    B, _, T = a.shape
    c_out = w.shape[1]
    p = (k - u) // 2 + (1 if defect == "pad_off_by_one" else 0)
    out = a.new_zeros(B, c_out, T, u)
    for delta in (-1, 0, 1):
        wd = a.new_zeros(w.shape[0], c_out, u)
        for r in range(u):
            j = r + p - u * delta
            if 0 <= j < k:
                wd[:, :, r] = w[:, :, j]
        sh = a.new_zeros(a.shape)   # sh[q] = a[q + delta], zero outside the utterance
        if delta == 0:
            sh = a
        elif delta == 1:
            sh[:, :, :T - 1] = a[:, :, 1:]
            if defect == "plus_tap_at_end":
                sh[:, :, T - 1] = a[:, :, T // 2]
            if defect == "seam_tap_dropped":
                sh[:, :, at] = 0
        else:
            sh[:, :, 1:] = a[:, :, :T - 1]
            if defect == "minus_tap_at_start":
                sh[:, :, 0] = a[:, :, T // 2]
        out = out + torch.einsum("bct,cor->botr", sh, wd)
    if b is not None:
        out = out + b.view(1, -1, 1, 1)
    if defect == "phase_rotated":
        out = torch.roll(out, 1, dims=3)
    if defect == "pad_channel_store":
        out = out.clone()
        out[:, 0, at + 1, 0] = 0
    return out.reshape(B, c_out, T * u)


def planted(defect, at=None):
    """an Emulator hook that replaces ups.0 by the polyphase sum carrying `defect`, at the emulator's own rounding points"""
    def hook(name, x, emu):
        if name == "conv_pre":
            emu.ups_input = x
        if name == "ups.0":
            u, k = emu.cfg["upsample_rates"][0], emu.cfg["upsample_kernel_sizes"][0]
            return emu._serial(lambda a, w, b: polyphase(a, w, b, u, k, defect, at), emu.ups_input, "ups.0", 0.1)
    return hook
