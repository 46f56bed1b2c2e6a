"""dict_tts_amd.fft.FFTBlocks (csrc/fft_blocks.hip, dtts_fft_blocks_forward) row by row against the float64 restatement tests/fft_ref.py,
at the seams of its kernels and at the model shapes of tests/fft_shapes.py (which names the kernel every launch runs at every case;
tests/test_fft_blocks_cpu.py proves that the table reaches the branches it names and that the planted defects exceed the bounds).

Every comparison prints one ``FFTMEAS {json}`` line (pytest -s): the whole output, the first 8 and the last 8 valid rows of every
utterance (the rows on which the k-tap halo of ffn_1 reads the LayerNorm bias of padded frames), each against fft_ref.FFT_BOUNDS (max abs,
largest 8-row window RMS, RMS), and rows past an utterance's end must be exactly 0.  ``oracle_fp32`` lines are the fp32 oracle's own
distance from float64 on the same case, for context: they are not asserted.

  * position seams: fft_positions_kernel scans in chunks of 256 frames (4 waves of 64 lanes) with a carry; first-channel-zero frames at
    0, 63, 64, 255, 256, 511, 512, value-derived padding and an explicit mask SHORTER than the non-zero extent of x, alpha 0.8 and 1
  * attention and the 32-row convolution tiles: padded T 97 .. 161 across the 128 / 129 switch of mha_launch, lengths 1 .. 128 in one batch,
    each padded T at B = 1 too
  * the positional table regrown at T >= 2000, and a short call after it
  * every fft_shapes entry end to end, the two-sided ones on both sides of the 256-tile limit of the fp32 short kernel
  * the constructor switches, the refusals by message, and one shape per branch under debug_redzone

Out of scope: interior all-zero frames (non-suffix padding).  rowcount_nonzero counts rows, and fft.py requires a suffix mask; the
reference would mask such a frame as a key in the middle of an utterance.
"""
import json

import numpy as np
import pytest
import torch

import fft_ref as fr
import fft_shapes as fs
from dict_tts_amd import abi, fft
from oracle import fft_blocks_ref as oref

pytestmark = pytest.mark.gpu

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
DEFAULT = fs.SHAPES["h192_heads2"]


def make(shape, sd_np, hparams=None, **kw):
    m = fft.FFTBlocks(shape["hidden"], shape["layers"], ffn_kernel_size=shape["k"], num_heads=shape["heads"], hparams=hparams or {}, **kw)
    m.load_state_dict({k: T(v) for k, v in sd_np.items()})
    return m


def run(m, x, lens=None):
    """the module's output on the host; lens: an explicit suffix padding_mask of these lengths"""
    pm = None if lens is None else T(np.arange(x.shape[1])[None, :] >= np.asarray(lens)[:, None])
    y = m(T(x), padding_mask=pm)
    torch.cuda.synchronize()
    return y.cpu()


def ref64(shape, sd_np, x, lens=None, **kw):
    tab = fr.table(max(2000, x.shape[1] + 1), shape["hidden"]) if kw.get("use_pos_embed", True) else None
    return fr.forward(fr.state(sd_np), T(x).double(), lens=lens, num_heads=shape["heads"], kernel_size=shape["k"], pos_table=tab, **kw)


def oracle_line(case, shape, sd_np, x, lens, want, use_pos_embed=True, use_last_norm=True):
    """context: the fp32 oracle's own error against float64 on this case"""
    pm = None if lens is None else T(np.arange(x.shape[1])[None, :] >= np.asarray(lens)[:, None])
    o = oref.fft_blocks({k: T(v) for k, v in sd_np.items()}, T(x), padding_mask=pm, num_heads=shape["heads"], kernel_size=shape["k"],
                        use_pos_embed=use_pos_embed, use_last_norm=use_last_norm)
    print("FFTMEAS " + json.dumps({"case": case, "what": "oracle_fp32", **fr.rowcmp(o, want)}), flush=True)


def true_lens(x, lens=None):
    return [int(n) for n in (lens if lens is not None else (np.abs(x).sum(-1) != 0).sum(1))]


# ------------------------------------------------------------------------------------------------------------------ position seams
@pytest.mark.parametrize("kind", ["derived", "mask", "alpha1"])
def test_position_seams(kind):
    """B = 3, T = 513, lengths 513 / 257 / 256: zero-first-channel frames beside the wave and chunk boundaries of the position scan and at
    the last valid frame of utterance 1; with an explicit mask the positions still count the non-zero frames BEHIND the mask's end.  With
    one layer and alpha = 1 the table row of every frame reaches the output at full weight: a position off by one is an error of ~1."""
    s = fs.SEAM_SHAPE
    sd = fs.state_np(s)
    if kind == "alpha1":
        sd["pos_embed_alpha"] = np.array([1.0], np.float32)
    x, lens = fs.seam_input(kind == "mask")
    want = ref64(s, sd, x, lens)
    got = run(make(s, sd), x, lens)
    oracle_line("seam." + kind, s, sd, x, lens, want)
    bad = fr.compare("seam." + kind, got, want, true_lens(x, lens), fr.bounds_of(192))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------ attention + 32-row conv tiles
TILE_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def tile_lens(T_pad):
    return TILE_LENS + ((129,) if T_pad == 129 else ()) if T_pad in (128, 129) else (T_pad, T_pad - 1, 65, 32, 1)


@pytest.fixture(scope="module")
def tile_models():
    out = {}
    for name in ("h192_heads2", "h384_heads4-mfma_c384-ffn2_generic"):
        sd = fs.state_np(fs.SHAPES[name])
        out[name] = (sd, make(fs.SHAPES[name], sd))
    return out


@pytest.mark.parametrize("T_pad", [97, 100, 128, 129, 161])
@pytest.mark.parametrize("name", ["h192_heads2", "h384_heads4-mfma_c384-ffn2_generic"])
def test_attention_and_conv_tiles(tile_models, name, T_pad):
    """mha_mfma_kernel (128-query tiles) up to T = 128, mha_mfma_split_kernel (32-query tiles, keys split over the waves) from 129, at
    the row pitches of C = 192 and C = 384; utterance ends on both sides of every 32-row convolution tile and of the 64-key / 128-query
    tiles; the full-length utterance once more ALONE (B = 1), against the same reference rows and bit-identical to its rows in the batch"""
    s = fs.SHAPES[name]
    sd, m = tile_models[name]
    lens = tile_lens(T_pad)
    assert fs.mha_kernel(s["hidden"], s["heads"], T_pad) == ("mfma_split" if T_pad > 128 else "mfma")
    x = fs.ragged(f"tiles.{name}.{T_pad}", (len(lens), T_pad, s["hidden"]), lens)
    want = ref64(s, sd, x)
    case = f"tiles.{name.split('-')[0]}.T{T_pad}"
    got = run(m, x)
    oracle_line(case, s, sd, x, None, want)
    bad = fr.compare(case, got, want, lens, fr.bounds_of(s["hidden"]))
    b = int(np.argmax(lens))                                             # the longest utterance alone: value-derived T stays T_pad
    alone = run(m, x[b:b + 1])
    bad += fr.compare(case + ".B1", alone, want[b:b + 1], lens[b:b + 1], fr.bounds_of(s["hidden"]))
    assert not bad, bad
    # batch-invariant arithmetic: no launch rule of these two shapes depends on B, so alone = inside the batch, bit for bit
    assert torch.equal(alone[0], got[b]), f"{case}: the utterance alone differs from the same utterance inside the batch"


# ------------------------------------------------------------------------------------------------------------------ table regrowth
def test_positional_table_regrowth():
    """fft.py keeps a table of 2000 rows and regrows it when T >= 2000 (the library wants n_pos > T): T = 1999, 2000, 2001 in that order on
    one module, then T = 45 — with the grown table it must give the bits a fresh module gives; n_pos == T is refused by name"""
    s = dict(DEFAULT, layers=1)
    sd = fs.state_np(s)
    m = make(s, sd)
    x = fs.ragged("regrow", (1, 2001, 192), (2001,))
    bad = []
    for T_pad in (1999, 2000, 2001):
        xt = np.ascontiguousarray(x[:, :T_pad])
        got = run(m, xt)
        assert m._table.shape[0] == max(2000, T_pad + 1)
        bad += fr.compare(f"regrow.T{T_pad}", got, ref64(s, sd, xt), [T_pad], fr.bounds_of(192))
    x45 = fs.ragged("regrow45", (2, 45, 192), (45, 30))
    after, fresh = run(m, x45), run(make(s, sd), x45)
    assert m._table.shape[0] == 2002 and torch.equal(after, fresh)
    bad += fr.compare("regrow.then45", after, ref64(s, sd, x45), [45, 30], fr.bounds_of(192))
    assert not bad, bad
    xd = T(x45).cuda()
    y = torch.empty_like(xd)
    tab = fft.sinusoid_table(45, 192, 0).cuda()
    with pytest.raises(abi.DttsError, match=r"pos_table needs > T = 45 rows \(got 45\)"):
        m.ctx.fft_blocks_forward(xd.data_ptr(), None, tab.data_ptr(), 45, 2, 45, y.data_ptr(), torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------------------------------------------- every table entry
@pytest.mark.parametrize("name", list(fs.SHAPES))
def test_every_shape_end_to_end(name):
    """ragged batch of the shape's table entry; with `repeat`, the same utterances that many times over in a second batch: for the
    two-sided entries (h256: ffn_2, h768: ffn_1) that is the other side of the 256-tile limit, where the layer leaves the fp32 short kernel
    for the generic one — both inside the bounds, bit-identity printed (the two kernels sum in different orders by design); at hidden
    192 every convolution keeps the three-piece short kernel at any batch, and B = 6 and B = 90 must give the same bits"""
    s = fs.SHAPES[name]
    sd = fs.state_np(s)
    m = make(s, sd)
    x, lens = fs.shape_input(name), list(s["lens"])
    want = ref64(s, sd, x)
    case = "shape." + name.split("-")[0]
    got = run(m, x)
    oracle_line(case, s, sd, x, None, want)
    bounds = fr.bounds_of(s["hidden"])
    bad = fr.compare(case, got, want, lens, bounds)
    if s["repeat"]:
        r = s["repeat"]
        big = run(m, np.tile(x, (r, 1, 1)))
        bad += fr.compare(f"{case}.x{r}", big, want.repeat(r, 1, 1), lens * r, bounds)
        same = all(torch.equal(big[i * len(lens):(i + 1) * len(lens)], got) for i in range(r))
        print("FFTMEAS " + json.dumps({"case": case, "what": f"B{len(lens)}_bit_identical_to_B{len(lens) * r}", "value": same,
                                       "kernels_small": fs.kernels(s, len(lens), s["T"]), "kernels_big": fs.kernels(s, len(lens) * r, s["T"])}), flush=True)
        if s["hidden"] == 192:
            assert same, "hidden 192: the three-piece short kernel must give an utterance the same bits at B = 6 and B = 90"
        else:   # both copies of the batch ran the same kernels: every repetition must at least equal the first
            assert all(torch.equal(big[i * len(lens):(i + 1) * len(lens)], big[:len(lens)]) for i in range(r))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- switches
@pytest.mark.parametrize("switch", ["no_last_norm", "no_pos_quiet", "no_pos_alpha", "alpha_0.37"])
def test_switches(switch):
    """use_last_norm=False (the copy exit), use_pos_embed=False (on an input with near-silent rows, where LayerNorm's eps 1e-5 shows),
    use_pos_embed_alpha=False (alpha = 1, the state dict's 0.8 ignored as the reference ignores it), alpha = 0.37"""
    s = dict(DEFAULT, layers=1)
    kw, x, lens = {}, fs.ragged("switch", (3, 70, 192), (70, 33, 9)), [70, 33, 9]
    x[0, 32, 0] = 0.0                                                   # one frame without a position
    if switch == "no_last_norm":
        kw = dict(use_last_norm=False)
    elif switch == "no_pos_quiet":
        kw = dict(use_pos_embed=False)
        x, lens = fs.quiet_input()
    elif switch == "no_pos_alpha":
        kw = dict(use_pos_embed_alpha=False)
    sd = fs.state_np(s, **{k: v for k, v in kw.items() if k != "use_pos_embed_alpha"})
    if switch == "alpha_0.37":
        sd["pos_embed_alpha"] = np.array([0.37], np.float32)
    want = ref64(s, sd, x, **kw)
    if switch in ("no_pos_alpha", "alpha_0.37"):                        # the switch acts: alpha 0.8 would be far outside the bounds
        assert fr.rowcmp(ref64(s, fs.state_np(s), x), want)["max"] > 1e-2
    got = run(make(s, sd, **kw), x)
    bad = fr.compare("switch." + switch, got, want, lens, fr.bounds_of(192))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_message():
    """what the library does not run is refused by name, never computed wrongly: dk > 96 and a hidden size that is no multiple of 64 by
    dtts_create, an even kernel and heads that do not divide the hidden size by the weight finalisation, forward before the weights"""
    with pytest.raises(abi.DttsError, match="dtts_create: unsupported configuration"):      # the reference's base shape: dk = 128
        fft.FFTBlocks(256, 1, num_heads=2, hparams={})
    with pytest.raises(abi.DttsError, match="dtts_create: unsupported configuration"):
        fft.FFTBlocks(190, 1, num_heads=4, hparams={})
    s = dict(DEFAULT, layers=1, k=4)
    with pytest.raises(RuntimeError, match=r"FFT blocks: unsupported configuration \(layers=1 kernel=4 hidden=192 heads=2\)"):
        make(s, fs.state_np(s))
    s = dict(DEFAULT, layers=1, heads=5)
    with pytest.raises(RuntimeError, match=r"FFT blocks: unsupported configuration \(layers=1 kernel=9 hidden=192 heads=5\)"):
        make(s, fs.state_np(s))
    m = fft.FFTBlocks(192, 1, num_heads=2, hparams={})
    with pytest.raises(RuntimeError, match=r"load_state_dict\(\) must be called first"):
        m(torch.zeros(1, 4, 192))


# -------------------------------------------------------------------------------------------------------------------- memory safety
REDZONE = [("h192_heads2", False), ("h256_heads4-mha_dk64-ffn2_f32_short_or_generic", False), ("h256_heads4-mha_dk64-ffn2_f32_short_or_generic", True),
           ("h384_heads4-mfma_c384-ffn2_generic", False), ("h768_heads8-ffn1_generic_gelu", True), ("h192_k13", False)]


@pytest.mark.parametrize("name,big", REDZONE, ids=[n.split("-")[0] + (".big" if b else "") for n, b in REDZONE])
def test_memory_safety(name, big):
    """debug_redzone (every workspace buffer and weight pack between red zones, the workspace NaN-filled): one shape per convolution and
    attention branch; no zone damaged, and the bits of the release context"""
    s = fs.SHAPES[name]
    sd = fs.state_np(s)
    x = fs.shape_input(name)
    if big:
        x = np.tile(x, (s["repeat"], 1, 1))
    rel, dbg = make(s, sd), make(s, sd, hparams={"dtts_debug_redzone": 1})
    a, b = run(rel, x), run(dbg, x)
    n = dbg.ctx.debug_check(torch.cuda.current_stream().cuda_stream)
    assert n == 0, f"{name}: {dbg.ctx.last_error()}"
    assert torch.isfinite(b).all() and torch.equal(a, b)
