"""The gloss encoder on the GPU (dict_tts_amd/gloss_encoder.py, csrc/gloss.hip) against the float64 restatement tests/gloss_ref.py, which
tests/test_gloss_cpu.py anchors on Hugging Face's RoFormerForMaskedLM.  Seeded weights (gloss_shapes.seeded_state), never a checkpoint.

Error gate: max |gpu - float64| over a call <= 8 x max |float32 restatement - float64| on the same inputs, both measured here.  Both sides
form the same exact fp32 products and differ in summation order and in exp / erf / rsqrt, which moves the rounding error by a single-digit
factor: 8 is the project's margin for that situation (tests/test_disc_gpu.py, tests/test_spkenc_gpu.py).  The ratios are printed.

Measured on an MI355X (LABNOTES.md "Gloss encoder"): mixed lengths 0.37 x (h128x7), 1.06 x (h768x1), 0.62 x (h384x2); a single token
0.71 / 1.52 / 1.18 x; the golden 0.74 x of the float32 restatement's error (gate 9 x); table path - tensor path pron_attn 6.0e-8, dict_attn
1.8e-6.

Beside that gate, which a few softmax-sensitive rows set 45 .. 90 x above a typical row, every call is held to gloss_ref.BOUNDS (R.judge,
one ``GLOSSMEAS {json}`` line per call): the global RMS (rms(gpu - f64) <= 4 x rms(f32 - f64)) and every row (rms_r(gpu - f64) <= 6 x
max(rms_r(f32 - f64), rms(f32 - f64))).  Measured on an MI355X, max / rms / worst row, mixed lengths then a single token:
    h128x7           0.37 / 0.45 / 1.16    0.71 / 0.79 / 0.79        h64_nh1_wideffn  0.29 / 0.47 / 1.09    0.82 / 1.17 / 1.17
    h768x1           1.06 / 1.09 / 1.57    1.52 / 1.43 / 1.43        h192_nh3_pad     0.69 / 0.51 / 1.28    0.63 / 0.83 / 0.83
    h384x2           0.62 / 0.84 / 1.48    1.18 / 1.38 / 1.38        h832_generic     1.82 / 1.67 / 2.92    1.52 / 1.53 / 1.53
                                                                     h1024_generic    2.02 / 2.02 / 3.31    1.55 / 1.82 / 1.82
the seams (test_row_and_length_seams) 0.52 .. 0.91 / 0.56 .. 0.69 / 0.82 .. 1.77 at h128x7 and 1.50 .. 2.04 / 1.63 .. 2.11 / 2.28 ..
3.28 at h832_generic; hidden 64 / ffn 204 0.35 / 0.52 / 1.62; the seven layer views of h128x7 (test_layer_resolved_rows) at most 0.64 /
0.64 / 2.42.  Worst of all: 2.04 / 2.11 / 3.31, so the margins are 1.9 x and 1.8 x the
worst ratio (the project's practice: at most 3 x), and they satisfy the two conditions of the planted defects (tests/test_gloss_cpu.py):
rms <= 6 (eps_1e-6 reads 6.55 at its least sensitive shape) and row <= 8 (10.7).  The shapes on conv1d_cl_kernel<ENG_F32> (hidden >= 832)
read about twice the short kernel's ratios: there one fp32 accumulator takes all C_in products of an output in sequence, where the short
kernel sums four parts and the float32 restatement's GEMM sums blocks — a single-digit factor in rounding, no defect.

intermediate_size = 202 (no multiple of 4) is REFUSED, by check_config and by dtts_finalize_weights(DTTS_PART_GLOSS): output.dense stages
its input rows (pitch intermediate_size floats) as 16-byte loads guarded by the piece's first channel (conv1d.hip: `ci < p.C_in`), so every
odd row's loads would be misaligned and the last piece of the last row would read two floats behind it; 204 runs, red zones whole."""
import numpy as np
import pytest
import torch

import gloss_ref as R
import gloss_shapes as S
from dict_tts_amd import abi, synth
from dict_tts_amd import gloss_encoder as G
from dict_tts_amd import model as M

pytestmark = pytest.mark.gpu
MARGIN = 8.0
_CACHE = {}


def setup(name):
    """per configuration, once: the weights, the encoder, the mixed-length id set, its float64 / float32 restatements and the GPU's result"""
    if name not in _CACHE:
        cfg, n_hidden = (S.GOLDEN_CFG, 8) if name == "golden" else S.ALL_CFGS[name]
        st = S.seeded_state(cfg)
        enc = G.GlossEncoder.from_pretrained(st, cfg, n_hidden=n_hidden)
        ids = S.id_sets(S.MIXED_LENGTHS)
        c = {"cfg": cfg, "n_hidden": n_hidden, "state": st, "enc": enc, "ids": ids}
        if name != "golden":
            c["f64"] = R.encode_np(st, cfg, ids, torch.float64, n_hidden)
            c["f32"] = R.encode_np(st, cfg, ids, torch.float32, n_hidden)
            c["gpu"] = enc.encode(ids)
        _CACHE[name] = c
    return _CACHE[name]


@pytest.fixture(autouse=True, scope="module")
def _module():
    yield
    _CACHE.clear()


def cat(outs):
    return torch.cat(outs).double().cpu().numpy()


@pytest.mark.parametrize("name", list(S.ALL_CFGS))
def test_accuracy_mixed_lengths(name):
    c = setup(name)
    assert sum(S.MIXED_LENGTHS) % 32 and sum(S.MIXED_LENGTHS) % 128
    got = cat(c["gpu"])
    assert [tuple(o.shape) for o in c["gpu"]] == [(L, c["cfg"]["hidden_size"]) for L in S.MIXED_LENGTHS] and np.isfinite(got).all()
    e_gpu, e_f32 = np.abs(got - c["f64"]).max(), np.abs(c["f32"] - c["f64"]).max()
    print(f"GLOSSMEAS {name}: gpu - f64 {e_gpu:.3g}, f32 - f64 {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}, scale {np.abs(c['f64']).max():.3g}")
    assert e_gpu <= MARGIN * e_f32
    fails = R.judge(f"{name} mixed", got, c["f64"], c["f32"])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", list(S.ALL_CFGS))
def test_accuracy_single_token(name):
    c = setup(name)
    ids = S.id_sets((1,), seed=S.SEED + 1)
    got = cat(c["enc"].encode(ids))
    f64 = R.encode_np(c["state"], c["cfg"], ids, torch.float64, c["n_hidden"])
    f32 = R.encode_np(c["state"], c["cfg"], ids, torch.float32, c["n_hidden"])
    e_gpu, e_f32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
    print(f"GLOSSMEAS {name} L = 1: gpu - f64 {e_gpu:.3g}, f32 - f64 {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}")
    assert got.shape == (1, c["cfg"]["hidden_size"]) and e_gpu <= MARGIN * e_f32
    fails = R.judge(f"{name} L = 1", got, f64, f32)
    assert not fails, "\n".join(fails)


def test_golden():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_gloss.npz"))
    c = setup("golden")
    ids = [g["ids"][a:b] for a, b in zip(g["tok_off"][:-1], g["tok_off"][1:])]
    got = cat(c["enc"].encode(ids))
    e_f32 = np.abs(R.encode_np(c["state"], c["cfg"], ids, torch.float32, 8) - g["feat"]).max()
    e_gpu = np.abs(got - g["feat"]).max()
    print(f"GLOSSMEAS golden: gpu - golden {e_gpu:.3g}, f32 - golden {e_f32:.3g}, ratio {e_gpu / e_f32:.2f}")
    assert e_gpu <= (MARGIN + 1) * e_f32


def independence(name):
    c = setup(name)
    enc = c["enc"]
    lengths = [1 + (7 * i) % 64 for i in range(39)]
    others = S.id_sets(lengths, seed=S.SEED + 2)
    fails = []
    for L in (1, 33, 64):
        me = S.id_sets((L,), seed=S.SEED + 3)[0]
        alone = enc.encode([me])[0]
        for place in (0, 20, 39):
            seqs = others[:place] + [me] + others[place:]
            got = enc.encode(seqs)[place]
            if not torch.equal(got, alone):
                fails.append(f"L = {L} at place {place} of 40: differs from the gloss alone by {float((got - alone).abs().max()):.3g}")
    small = G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=c["n_hidden"], row_budget=64)
    a, b = enc.encode(others), small.encode(others)
    fails += [f"gloss {i} (L = {lengths[i]}): row budgets 16384 and 64 differ" for i in range(len(others)) if not torch.equal(a[i], b[i])]
    assert not fails, "\n".join(fails)


def test_batch_independence():
    """a gloss alone, first, last and in the middle of a 40-gloss call, and the whole call under two row budgets: the same bits"""
    independence("h128x7")


@pytest.mark.parametrize("name", ["h768x1", "h832_generic", "h192_nh3_pad"])
def test_batch_independence_at(name):
    """the same where the short kernel stages the wide tile (768: U = 24; how many waves share a contraction follows from the grid), on
    the generic kernel (832: its tile shape follows from the row count) and with padded channel counts (192 / 200)"""
    independence(name)


def test_refusals_and_status():
    c = setup("h128x7")
    enc = c["enc"]
    ctx, dev = enc.ctx, enc.device
    stream = torch.cuda.current_stream().cuda_stream
    ids = torch.zeros(128, dtype=torch.int64, device=dev)
    out = torch.empty(128, 128, dtype=torch.float32, device=dev)
    status = torch.zeros(2, dtype=torch.int64, device=dev)

    def call(off, sum_L, L_max):
        t = torch.tensor(off, dtype=torch.int32, device=dev)
        ctx.gloss_encode(len(off) - 1, stream, ids=ids.data_ptr(), tok_off=t.data_ptr(), sum_L=sum_L, L_max=L_max, out=out.data_ptr(), status=status.data_ptr())

    for off, sum_L, L_max, word in (([0, 3, 68], 68, 64, "gloss 1 has L = 65"), ([0, 0, 5], 5, 5, "gloss 0 has L = 0"), ([0, 3, 8], 8, 6, "L_max = 6"),
                                    ([1, 3, 8], 8, 5, "tok_off[0] = 1"), ([0, 3, 7], 8, 5, "tok_off[n_gloss] = 7")):
        with pytest.raises(abi.DttsError, match=r"\(-22\).*" + word.replace("[", r"\[").replace("]", r"\]")):
            call(off, sum_L, L_max)
    call([0, 3, 8], 8, 5)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0]
    # an id equal to the vocabulary's size: a zero embedding row, the status names row and id, Python raises with the gloss and the position
    seqs = [np.array([1, 2, 3]), np.array([4, S.VOCAB, 5, S.VOCAB + 1])]
    with pytest.raises(abi.DttsError, match=rf"gloss 1, position 1: token id {S.VOCAB} .*row 4"):
        enc.encode(seqs)
    with pytest.raises(abi.DttsError, match="no weights"):
        G.GlossEncoder().encode([[1, 2]])
    fresh = abi.Context()
    with pytest.raises(abi.DttsError, match=r"\(-1\).*before dtts_finalize_weights\(DTTS_PART_GLOSS\)"):
        fresh.gloss_encode(1, stream, ids=ids.data_ptr(), tok_off=ids.data_ptr(), sum_L=3, L_max=3, out=out.data_ptr(), status=status.data_ptr())
    # finalize names what it refuses
    w = dict(enc._state())
    for change, word in (({"config": np.array([4, 1e-12, 0, 0], np.float32)}, "heads of 64"), ({"config": np.array([2, 1e-12, 1, 0], np.float32)}, "rotary_value"),
                         ({"config": np.array([2, 1e-12, 0, 1], np.float32)}, "hidden_act"),
                         ({"embeddings.word_embeddings.weight": np.zeros((S.VOCAB, 64), np.float32)}, "embedding_size = 64")):
        bad = abi.Context()
        bad.load_state_dict("gloss", {**w, **change})
        with pytest.raises(abi.DttsError, match=r"\(-22\).*" + word):
            bad.finalize(abi.PART_GLOSS)
    bad = abi.Context()
    bad.load_state_dict("gloss", {k: v for k, v in w.items() if k != "encoder.layer.2.intermediate.dense.bias"})
    with pytest.raises(abi.DttsError, match=r"\(-22\).*missing tensor gloss.encoder.layer.2.intermediate.dense.bias"):
        bad.finalize(abi.PART_GLOSS)


def red_zones(name):
    c = setup(name)
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    ctx = abi.Context(cfg)
    enc = G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=c["n_hidden"], ctx=ctx, row_budget=128)
    got = enc.encode(c["ids"])
    damaged = ctx.debug_check(torch.cuda.current_stream().cuda_stream)
    assert damaged == 0, ctx.last_error()
    assert all(torch.equal(a, b) for a, b in zip(got, c["gpu"]))


def test_red_zones_stay_whole():
    """debug_redzone = 1: every workspace buffer between red zones and 0xFF before each call; no launch damages a zone, no stale word is
    consumed (the result would be NaN), and the bits are those of the plain context"""
    red_zones("h128x7")


@pytest.mark.parametrize("name", ["h768x1", "h832_generic", "h192_nh3_pad"])
def test_red_zones_stay_whole_at(name):
    """... at 192 / 200 in particular: the last 16-byte piece of a feed-forward row (channels 196 .. 199) ends on the row's end, the padded
    channels 200 .. 255 of output.dense's tile are zeros and not loads"""
    red_zones(name)


@pytest.mark.parametrize("lengths", S.SEAM_LENGTHS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("name", ["h128x7", "h832_generic"])
def test_row_and_length_seams(name, lengths):
    """row totals that end on a 32-row and on a 128-row tile, 64 / 65 rows around the generic kernel's tile switch, and calls whose
    longest gloss (the pitch of every LDS tile of the attention kernel) has 2 and 33 tokens: the three gates, and the bits of each gloss alone"""
    c = setup(name)
    ids = S.id_sets(lengths, seed=S.SEED + 5)
    outs = c["enc"].encode(ids)
    got = cat(outs)
    f64 = R.encode_np(c["state"], c["cfg"], ids, torch.float64, c["n_hidden"])
    f32 = R.encode_np(c["state"], c["cfg"], ids, torch.float32, c["n_hidden"])
    fails = R.judge(f"{name} lengths {list(lengths)}", got, f64, f32)
    fails += [f"gloss {i} (L = {len(s)}) of lengths {lengths}: differs from the gloss alone" for i, s in enumerate(ids)
              if not torch.equal(c["enc"].encode([s])[0], outs[i])]
    assert got.shape == (sum(lengths), c["cfg"]["hidden_size"]) and not fails, "\n".join(fails)


def test_layer_resolved_rows():
    """The mean hides a layer among n_hidden + 1 terms.  Encoders of n_hidden = k = 2 .. 8 on the same weights give feat_k, and
    (k + 1) feat_k - k feat_(k - 1) = h_(k - 1) recovers each hidden state (k = 2: 3 feat_2 = E + h_0 + h_1, layer 0's output beside two
    terms that are a gather and one LayerNorm).  The recovery multiplies the rounding of the stored means by about 2 k + 1 half-ulps; the
    float32 restatement is recovered by the same formula from ITS float32 means, so the yardstick of each view carries the same
    amplification and every view is held to the row gate (and the other two) as it stands"""
    c = setup("h128x7")
    ids = c["ids"]
    feats = {k: cat(G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=k).encode(ids)) for k in range(2, 9)}
    assert np.array_equal(feats[8], cat(c["gpu"]))
    ref = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            hs = [R.hidden_states(c["state"], c["cfg"], i, dt, "cpu", 8) for i in ids]   # one run: n_hidden = k takes its first k + 1 entries
            ref[dt] = {k: np.concatenate([torch.stack(h[:k + 1]).mean(dim=0).double().numpy() for h in hs]) for k in range(2, 9)}
    assert np.array_equal(ref[torch.float64][8], c["f64"]) and np.array_equal(ref[torch.float32][8], c["f32"])
    view = lambda f, k: 3 * f[2] if k == 2 else (k + 1) * f[k] - k * f[k - 1]
    fails = []
    for k in range(2, 9):
        fails += R.judge(f"h128x7 layer view k = {k}", view(feats, k), view(ref[torch.float64], k), view(ref[torch.float32], k))
    assert not fails, "\n".join(fails)


def test_status_word_names_the_first_offender():
    """gloss_embed_kernel's reduction over 300 rows: thread r % 256 owns row r, then a tree over the 256 threads"""
    c = setup("h128x7")
    enc = c["enc"]
    ctx, dev, stream = enc.ctx, enc.device, torch.cuda.current_stream().cuda_stream
    lens = [64, 64, 64, 64, 44]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=dev)
    clean = torch.from_numpy(np.concatenate(S.id_sets(lens, seed=S.SEED + 6))).to(dev)
    out = torch.empty(300, 128, dtype=torch.float32, device=dev)
    for bad, want in (({299: S.VOCAB + 3, 257: -5}, [258, -5]),          # both behind the first stride: thread 1 (row 257) against thread 43
                      ({260: S.VOCAB, 5: S.VOCAB + 9}, [6, S.VOCAB + 9]),   # thread 4 holds row 260, thread 5 row 5: the lower ROW wins
                      ({}, [0, 0])):
        ids = clean.clone()
        for r, v in bad.items():
            ids[r] = v
        status = torch.full((2,), -7, dtype=torch.int64, device=dev)
        ctx.gloss_encode(len(lens), stream, ids=ids.data_ptr(), tok_off=off.data_ptr(), sum_L=300, L_max=64, out=out.data_ptr(), status=status.data_ptr())
        torch.cuda.synchronize()
        assert status.tolist() == want, (bad, status.tolist())
        assert bool(torch.isfinite(out).all())
        for r in bad:   # an offender's embedding is zero: its mean still holds the hidden states
            assert float(out[r].abs().max()) > 0
    # through encode, row budget 64: glosses of 40 | 30 + 20 tokens are two calls; the offender sits in the second one
    small = G.GlossEncoder.from_pretrained(c["state"], c["cfg"], n_hidden=c["n_hidden"], row_budget=64)
    seqs = [s.copy() for s in S.id_sets((40, 30, 20), seed=S.SEED + 7)]
    seqs[2][7] = S.VOCAB + 11
    with pytest.raises(abi.DttsError, match=rf"gloss 2, position 7: token id {S.VOCAB + 11} .*row 37 of its call"):
        small.encode(seqs)


def test_rows_times_width_above_int_max_is_refused_before_any_launch():
    """hidden 64, ffn 65536: the workspace row is 65536 floats, so one call takes INT_MAX / 65536 = 32767 rows; 513 glosses of 64 tokens
    are 32832.  (The call just below the limit would take an 8.6 GB workspace: not run.)"""
    cfg = S.config(64, 1, 65536, 1)
    enc = G.GlossEncoder.from_pretrained(S.seeded_state(cfg), cfg, n_hidden=2)
    ctx = enc._context()
    dev, stream = enc.device, torch.cuda.current_stream().cuda_stream
    n, rows = 513, 513 * 64
    ids = torch.zeros(rows, dtype=torch.int64, device=dev)
    off = torch.arange(n + 1, dtype=torch.int32, device=dev) * 64
    out = torch.full((rows, 64), 3.0, dtype=torch.float32, device=dev)
    status = torch.full((2,), -7, dtype=torch.int64, device=dev)
    with pytest.raises(abi.DttsError, match=r"\(-22\).*sum_L = 32832 rows .*intermediate_size 65536 one call takes at most 32767"):
        ctx.gloss_encode(n, stream, ids=ids.data_ptr(), tok_off=off.data_ptr(), sum_L=rows, L_max=64, out=out.data_ptr(), status=status.data_ptr())
    torch.cuda.synchronize()
    assert status.tolist() == [-7, -7] and bool((out == 3.0).all())
    # the same context runs a call of a size it takes
    got = cat(enc.encode(S.id_sets((3, 64))))
    assert got.shape == (67, 64) and np.isfinite(got).all()


def test_finalize_refuses_an_intermediate_size_that_is_no_multiple_of_4():
    """hidden 64 / ffn 202: output.dense would stage rows of 202 floats in 16-byte pieces — every odd row misaligned, the last piece of
    the last row two floats past it (conv1d.hip: `ci < p.C_in` guards a piece's first channel).  Refused by name; 204 runs"""
    cfg = S.config(64, 1, 202, 1)
    w = dict(S.seeded_state(cfg))
    w["config"] = np.array([1, 1e-12, 0, 0], np.float32)
    bad = abi.Context()
    bad.load_state_dict("gloss", w)
    with pytest.raises(abi.DttsError, match=r"\(-22\).*intermediate_size = 202"):
        bad.finalize(abi.PART_GLOSS)
    with pytest.raises(ValueError, match="intermediate_size = 202"):
        G.GlossEncoder.from_pretrained(S.seeded_state(cfg), cfg, n_hidden=2)
    cfg = S.config(64, 1, 204, 1)
    st, ids = S.seeded_state(cfg), S.id_sets(S.MIXED_LENGTHS)
    zone = abi.default_config()
    zone.debug_redzone = 1
    ctx = abi.Context(zone)
    got = cat(G.GlossEncoder.from_pretrained(st, cfg, n_hidden=2, ctx=ctx).encode(ids))
    assert ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, ctx.last_error()
    fails = R.judge("h64 ffn 204", got, R.encode_np(st, cfg, ids, torch.float64, 2), R.encode_np(st, cfg, ids, torch.float32, 2))
    assert not fails, "\n".join(fails)


def test_end_to_end_through_the_dictionary_table():
    """build_table -> dtts_dict_table_upload -> dtts_text2mel_encode_ids on a three-word sentence: pron_attn and dict_attn equal those of
    the tensor path (dtts_text2mel_encode) fed the same embeddings, within the per-row maxima tests/test_s2pa_gpu.py holds both paths to
    (acoustic_ref.BOUNDS)"""
    import acoustic_ref as ar
    c = setup("h768x1")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    g = S.id_sets((5, 3, 5, 32, 7), seed=S.SEED + 4)
    n_words = 8
    entries = {3: [(("zh", "ong1"), g[0])], 4: [(("h", "ang2"), g[1]), (("x", "ing2"), g[2]), (("h", "ang4"), g[3])], 6: [(("d", "e5"), g[4])]}
    table = c["enc"].build_table(entries, n_words)
    assert table["keys"].shape == (3 * 5 + 5 + 40 + 7, 768) and np.isfinite(table["keys"]).all() and np.abs(table["keys"][table["tok_off"][3]:table["tok_off"][4]]).max() > 0.1
    m = M.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(1234).items()})
    m.upload_dict_table(table)
    sent = [[3, 4, 5]]   # one gloss, three glosses, a word the dictionary lacks
    ib = synth.make_id_batch(sent, table, pron_every=0)
    assert (ib["L_k"], ib["P"]) == (40, 6)
    Tw = 5
    keys = np.zeros((1, Tw, 40, 768), np.float32)
    key_map, pinyin, pinyin_map = np.zeros((1, Tw, 40), np.float32), np.zeros((1, Tw, 6), np.int64), np.zeros((1, Tw, 6), np.int64)
    for t, w in enumerate(sent[0]):
        a, b, p, q = table["tok_off"][w], table["tok_off"][w + 1], table["pin_off"][w], table["pin_off"][w + 1]
        keys[0, t + 1, :b - a], key_map[0, t + 1, :b - a] = table["keys"][a:b], table["key_map"][a:b]
        pinyin[0, t + 1, :q - p], pinyin_map[0, t + 1, :q - p] = table["pinyin"][p:q], table["pinyin_map"][p:q]
    key_map[:, [0, -1]] = 1
    pinyin_map[:, [0, -1]] = 1
    m2w = T(synth.teacher_mel2word(ib["word_tokens"], 8, 4))
    assert m2w.shape[1] == 32
    z = T(synth.noise(1234, 1, 8, "gloss.z"))
    by_id = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], mel2word=m2w, z_p=z)
    by_tensor = m((T(ib["word_tokens"]), None), T(ib["pron_modified"]), (None, None, None), None, None,
                  (T(keys), T(keys.copy()), T(key_map), T(pinyin), T(pinyin_map)), infer=True, z_p=z, mel2word=m2w)
    for k in ("pron_attn", "dict_attn"):
        d = float((by_id[k].double() - by_tensor[k].double()).abs().max())
        print(f"GLOSSMEAS end to end: {k} table - tensor {d:.3g}")
        assert by_id[k].shape == by_tensor[k].shape and d <= ar.BOUNDS[k]["max"], k
    # the words attend to their glosses: weights on the live rows of the three-gloss word sum to 1, the missing word's single live row takes all
    da = by_id["dict_attn"][0, 0].cpu().numpy()   # [L_k, T_w]
    assert abs(da[:40, 2].sum() - 1) < 1e-5 and abs(da[1, 3] - 1) < 1e-5
