"""The text-to-mel kernels row by row against the float64 restatement (tests/acoustic_ref.py), at the tile edges of the default shape
and at non-default model shapes (run with `-m gpu` on an MI355X).

Every comparison applies three bounds per output (acoustic_ref.BOUNDS): the max abs error, the largest RMS over 8 consecutive rows
(frames or words) of one utterance, and the global RMS, and prints one ``T2MMEAS {json}`` line (run with -s to see them).  The
end-to-end gates of test_gpu_parity.py hold mel to 1e-3 and word_encoder_out to 1e-4 against the fp32 oracle, which is itself ~1e-5
from float64; a seam defect of a few 1e-4 passes them (tests/test_acoustic_ref_cpu.py plants three).

Shapes.  The kernels size their grids and tiles from the batch's PADDED length (its longest utterance) and follow each utterance's own
length inside a tile, so every edge below runs both ways: as a padded length (alone, B = 1, or as the longest utterance) and as a
per-utterance length inside a longer batch.
  - the prior flow's chunk seams: T_mel/4 in {1, 2, RC-1, RC, RC+1, 2RC, 2RC+1} (RC = 96 rows a flowstack chunk keeps) in one ragged
    batch and each at B = 1; RC-1 / RC / RC+1 at B = 1 for the 2- and 8-block flows too.  The posterior pass's masked forward flow (its
    z_p) on the same lengths.  The reverse flow's z is not exposed: mel is its observable.
  - the decoder's 64-row vconv tiles: T_mel in {60, 64, 68, 124, 128, 132} beside a 400-frame utterance (every frame, each utterance's
    own frames, its first / last 8, its padded frames: the decoder runs them unmasked, as the reference does) and each at B = 1.
  - the encoders and S2PA (ENC_CASES): padded T_w 32, 64, 100, 128, 65, 129, 161 and per-utterance T_w 1, 2, 31, 33, 63, 97, 160 -- the
    32-row conv1d_short_kernel tiles, mha_mfma_kernel up to T = 128 (its fourth query wave and key tile live at 97-128) and
    mha_mfma_split_kernel from 129 on; the MFMA-side lengths at hidden 384 too.  Tensor API and resident-table ids;
    mel2word exact except near-ties.  B = 6 against B = 90: the short kernel's parts-per-wave choice.
  - acoustic_ref.CONFIGS: non-default shapes, each named after the branch it forces, end to end (tensor API and ids), the posterior
    pass for one shape per FVAE family, and one shape per kernel family under debug_redzone (bit-identical to the release context).
    An odd prior_glow_n_blocks is refused by name.

Measured on MI355X, worst over every case here (GPU - float64, max / 8-row window RMS / RMS).  These are the first GPU - float64 figures
for text-to-mel; the only earlier ones were GPU - fp32 oracle (mel 3e-5 with the split-bf16 decoder, 1.4e-5 with decoder_fp32, 1.5e-4 on
the posterior pass).  The bounds (acoustic_ref.BOUNDS) are at most 3x these (1.5x-3x):
  mel (infer)        3.5e-5 / 8.5e-6 / 7.0e-6      mel (posterior)  3.0e-4 / 7.5e-5 / 2.3e-5
  word_encoder_out   1.5e-5 / 2.6e-6 / 1.3e-6      context          2.9e-5 / 4.0e-6 / 2.0e-6
  dur                5.4e-6 / 2.4e-6 / 1.3e-6      dict_attn        6.0e-6 / 6.9e-7 / 3.3e-7
  pron_attn          2.6e-6 / 9.1e-7 / 1.5e-7      z_p (posterior)  3.4e-3 / 3.2e-4 / 1.1e-4 (|z_p| up to ~57)
  m_q                5.3e-5 / 1.5e-5 / 1.1e-5      logs_q           5.7e-5 / 1.4e-5 / 1.0e-5      kl relative 4.8e-6
Bugs these tests found (each failed here before its fix): the resident-table id path at hidden_size > 256 returned pron_attn 0 instead
of 1 on the padded batch's last word row (ops.hip s2pa_kernel's early exit for dead words took a table row of entry -1, whose key_map
row is all ones, for an all-zero one); a latent_size other than 16 failed dtts_finalize_weights, inference included, because the
posterior pass refused the shape there (now only the posterior call is refused).
"""
import numpy as np
import pytest
import torch

import acoustic_ref as ar
from acoustic_ref import as_rows, compare, sd_np, shape_hp   # (shared with the CPU suites: they live beside the bounds)
import posterior_ref as pr
from dict_tts_amd import abi, synth
from oracle import dict_tts_ref as ref

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
ENC = ("word_encoder_out", "context", "dur", "dict_attn", "pron_attn")


@pytest.fixture(autouse=True, scope="module")
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(n)


def make_model(hp, **extra):
    from dict_tts_amd import model
    m = model.PortaSpeech_dict(hparams={**hp, **extra})
    m.load_state_dict({k: T(v) for k, v in sd_np(hp).items()}, strict=True)
    return m


_MODELS = {}


def table_model(name):
    """the release model of shape `name` ("default" or an acoustic_ref.CONFIGS key) with the resident dictionary uploaded, one per module"""
    if name not in _MODELS:
        m = make_model(shape_hp(name))
        m.upload_dict_table(synth.dict_table(ar.SEED))
        _MODELS[name] = m
    return _MODELS[name]


@pytest.fixture(scope="module")
def default():
    yield table_model("default")
    _MODELS.clear()


def run(m, batch, z=None, m2w=None):
    b = {k: T(v) for k, v in batch.items()}
    r = m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
          (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=True, z_p=z,
          mel2word=None if m2w is None else T(m2w))
    return with_context(m, r, *batch["word_tokens"].shape)


def run_ids(m, sentences, batch, z=None, m2w=None):
    ib = synth.make_id_batch(sentences, synth.dict_table(ar.SEED), pron_every=3)
    assert np.array_equal(ib["word_tokens"], batch["word_tokens"]) and np.array_equal(ib["pron_modified"], batch["pron_modified"])
    r = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], z_p=z,
                      mel2word=None if m2w is None else T(m2w))
    return with_context(m, r, *batch["word_tokens"].shape)


def with_context(m, r, B, T_w):
    c = torch.empty(B, T_w, m.cfg.hidden_size, dtype=torch.float32, device="cuda")
    m.ctx.fetch(abi.OUT_CONTEXT, c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    r["context"] = c
    return r


def reference(hp, batch, m2w=None, z=None):
    """the float64 restatement; z: the same prior sample the GPU gets"""
    return ar.forward(ar.state(sd_np(hp), torch.float64), hp, *ar.inputs(batch, torch.float64),
                      mel2word=None if m2w is None else T(m2w), z_p=z)


def near_ties(want):
    """utterances whose predicted integer durations lie within 5e-5 of a rounding tie in the reference"""
    v = want["dur"].exp() - 1
    tie = ((v - v.floor() - 0.5).abs() < 5e-5) & (want["word_encoder_out"].abs().sum(-1) > 0)
    return set(int(b) for b in torch.nonzero(tie)[:, 0])


def mel2word_exact(case, got, want, fails):
    ties = near_ties(want)
    g, w = got["mel2word"].cpu(), want["mel2word"]
    for b in range(g.shape[0]):
        if b in ties:
            print(f"{case}: utterance {b} has a near-tie duration; its mel2word is not compared")
            continue
        n = min(g.shape[1], w.shape[1])
        if not (torch.equal(g[b, :n], w[b, :n]) and not g[b, n:].any() and not w[b, n:].any()):
            fails.append(f"{case}: mel2word of utterance {b} differs")


def noise(name, B, T4, Z=16):
    return T(synth.randn(ar.SEED, name, (B, Z, T4)))


# ------------------------------------------------------------------------------------------------------- default shape: tile edges
RC = ar.flow_rc()
SEAM_T4 = (1, 2, RC - 1, RC, RC + 1, 2 * RC, 2 * RC + 1)


def test_prior_flow_chunk_seams(default):
    fails = []
    words = [3, 5, 12, 12, 12, 20, 20]
    batch = ar.batch_of(words)
    m2w = ar.spread_mel2word(batch["word_tokens"], [4 * t for t in SEAM_T4])
    z = noise("seam.z", len(words), max(SEAM_T4))
    got, want = run(default, batch, z, m2w), reference({}, batch, m2w, z)
    assert torch.equal(got["mel2word"].cpu(), want["mel2word"])
    compare("flow seams ragged", got, want, ("mel_out",) + ENC, fails, batch)
    # the flowstack grid covers the PADDED T_mel/4 (the reverse flow is unmasked): in the batch every utterance runs as 2 RC + 1 rows, so
    # the chunk-count edges (one exact chunk at RC, a one-row last chunk at RC + 1 and 2 RC + 1, ...) are run at B = 1
    for i, t4 in enumerate(SEAM_T4):
        compare(f"flow seams B=1 T4={t4}", *single_flow_case(default, {}, words[i], t4, f"seam.z1.{i}"), ("mel_out",), fails)
    assert not fails, "\n".join(fails)


def single_flow_case(m, hp, words, t4, name):
    """B = 1, `words` words, teacher-forced to exactly 4 t4 frames -> (got, want)"""
    b1 = synth.make_batch(ar.sentences_of([words]), ar.SEED, pron_every=3)
    m1 = ar.spread_mel2word(b1["word_tokens"], [4 * t4])
    z1 = noise(name, 1, t4, synth.acoustic_shape(hp)["latent_size"])
    got, want = run(m, b1, z1, m1), reference(hp, b1, m1, z1)
    assert torch.equal(got["mel2word"].cpu(), want["mel2word"])
    return got, want


def test_posterior_forward_flow_chunk_seams(default):
    """the posterior pass's masked forward flow (flowstack, forward direction) on the seam lengths: z_p, m_q, logs_q, mel row by row"""
    fails = []
    words = [3, 5, 12, 12, 12, 20, 20]
    batch = ar.batch_of(words)
    m2w = ar.spread_mel2word(batch["word_tokens"], [4 * t for t in SEAM_T4])
    got, want = posterior(default, {}, batch, m2w, "seam")
    compare("posterior seams", got, want, ("mel_out",), fails, mel="mel_post")
    compare("posterior seams", {k: got[k].transpose(1, 2) for k in ("z_p", "m_q", "logs_q")},
            {k: want[k].transpose(1, 2) for k in ("z_p", "m_q", "logs_q")}, ("z_p", "m_q", "logs_q"), fails)
    kl_rel = abs(float(got["kl"]) - float(want["kl"])) / abs(float(want["kl"]))
    print(f"posterior seams: kl rel {kl_rel:.2e}")
    assert kl_rel <= ar.KL_REL, kl_rel
    assert not fails, "\n".join(fails)


def posterior(m, hp, batch, m2w, name):
    mels = pr.tgt_mels_for(m2w, name=f"{name}.mel")
    Z = synth.acoustic_shape(hp)["latent_size"]
    eps = synth.randn(ar.SEED, f"{name}.eps", (mels.shape[0], Z, mels.shape[1] // 4))
    b = {k: T(v) for k, v in batch.items()}
    with torch.no_grad():
        got = m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
                (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=False, tgt_mels=T(mels), mel2word=T(m2w),
                eps=T(eps))
    want = pr.forward_posterior(ar.state(sd_np(hp), torch.float64), *ar.inputs(batch, torch.float64), T(mels).double(), T(m2w),
                                T(eps).double(), hp=hp)
    return got, want


def test_decoder_tile_edges(default):
    """T_mel around the 64-row vconv tiles beside a 400-frame utterance (the batch's padded T_mel): every frame, then per utterance its own
    frames (where its first and last 4-frame groups of g_pre_poly act), its first and last WIN frames, and the padded frames after it
    (decoded unmasked, as the reference does).  The tiles cover the padded T_mel, so each length also runs alone (B = 1), where the
    tile edge falls at the utterance's end"""
    fails = []
    frames = (60, 64, 68, 124, 128, 132, 400)
    words = [6, 7, 8, 10, 11, 12, 30]
    batch = ar.batch_of(words, offset=300)
    m2w = ar.spread_mel2word(batch["word_tokens"], frames)
    z = noise("dec.z", len(frames), 100)
    got, want = run(default, batch, z, m2w), reference({}, batch, m2w, z)
    assert torch.equal(got["mel2word"].cpu(), want["mel2word"])
    compare("decoder tiles", got, want, ("mel_out",), fails)
    W = ar.WIN
    for b, n in enumerate(frames):
        u = slice(b, b + 1)
        compare(f"decoder tiles utt {b} frames [0, {n})", got, want, ("mel_out",), fails, sel=(u, slice(0, n)))
        compare(f"decoder tiles utt {b} first {W}", got, want, ("mel_out",), fails, sel=(u, slice(0, W)))
        compare(f"decoder tiles utt {b} last {W}", got, want, ("mel_out",), fails, sel=(u, slice(n - W, n)))
        if n < frames[-1]:
            compare(f"decoder tiles utt {b} padded [{n}, {frames[-1]})", got, want, ("mel_out",), fails, sel=(u, slice(n, None)))
    for i, n in enumerate(frames[:-1]):
        b1 = synth.make_batch(ar.sentences_of([words[i]], offset=300), ar.SEED, pron_every=3)
        m1 = ar.spread_mel2word(b1["word_tokens"], [n])
        z1 = noise(f"dec.z1.{i}", 1, n // 4)
        g1, w1 = run(default, b1, z1, m1), reference({}, b1, m1, z1)
        compare(f"decoder tiles B=1 T_mel={n}", g1, w1, ("mel_out",), fails)
    assert not fails, "\n".join(fails)


# (shape, word counts): the kernels choose their tiles from the batch's PADDED T_w (its longest utterance), and inside a tile they follow
# each utterance's length.  Padded T_w: 32, 64, 128 (whole 32-row conv tiles; at 128 the MFMA attention kernel's fourth query wave and
# fourth key tile are full), 100 (MFMA, partial fourth wave), 65, 129 (one row past a tile; split attention from 129 on), 161 (split).
# Per-utterance lengths only (inside a longer batch): 1, 2, 31, 33, 63, 97, 160.  The same padded lengths at hidden 384 (MFMA attention at
# C = 384, the D > 256 S2PA table form).
ENC_CASES = [("default", [1, 31, 32, 33, 63, 64, 65, 2]), ("default", [97, 100, 128]), ("default", [128, 129, 160, 161])] + \
            [("default", [n]) for n in (32, 64, 100, 128, 129, 161)] + \
            [("h384_heads4-mfma_c384-s2pa_table_d384", [97, 100, 128])] + \
            [("h384_heads4-mfma_c384-s2pa_table_d384", [n]) for n in (32, 64, 100, 128, 129)]


@pytest.mark.parametrize("shape,words", ENC_CASES, ids=[f"{s.split('-')[0]}-Tw_{'_'.join(map(str, w))}-B{len(w)}" for s, w in ENC_CASES])
def test_encoders_and_s2pa_word_counts(default, shape, words):
    """predicted durations on the GPU: the encoder outputs row by row against float64, integer durations (mel2word) exact except
    near-ties (the float64 durations through the length regulator); the id path too where every utterance has its BOS and EOS.  The
    float64 reference decodes a short teacher-forced mel2word (2 frames per word): the encoder outputs do not depend on it"""
    fails = []
    m, hp = table_model(shape), shape_hp(shape)
    batch = ar.batch_of(words, offset=500)
    short = ar.spread_mel2word(batch["word_tokens"], [2 * max(1, n) for n in words])
    want = reference(hp, batch, short, lambda B, T4: noise("enc.z", B, T4, synth.acoustic_shape(hp)["latent_size"]))
    want["mel2word"] = predicted_mel2word(want)
    got = run(m, batch)
    case = f"{shape} encoders T_w {words}"
    compare(case, got, want, ENC, fails, batch)
    mel2word_exact(case, got, want, fails)
    if 1 not in words:
        gi = run_ids(m, ar.sentences_of(words, offset=500), batch)
        compare(case + " ids", gi, want, ENC, fails, batch)
        mel2word_exact(case + " ids", gi, want, fails)
    assert not fails, "\n".join(fails)


def predicted_mel2word(want):
    """mel2word from the reference's durations (add_dur's rounding and length regulator, expand's pad to frames_multiple)"""
    weo = want["word_encoder_out"]
    d = torch.clamp(torch.round(want["dur"].exp() - 1), min=0).long()
    m2w = ref.length_regulator(d, (weo.abs().sum(-1) != 0).long().sum(-1))
    return ref.expand(weo, m2w)[2]


def test_encoders_batch_size_policy(default):
    """B = 90 utterances of 31-65 words against B = 6 of the same utterances, through the tensor API and the ids: every utterance's rows
    within the bounds.  The encoder convolutions carry a three-piece bf16 copy, so both batches run conv1d_short_kernel; what the batch
    size changes is launch_short_policy's parts-per-wave choice: one contraction part per wave at B = 6 (a 4x shorter chain per output
    tile), all four parts in one wave at B = 90 (270 tiles: the 4- and 2-wave forms would not stay co-resident)"""
    fails = []
    words = [65, 64, 63, 33, 32, 31]
    small = ar.batch_of(words, offset=800)
    want = reference({}, small, z=lambda B, T4: noise("pol.z", B, T4))
    sents = ar.sentences_of(words, offset=800) * 15
    big = synth.make_batch(sents, ar.SEED, pron_every=3)
    for b in range(6):   # pron_every counts over the whole batch: keep every copy's forced senses the same as in the small batch
        big["pron_modified"][b::6] = small["pron_modified"][b]
    idx = [b % 6 for b in range(90)]
    want90 = {k: (v[idx] if k != "mel2word" else v) for k, v in want.items() if k in ENC}
    for name, bt in (("B=6", small), ("B=90", big)):
        got = run(default, bt)
        compare(f"policy {name}", got, want if name == "B=6" else want90, ENC, fails, bt)
    ib = synth.make_id_batch(sents, synth.dict_table(ar.SEED), pron_every=3)
    ib["pron_modified"] = big["pron_modified"]
    r = default.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"])
    compare("policy ids B=90", with_context(default, r, 90, big["word_tokens"].shape[1]), want90, ENC, fails, big)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------- non-default shapes
def shape_case(hp):
    """words [12, 33, 65, 130] (the 130-word utterance crosses the attention threshold); T_mel/4 at RC - 1, RC, RC + 1 and 1.5 RC of the
    shape's flowstack chunk"""
    rc = ar.flow_rc(hp)
    words = [12, 33, 65, 130]
    batch = ar.batch_of(words, offset=1000)
    t4 = [rc - 1, rc, rc + 1, rc + rc // 2]
    m2w = ar.spread_mel2word(batch["word_tokens"], [4 * t for t in t4])
    z = noise("shape.z", 4, max(t4), synth.acoustic_shape(hp)["latent_size"])
    return words, batch, m2w, z


@pytest.mark.parametrize("name", sorted(ar.CONFIGS))
def test_nondefault_shape_end_to_end(name):
    hp = ar.CONFIGS[name]
    fails = []
    words, batch, m2w, z = shape_case(hp)
    m = make_model(hp)
    m.upload_dict_table(synth.dict_table(ar.SEED))
    want = reference(hp, batch, m2w, z)
    got = run(m, batch, z, m2w)
    assert torch.equal(got["mel2word"].cpu(), want["mel2word"])
    compare(name, got, want, ("mel_out",) + ENC, fails, batch)
    gi = run_ids(m, ar.sentences_of(words, offset=1000), batch, z, m2w)
    compare(name + " ids", gi, want, ("mel_out",) + ENC, fails, batch)
    if "flowstack" in name:   # the batch runs as one padded T_mel/4 = 1.5 RC: the chunk-count edges of this halo at B = 1
        rc = ar.flow_rc(hp)
        for t4 in (rc - 1, rc, rc + 1):
            compare(f"{name} B=1 T4={t4}", *single_flow_case(m, hp, 12, t4, f"shape.z1.{t4}"), ("mel_out",), fails)
    assert not fails, "\n".join(fails)


POSTERIOR = [n for n in sorted(ar.CONFIGS) if n.startswith(("fvae", "h256", "glow_blocks8"))]


@pytest.mark.parametrize("name", POSTERIOR)
def test_nondefault_shape_posterior(name):
    hp = ar.CONFIGS[name]
    fails = []
    _, batch, m2w, _ = shape_case(hp)
    got, want = posterior(make_model(hp), hp, batch, m2w, "shape")
    compare(name + " posterior", got, want, ("mel_out",), fails, mel="mel_post")
    compare(name + " posterior", {k: got[k].transpose(1, 2) for k in ("z_p", "m_q", "logs_q")},
            {k: want[k].transpose(1, 2) for k in ("z_p", "m_q", "logs_q")}, ("z_p", "m_q", "logs_q"), fails)
    kl_rel = abs(float(got["kl"]) - float(want["kl"])) / abs(float(want["kl"]))
    print(f"{name} posterior: kl rel {kl_rel:.2e}")
    assert kl_rel <= ar.KL_REL, kl_rel
    assert not fails, "\n".join(fails)


def test_posterior_refuses_a_latent_other_than_16():
    """latent_size 8 loads and infers (test_nondefault_shape_end_to_end); the posterior pass alone is refused, naming the hparam (the
    whole checkpoint failed to load before)"""
    hp = ar.CONFIGS["glow_k5_h128_latent8-flow_fallback"]
    _, batch, m2w, _ = shape_case(hp)
    with pytest.raises(abi.DttsError, match="supports latent_size 16.*latent_size 8"):
        posterior(make_model(hp), hp, batch, m2w, "refuse")


@pytest.mark.parametrize("blocks", [1, 3])
def test_odd_prior_glow_n_blocks_is_refused_by_name(blocks):
    with pytest.raises(RuntimeError, match=f"prior_glow_n_blocks {blocks}: an odd number of flow blocks is not supported"):
        make_model({"prior_glow_n_blocks": blocks})


REDZONE = ["h256_heads4-mha_dk64-s2pa_1x4-post_cond_f32", "h384_heads4-mfma_c384-s2pa_table_d384", "fvae160_k7_dec6-vconv",
           "glow_blocks8-flowstack_rc64", "glow_k5_h128_latent8-flow_fallback", "ffn9-conv_k9"]


@pytest.mark.parametrize("name", REDZONE)
def test_nondefault_shape_memory_safety(name):
    """debug_redzone (every workspace buffer and weight pack between red zones, workspaces NaN-filled): no zone damaged after the tensor
    and the id forward, and every output bit-identical to the release context's"""
    hp = ar.CONFIGS[name]
    words, batch, m2w, z = shape_case(hp)
    rel, dbg = make_model(hp), make_model(hp, dtts_debug_redzone=1)
    table = synth.dict_table(ar.SEED)
    rel.upload_dict_table(table)
    dbg.upload_dict_table(table)
    s = torch.cuda.current_stream().cuda_stream
    keys = ("mel_out", "mel2word") + ENC
    for path in ("tensor", "ids"):
        if path == "tensor":
            a, b = run(rel, batch, z, m2w), run(dbg, batch, z, m2w)
        else:
            sents = ar.sentences_of(words, offset=1000)
            a, b = run_ids(rel, sents, batch, z, m2w), run_ids(dbg, sents, batch, z, m2w)
        n = dbg.ctx.debug_check(s)
        assert n == 0, f"{name} {path}: {dbg.ctx.last_error()}"
        for k in keys:
            x, y = a[k].cpu(), b[k].cpu()
            assert torch.isfinite(y.float()).all() and torch.equal(x, y), (name, path, k)
