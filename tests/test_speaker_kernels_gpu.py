"""Speaker-conditioned text-to-mel row by row against the float64 restatement (tests/acoustic_ref.forward(form=, spk=),
tests/posterior_ref.forward_posterior), at the shapes where the conditioned kernels index differently (tests/speaker_shapes.py; run with
`-m gpu` on an MI355X).  tests/test_speaker_gpu.py holds one shape to whole-tensor gates against the fp32 goldens; a wrong speaker row on
one boundary row of one utterance passes those (tests/test_speaker_cpu.py plants it).

What is compared.
  * The projected rows themselves, element by element: the padded rows of the fetched word_encoder_out ARE the speaker rows.  Form "id":
    the bits of the table row.  Form "embed" with e = 0, a one-hot e or a single -1: the bits of fp32(+-W[o, k]) + bias[o] (the FMA chain
    adds exact zeros and one exact product).  General e: |row - row64| <= gamma_257 (sum_k |W[o,k] e[k]| + |bias[o]|), the textbook bound of
    a fixed-order fp32 chain of 256 FMAs and one add; the largest ratio to it is printed.  An utterance without a padded row (word count
    = T_w) is checked through its valid rows only (the row-by-row comparison below).
  * Every conditioned output against float64 with acoustic_ref.BOUNDS unchanged (max, 8-row window RMS, RMS; one T2MMEAS line each):
    word_encoder_out (valid and padded rows), context, dur, dict_attn, pron_attn with predicted durations, mel_out decoding a short
    teacher-forced mel2word; mel2word exact except near-ties (at most speaker_shapes.MAX_TIES utterances of a case, checked on the CPU);
    the posterior pass's mel_out, z_p, m_q, logs_q and kl.  In the row-mapping cases the first and the last valid row of every utterance
    on its own as well.
  * Batch and state: utterances bit-identical to themselves run alone; arming B = 2, 300, 2; out-of-range ids behind the gather's
    256-utterance search stride; debug_redzone; an embedding that stays on the device from the speaker encoder.

Measured on MI355X, worst over every case here (GPU - float64, max / 8-row window RMS / RMS; the case in brackets).  No bound of
acoustic_ref.BOUNDS is exceeded and none was added or changed; the conditioned figures lie at or below the unconditioned ones of
tests/test_text2mel_kernels_gpu.py:
  word_encoder_out   1.6e-5 / 2.1e-6 / 8.9e-7  (hidden 384, ids)     context      2.8e-5 / 3.2e-6 / 1.4e-6  (hidden 384, ids)
  dur                5.1e-6 / 2.2e-6 / 1.3e-6  (hidden 384; B = 257) dict_attn    5.8e-6 / 5.2e-7 / 2.2e-7  (hidden 384, ids)
  pron_attn          1.7e-6 / 6.0e-7 / 1.4e-7  (T_w 161, ids)        mel (infer)  3.6e-5 / 8.4e-6 / 6.9e-6  (glow_blocks8, id)
  posterior: mel 2.0e-4 / 5.1e-5 / 1.8e-5, z_p 9.8e-4 / 1.0e-4 / 4.2e-5, m_q 5.3e-5 / 1.5e-5 / 1.1e-5, logs_q 4.7e-5 / 1.5e-5 / 1.0e-5,
  kl relative 3.7e-6 (default shape, embed); word_encoder_out 8.5e-6 / 1.3e-6 / 4.6e-7 and dur 2.8e-6 / 1.4e-6 / 5.3e-7 (hidden 256).
The projection: every "id" row and every exact "embed" row (zero, one-hot at k = 0, 1, 127, 255, a single -1) bit-identical; general
embeddings reach at most 0.019 of the gamma_257 bound (hidden 256; 25 comparisons).  No utterance of any case was skipped as a near-tie.
Every utterance of the row-mapping batches and utterances 0, 254, 255, 256 of B = 257 equal themselves alone bit for bit, both forms.
Bugs these tests found: none.  All 77 tests passed on their first run on the device; the kernels are unchanged.
"""
import numpy as np
import pytest
import torch

import acoustic_ref as ar
import speaker_shapes as sh
from acoustic_ref import compare
from dict_tts_amd import abi, synth

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
ENC = ("word_encoder_out", "context", "dur", "dict_attn", "pron_attn")
bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.fixture(autouse=True, scope="module")
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(n)


def make_model(c, **extra):
    """the model of a case: its shape's hparams, its speaker form and num_spk, the seeded checkpoint with that spk_embed_proj"""
    from dict_tts_amd import model
    hp = {**ar.shape_hp(c["shape"]), "num_spk": c["num_spk"], "use_spk_id" if c["form"] == "id" else "use_spk_embed": True}
    m = model.PortaSpeech_dict(hparams={**hp, **extra})
    m.load_state_dict({k: T(v) for k, v in sh.state_np(c).items()}, strict=True)
    return m


_MODELS = {}


def model_of(c):
    """one release model per (shape, form, num_spk, checkpoint), the resident dictionary uploaded"""
    key = (c["shape"], c["form"], c["num_spk"], c["kind"] == "g11")
    if key not in _MODELS:
        m = make_model(c)
        m.upload_dict_table(synth.dict_table(ar.SEED))
        _MODELS[key] = m
    return _MODELS[key]


@pytest.fixture(autouse=True, scope="module")
def _models():
    yield
    _MODELS.clear()


def with_context(m, r, B, T_w):
    c = torch.empty(B, T_w, m.cfg.hidden_size, dtype=torch.float32, device="cuda")
    m.ctx.fetch(abi.OUT_CONTEXT, c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    r["context"] = c
    return r


def run(m, batch, spk, z=None, m2w=None):
    b = {k: T(v) for k, v in batch.items()}
    r = m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
          (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=True, z_p=None if z is None else T(z),
          mel2word=None if m2w is None else T(m2w), spk_embed=spk if torch.is_tensor(spk) else T(spk))
    return with_context(m, r, *batch["word_tokens"].shape)


def run_ids(m, name, spk, z=None, m2w=None):
    batch = sh.batch(name)
    ib = synth.make_id_batch(sh.sentences(name), synth.dict_table(ar.SEED), pron_every=3)
    assert np.array_equal(ib["word_tokens"], batch["word_tokens"]) and np.array_equal(ib["pron_modified"], batch["pron_modified"])
    r = m.forward_ids(T(ib["word_tokens"]), T(ib["entry_ids"]), T(ib["pron_modified"]), ib["L_k"], ib["P"], z_p=None if z is None else T(z),
                      mel2word=None if m2w is None else T(m2w), spk_embed=T(spk))
    return with_context(m, r, *batch["word_tokens"].shape)


def slice_batch(batch, u):
    return {k: np.ascontiguousarray(v[u:u + 1]) for k, v in batch.items()}


def mel2word_exact(case, got, want, fails):
    """got's predicted mel2word against the float64 durations through the length regulator; -> the utterances left uncompared"""
    g, w = got["mel2word"].cpu(), want["pred_mel2word"]
    n = min(g.shape[1], w.shape[1])
    for b in range(g.shape[0]):
        if b in want["ties"]:
            continue
        if not (torch.equal(g[b, :n], w[b, :n]) and not g[b, n:].any() and not w[b, n:].any()):
            fails.append(f"{case}: mel2word of utterance {b} differs")
    print(f"{case}: {len(want['ties'])} utterance(s) skipped as near-tie durations {want['ties']}")
    assert len(want["ties"]) <= sh.MAX_TIES


def projected_rows(case, c, weo, batch, fails):
    """the padded rows of the fetched word_encoder_out against the projection itself, element by element; -> the largest ratio to the
    gamma_257 bound (None where the rows must match bit for bit)"""
    pad = np.argwhere(batch["word_tokens"] == 0)
    full = sorted(set(range(batch["word_tokens"].shape[0])) - set(int(u) for u in pad[:, 0]))
    if full:
        print(f"{case}: utterances {full} have no padded row (word count = T_w): their speaker row is checked through their valid rows only")
    if not len(pad):
        return None
    g = weo.cpu().numpy()[pad[:, 0], pad[:, 1]]
    if c["form"] == "id" or c["kind"] == "exact":
        rows = sh.state_np(c)["spk_embed_proj.weight"][c["spk"]] if c["form"] == "id" else sh.exact_rows(c)
        bad = np.argwhere((bits(g) != bits(rows[pad[:, 0]])).any(1))[:, 0]
        if len(bad):
            u, t = pad[bad[0]]
            fails.append(f"{case}: the speaker row of utterance {u} (padded row {t}) is not bit-identical to its exact value "
                         f"({len(bad)} of {len(pad)} padded rows differ, max {np.abs(g - rows[pad[:, 0]]).max():.3g})")
        return None
    rows64, bound = sh.speaker_rows(c)
    ratio = np.abs(g.astype(np.float64) - rows64[pad[:, 0]]) / bound[pad[:, 0]]
    i, o = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"SPKPROJ {case}: largest |row - row64| / (gamma_257 (sum |W e| + |bias|)) = {ratio.max():.3g} at utterance {pad[i][0]} row "
          f"{pad[i][1]} channel {o}")
    if ratio.max() > 1:
        fails.append(f"{case}: projected row of utterance {pad[i][0]} channel {o} exceeds the fp32 chain bound {ratio.max():.3g}x")
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------- conditioned outputs, row by row
@pytest.mark.parametrize("name", [c["name"] for c in sh.INFER])
def test_conditioned_forward_row_by_row(name):
    c = sh.BY_NAME[name]
    batch, want, m = sh.batch(name), sh.reference(name), model_of(c)
    fails = []
    got = run(m, batch, c["spk"])                                          # predicted durations
    compare(name, got, want, ENC, fails, batch)
    mel2word_exact(name, got, want, fails)
    projected_rows(name, c, got["word_encoder_out"], batch, fails)
    m2w, z = sh.mel2word(name), sh.prior_noise(name)
    tf = run(m, batch, c["spk"], z, m2w)                                   # the short teacher-forced decode the reference ran
    assert torch.equal(tf["mel2word"].cpu(), want["mel2word"])
    compare(name + " teacher-forced", tf, want, ("mel_out",), fails)
    for k in ENC:                                                          # the encoder does not depend on the durations' source
        assert torch.equal(tf[k], got[k]), k
    if c["ids"]:
        gi = run_ids(m, name, c["spk"])
        compare(name + " ids", gi, want, ENC, fails, batch)
        mel2word_exact(name + " ids", gi, want, fails)
        projected_rows(name + " ids", c, gi["word_encoder_out"], batch, fails)
        ti = run_ids(m, name, c["spk"], z, m2w)
        compare(name + " ids teacher-forced", ti, want, ("mel_out",), fails)
    if c["kind"] == "rowmap":   # the rows where a workgroup of the speaker LayerNorm changes utterance
        for u, n in enumerate(sh.word_counts(name)):
            for t in sorted({0, n - 1}):
                compare(f"{name} utt {u} row {t} of {n}", got, want, ENC, fails, batch, sel=(slice(u, u + 1), slice(t, t + 1)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", [c["name"] for c in sh.POSTERIOR])
def test_conditioned_posterior_row_by_row(name):
    c = sh.BY_NAME[name]
    batch, m = sh.batch(name), model_of(c)
    m2w, mels, eps = sh.posterior_inputs(name)
    assert (m2w[1] == 0).sum() > (m2w[1][::-1] > 0).argmax() + 7       # utterance 1: zeros inside its span as well as behind it
    b = {k: T(v) for k, v in batch.items()}
    with torch.no_grad():
        got = m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
                (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=False, tgt_mels=T(mels), mel2word=T(m2w),
                eps=T(eps), spk_embed=T(c["spk"]))
    want = sh.posterior(name)
    fails = []
    compare(name, got, want, ("mel_out",), fails, mel="mel_post")
    lat = ("z_p", "m_q", "logs_q")
    compare(name, {k: got[k].transpose(1, 2) for k in lat}, {k: want[k].transpose(1, 2) for k in lat}, lat, fails)
    compare(name, got, want, ("word_encoder_out", "dur", "dict_attn", "pron_attn"), fails, batch)
    projected_rows(name, c, got["word_encoder_out"], batch, fails)
    kl_rel = abs(float(got["kl"]) - float(want["kl"])) / abs(float(want["kl"]))
    print(f"{name}: kl rel {kl_rel:.2e}")
    assert kl_rel <= ar.KL_REL, kl_rel
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------- batch and state behaviour
ALONE = [c["name"] for c in sh.ROWMAP] + ["wide_B257_spk1000-id", "wide_B257-embed"]


@pytest.mark.parametrize("name", ALONE)
def test_utterances_equal_themselves_run_alone(name):
    """log-durations and the valid word_encoder_out rows of an utterance in the batch = the same utterance alone (the same padded row)
    with its own speaker, bit for bit: every utterance of the row-mapping batches; the first, 255th, 256th and last of B = 257"""
    c = sh.BY_NAME[name]
    batch, m = sh.batch(name), model_of(c)
    rB = run(m, batch, c["spk"])
    counts = sh.word_counts(name)
    for u in (range(len(counts)) if c["kind"] == "rowmap" else (0, 254, 255, 256)):
        r1 = run(m, slice_batch(batch, u), c["spk"][u:u + 1])
        n = counts[u]
        for k in ("dur", "word_encoder_out"):
            a, b = r1[k][0, :n].cpu(), rB[k][u, :n].cpu()
            assert torch.equal(a, b), (name, u, k, float((a - b).abs().max()))


@pytest.mark.parametrize("form", sh.FORMS)
def test_arming_a_small_batch_after_a_wide_one(form):
    """B = 2, then B = 300, then B = 2 again in one speaker workspace: the two small runs are bit-identical"""
    wide = sh.BY_NAME["wide_B300_spk8-id" if form == "id" else "wide_B300-embed"]
    m = model_of(wide)
    big = sh.batch(wide["name"])
    small = {k: np.ascontiguousarray(v[1:3]) for k, v in big.items()}
    spk2 = wide["spk"][1:3]
    first = run(m, small, spk2)
    z = first["z_p_in"]
    first = run(m, small, spk2, z.cpu().numpy())
    run(m, big, wide["spk"])
    again = run(m, small, spk2, z.cpu().numpy())
    for k in ENC + ("mel_out", "mel2word"):
        assert torch.equal(first[k], again[k]), k


def test_out_of_range_ids_behind_the_search_stride():
    """the gather's range search at B = 257: an id out of range at utterance 256 alone (its second trip) is found; with utterance 3 out
    of range too, utterance 3 is the one named; -1, num_spk and 2^40; after each refusal a valid call gives the bits it gave before"""
    c = sh.BY_NAME["wide_B257_spk1000-id"]
    batch, m = sh.batch(c["name"]), model_of(c)
    z = run(m, batch, c["spk"])["z_p_in"].cpu().numpy()
    good = run(m, batch, c["spk"], z)
    keys = ENC + ("mel_out", "mel2word")
    for value in (-1, c["num_spk"], 1 << 40):
        for where, named in (((256,), 256), ((3, 256), 3)):
            bad = c["spk"].copy()
            bad[list(where)] = value
            with pytest.raises(abi.DttsError, match=rf"speaker id {value} of utterance {named} .*{c['num_spk']} rows"):
                run(m, batch, bad)
            after = run(m, batch, c["spk"], z)
            for k in keys:
                assert torch.equal(after[k], good[k]), (value, where, k)


REDZONE = ["rowmap_Tw5_B5-embed", "hidden_h384-embed", "hidden_h384-id", "wide_B300_spk8-id"]


@pytest.mark.parametrize("name", REDZONE)
def test_conditioned_forward_under_memory_safety_mode(name):
    """debug_redzone = 1 (every workspace between red zones, NaN-filled): no zone damaged by the projection, the conditioned encode and
    decode or the word_encoder_out fetch; every output bit-identical to the release context's (tensor API, and the ids where they run)"""
    c = sh.BY_NAME[name]
    batch, rel, dbg = sh.batch(name), model_of(c), make_model(c, dtts_debug_redzone=1)
    dbg.upload_dict_table(synth.dict_table(ar.SEED))
    m2w, z = sh.mel2word(name), sh.prior_noise(name)
    s = torch.cuda.current_stream().cuda_stream
    for path in ("tensor", "ids") if c["ids"] else ("tensor",):
        for tf in (False, True):
            args = (c["spk"], z, m2w) if tf else (c["spk"],)
            if path == "tensor":
                a = run(rel, batch, *args)
                b = run(dbg, batch, *args, **({} if tf else {"z": a["z_p_in"].cpu().numpy()}))
            else:
                a = run_ids(rel, name, *args)
                b = run_ids(dbg, name, *args, **({} if tf else {"z": a["z_p_in"].cpu().numpy()}))
            assert dbg.ctx.debug_check(s) == 0, f"{name} {path}: {dbg.ctx.last_error()}"
            for k in ENC + ("mel_out", "mel2word"):
                x, y = a[k].cpu(), b[k].cpu()
                assert torch.isfinite(y.float()).all() and torch.equal(x, y), (name, path, tf, k)


def test_conditioned_posterior_under_memory_safety_mode():
    name = "posterior_default-embed"
    c = sh.BY_NAME[name]
    batch, rel, dbg = sh.batch(name), model_of(c), make_model(c, dtts_debug_redzone=1)
    m2w, mels, eps = sh.posterior_inputs(name)
    b = {k: T(v) for k, v in batch.items()}
    out = []
    for m in (rel, dbg):
        with torch.no_grad():
            out.append(m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None,
                         (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=False, tgt_mels=T(mels),
                         mel2word=T(m2w), eps=T(eps), spk_embed=T(c["spk"])))
    assert dbg.ctx.debug_check(torch.cuda.current_stream().cuda_stream) == 0, dbg.ctx.last_error()
    for k in ("mel_out", "z_p", "m_q", "logs_q", "kl", "word_encoder_out", "dur"):
        assert torch.isfinite(out[1][k]).all() and torch.equal(out[0][k], out[1][k]), k


def test_embeddings_from_the_speaker_encoder_stay_on_the_device():
    """VoiceEncoder.embed_batch's [B, 256] device tensor passed as spk_embed = its host copy passed as a numpy array, bit for bit"""
    import spkenc_shapes as S
    from dict_tts_amd import speaker_encoder as E
    enc = E.VoiceEncoder.from_checkpoint({"model_state": synth.voice_encoder_state_dict(S.SEED)})
    wavs, lens = S.batch(("L31520", "L25600"), pad=5, fill=0.0)
    e = enc.embed_batch(torch.from_numpy(wavs), lens.tolist())["embed"]
    assert e.is_cuda and e.shape == (2, 256) and e.dtype == torch.float32 and torch.isfinite(e).all()
    c = sh.BY_NAME["rowmap_Tw7_B4-embed"]
    m = model_of(c)
    batch = {k: np.ascontiguousarray(v[:2]) for k, v in sh.batch(c["name"]).items()}
    dev = run(m, batch, e)
    host = run(m, batch, e.cpu().numpy(), dev["z_p_in"].cpu().numpy())
    for k in ENC + ("mel_out", "mel2word"):
        assert torch.equal(dev[k], host[k]), k
    rows = dev["word_encoder_out"][1, 1:].cpu()   # utterance 1 has one word: the speaker row of e[1] on every other row
    assert torch.equal(rows, rows[:1].expand_as(rows)) and not torch.equal(rows[0], dev["word_encoder_out"][0, 0].cpu())
