"""The validation losses on the GPU (run with `-m gpu` on an MI355X): dtts_text2mel_fetch(DTTS_OUT_LOSSES) and
``dict_tts_amd.losses.ValidationLosses`` against the float64 restatement (tests/losses_ref.py) over the cases of tests/losses_shapes.py.

Bounds.  l1 / mse sums: 1e-6 relative (one fp32 rounding of p - t would give 6e-8 per term; the kernel subtracts in fp64 and accumulates
in fp64).  count: exact.  SSIM: the map's largest deviation from float64 and every utterance's relative deviation of sum w (1 - ssim) may
not exceed what the reference's float32 path (losses_ref.ssim_map32) shows on the same inputs; where that path happens to deviate by
exactly 0, 1e-6 absolute (map) / 1e-9 relative (sum).  On top of that the map is held to 1e-6 absolute in EVERY case: it is one fp32
rounding (6e-8 for |ssim| <= 1) of an fp64 quotient whose moments carry about 121 x 36 x 1.1e-16 / C2 = 5e-10; a window that differed
from the reference's in one float32 ulp would move it by 1e-5 and more.  Duration sums: 1e-12 relative.

Measured on an MI355X (LABNOTES.md "Validation losses"): the ratio kernel deviation / float32-path deviation per case is printed by
test_mel_sums_and_ssim_accuracy.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import losses_ref as lr
import losses_shapes as ls
import posterior_ref as pr
from dict_tts_amd import abi, synth
from dict_tts_amd import losses as L

pytestmark = pytest.mark.gpu
T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
R = abi.LOSS_TILE_ROWS
SENT = -7.0   # the fill of every output buffer's guard band


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    return abi.Context()


@pytest.fixture(scope="module")
def mel_refs():
    """the float64 restatement and the float32 yardstick of every mel case, computed once"""
    out = {}
    torch.set_num_threads(8)
    for c in ls.MEL_CASES:
        pred, tgt, lens = ls.mel_inputs(c)
        T = c["T"]
        sums, count, m = lr.mel_sums64(pred[:, :T], tgt[:, :T])
        s32, m32 = lr.mel_sums32(pred[:, :T], tgt[:, :T])
        out[c["name"]] = dict(pred=pred, tgt=tgt, lens=lens, sums=sums, count=count, map=m, s32=s32, m32=m32)
    return out


def _run_mel(ctx, pred, tgt, T, want_map=True, bias=ls.BIAS):
    """raw ABI call on host arrays [B, ld, n_mel] -> sums [B, 3], count [B], map [B, T, n_mel] (numpy); checks the guard bands"""
    B, M = pred.shape[0], pred.shape[2]
    p, t = T_(pred).cuda(), T_(tgt).cuda()
    sums = torch.full((B * 3 + 8,), SENT, dtype=torch.float64, device="cuda")
    count = torch.full((B + 8,), -7, dtype=torch.int64, device="cuda")
    smap = torch.full((B * T * M + 64,), SENT, dtype=torch.float32, device="cuda") if want_map else None
    ctx.losses(B, _stream(), pred=p.data_ptr(), tgt=t.data_ptr(), T=T, n_mel=M, mel_sums=sums.data_ptr(), mel_count=count.data_ptr(),
               pred_ld=0 if pred.shape[1] == T else pred.shape[1], tgt_ld=0 if tgt.shape[1] == T else tgt.shape[1], bias=bias,
               ssim_map=None if smap is None else smap.data_ptr())
    torch.cuda.synchronize()
    assert (sums[B * 3:] == SENT).all() and (count[B:] == -7).all()
    assert torch.equal(p.cpu().view(torch.int32), T_(pred).view(torch.int32)) and torch.equal(t.cpu().view(torch.int32), T_(tgt).view(torch.int32))
    m = None
    if smap is not None:
        assert (smap[B * T * M:] == SENT).all()
        m = smap[:B * T * M].reshape(B, T, M).cpu().numpy()
    return sums[:B * 3].reshape(B, 3).cpu().numpy(), count[:B].cpu().numpy(), m


def _run_dur(ctx, dp, m2w, wl, scale, T_w=None, want_gt=True):
    B = dp.shape[0]
    T_w = dp.shape[1] if T_w is None else T_w
    d, m, w = T_(dp).cuda(), T_(m2w).cuda(), T_(np.asarray(wl, np.int32)).cuda()
    sums = torch.full((B * 5 + 8,), SENT, dtype=torch.float64, device="cuda")
    gt = torch.full((B * T_w + 8,), -7, dtype=torch.int32, device="cuda")
    ctx.losses(B, _stream(), dur_pred=d.data_ptr(), mel2word=m.data_ptr(), word_len=w.data_ptr(), T_w=T_w, T_mel=m2w.shape[1],
               dur_scale=0 if scale == "log" else 1, dur_sums=sums.data_ptr(), dur_gt=gt.data_ptr() if want_gt else None)
    torch.cuda.synchronize()
    assert (sums[B * 5:] == SENT).all() and (gt[B * T_w:] == -7).all()
    return sums[:B * 5].reshape(B, 5).cpu().numpy(), gt[:B * T_w].reshape(B, T_w).cpu().numpy()


def _rel(got, want):
    """elementwise |got - want| / |want|; 0 where both are 0, inf where only want is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return np.where(want == 0, np.where(got == 0, 0.0, np.inf), r)


@pytest.mark.parametrize("case", ls.MEL_CASES, ids=lambda c: c["name"])
def test_mel_sums_and_ssim_accuracy(ctx, mel_refs, case):
    ref = mel_refs[case["name"]]
    T = case["T"]
    sums, count, m = _run_mel(ctx, ref["pred"], ref["tgt"], T)
    assert np.isfinite(sums).all() and np.isfinite(m).all()          # (the NaN rows beyond T of ld_poisoned were not read)
    assert np.array_equal(count, ref["count"])
    rel = _rel(sums, ref["sums"])
    map_dev, map_yard = np.abs(m - ref["map"]).max(), np.abs(ref["m32"].astype(np.float64) - ref["map"]).max()
    sum_dev, sum_yard = rel[:, 2], _rel(ref["s32"], ref["sums"][:, 2])
    print(f"losses {case['name']}: l1 rel {rel[:, 0].max():.2e}, mse rel {rel[:, 1].max():.2e}; SSIM map dev {map_dev:.2e} vs float32 path {map_yard:.2e} "
          f"(ratio {map_dev / map_yard if map_yard else float('nan'):.2e}); SSIM sum rel {sum_dev.max():.2e} vs {sum_yard.max():.2e} "
          f"(ratio {sum_dev.max() / sum_yard.max() if sum_yard.max() else float('nan'):.2e})")
    assert (rel[:, :2] <= 1e-6).all(), rel
    assert map_dev <= (map_yard if map_yard > 0 else 1e-6), (map_dev, map_yard)
    assert map_dev <= 1e-6, map_dev
    for b in range(sums.shape[0]):
        assert sum_dev[b] <= (sum_yard[b] if sum_yard[b] > 0 else 1e-9), (b, sum_dev, sum_yard)
    if case["all_zero"] is not None:
        b = case["all_zero"]
        assert count[b] == 0 and not sums[b].any()
        fig = L.mel_figures(sums, count)
        assert all(np.isfinite(float(fig[k])) for k in ("l1", "mse", "ssim")) and torch.isnan(fig["ssim_utt"][b])
        assert np.allclose([float(fig[k]) for k in ("l1", "mse", "ssim")], lr.batch_figures(ref["sums"], ref["count"]), rtol=1e-6, atol=0)
    for b, t in case["zero_rows"]:   # the silent frame has weight 0 although its neighbours count
        assert count[b] == (ref["lens"][b] - sum(1 for bb, _ in case["zero_rows"] if bb == b)) * case["n_mel"]


def test_mel_determinism_and_batch_invariance(ctx, mel_refs):
    ref = mel_refs[f"T{2 * R + 3}"]
    T = 2 * R + 3
    pred, tgt = ref["pred"], ref["tgt"]
    s0, c0, m0 = _run_mel(ctx, pred, tgt, T)
    s1, c1, m1 = _run_mel(ctx, pred, tgt, T)
    assert np.array_equal(s0.view(np.int64), s1.view(np.int64)) and np.array_equal(c0, c1) and np.array_equal(m0.view(np.int32), m1.view(np.int32))
    for b in range(pred.shape[0]):   # alone at the same T
        sa, ca, ma = _run_mel(ctx, pred[b:b + 1], tgt[b:b + 1], T)
        assert np.array_equal(sa[0].view(np.int64), s0[b].view(np.int64)) and ca[0] == c0[b], b
        assert np.array_equal(ma[0].view(np.int32), m0[b].view(np.int32)), b
    perm = [2, 0, 1, 0]              # any position, any neighbours
    sp, cp, _ = _run_mel(ctx, pred[perm], tgt[perm], T, want_map=False)
    for i, b in enumerate(perm):
        assert np.array_equal(sp[i].view(np.int64), s0[b].view(np.int64)) and cp[i] == c0[b], (i, b)
    # NOT the same as alone at a shorter T: utterance 1 ends early, its rows behind the end hold 6.0 after the bias here, zero there
    n = int(ref["lens"][1])
    short, _, _ = _run_mel(ctx, pred[1:2, :n], tgt[1:2, :n], n, want_map=False)
    assert short[0, 2] != s0[1, 2] and np.array_equal(short[0, :2].view(np.int64), s0[1, :2].view(np.int64))


@pytest.mark.parametrize("case", ls.DUR_CASES, ids=lambda c: c["name"])
def test_duration_sums(ctx, case):
    dp, m2w, wl = ls.dur_inputs(case)
    want, d = lr.dur_sums64(dp, m2w, wl, case["scale"])
    got, gt = _run_dur(ctx, dp, m2w, wl, case["scale"])
    assert np.array_equal(gt, d)
    rel = _rel(got, want)
    print(f"losses {case['name']}: duration sums rel {rel.max(0)}")
    assert (rel <= 1e-12).all(), (got, want, rel)
    assert np.array_equal(got[:, [1, 3]], want[:, [1, 3]])
    again, _ = _run_dur(ctx, dp, m2w, wl, case["scale"], want_gt=False)
    assert np.array_equal(got.view(np.int64), again.view(np.int64))
    for b in range(dp.shape[0]):   # alone = in the batch
        one, _ = _run_dur(ctx, dp[b:b + 1], m2w[b:b + 1], wl[b:b + 1], case["scale"])
        assert np.array_equal(one[0].view(np.int64), got[b].view(np.int64)), b


def test_duration_ignores_indices_outside_the_words_and_follows_ieee(ctx):
    dp, m2w, wl = ls.dur_inputs(ls.DUR_BY_NAME["Tw7_log"])
    base, gt0 = _run_dur(ctx, dp, m2w, wl, "log")
    m = m2w.copy()
    m[:, -3:] = [8, -1, 1 << 40]      # beyond T_w, negative, far outside: ignored like the padding index 0
    got, gt = _run_dur(ctx, dp, m, wl, "log")
    assert np.array_equal(gt, gt0) and np.array_equal(got.view(np.int64), base.view(np.int64))
    bad = dp.copy()
    bad[0, 0], bad[1, 0] = -1.0, -3.0   # log(0) = -inf, log(-2) = NaN: not special-cased
    got, _ = _run_dur(ctx, bad, m2w, wl, "log")
    want, _ = lr.dur_sums64(bad, m2w, wl, "log")
    assert np.isinf(got[0, 2]) and got[0, 4] == -np.inf and np.isnan(got[1, 2]) and np.isnan(got[1, 4])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert (_rel(got[2], want[2]) <= 1e-12).all()


def test_invalid_arguments_are_refused_by_name(ctx):
    c = ls.MEL_BY_NAME["T11"]
    pred, tgt, _ = ls.mel_inputs(c)
    p, t = T_(pred).cuda(), T_(tgt).cuda()
    sums, count = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    dp, m2w, wl = ls.dur_inputs(ls.DUR_BY_NAME["Tw7_log"])
    d, m, w = T_(dp).cuda(), T_(m2w).cuda(), T_(wl.astype(np.int32)).cuda()
    dsums = torch.zeros(16, dtype=torch.float64, device="cuda")
    mel = dict(pred=p.data_ptr(), tgt=t.data_ptr(), T=11, n_mel=80, mel_sums=sums.data_ptr(), mel_count=count.data_ptr())
    dur = dict(dur_pred=d.data_ptr(), mel2word=m.data_ptr(), word_len=w.data_ptr(), T_w=7, T_mel=m2w.shape[1], dur_sums=dsums.data_ptr())

    def refused(match, B=3, **kw):
        with pytest.raises(abi.DttsError, match=match):
            ctx.losses(B, _stream(), **kw)

    refused(r"\(-22\).*B = 0", B=0, **mel)
    refused(r"\(-22\).*B = -2", B=-2, **dur)
    refused(r"\(-22\).*T = 0", **{**mel, "T": 0})
    refused(r"\(-22\).*n_mel = 0", **{**mel, "n_mel": 0})
    refused(r"\(-22\).*n_mel = 129", **{**mel, "n_mel": 129})
    refused(r"\(-22\).*pred_ld = 10", **{**mel, "pred_ld": 10})
    refused(r"\(-22\).*tgt_ld = 3", **{**mel, "tgt_ld": 3})
    refused(r"\(-22\).*null pred_dev", **{**mel, "pred": None})
    refused(r"\(-22\).*null pred_dev / tgt_dev", **{**mel, "tgt": None})
    refused(r"\(-22\).*mel_count_dev", **{**mel, "mel_count": None})
    refused(r"\(-22\).*pred_dev = 0x[0-9a-f]+ is not aligned to 4", **{**mel, "pred": p.data_ptr() + 2})
    refused(r"\(-22\).*mel_sums_dev = 0x[0-9a-f]+ is not aligned to 8", **{**mel, "mel_sums": sums.data_ptr() + 4})
    refused(r"\(-22\).*bias = (inf|nan)", **{**mel, "bias": float("inf")})
    refused(r"\(-22\).*dur_scale = 2", **{**dur, "dur_scale": 2})
    refused(r"\(-22\).*T_w = 0", **{**dur, "T_w": 0})
    refused(rf"\(-22\).*T_w = {abi.LOSS_MAX_WORDS + 1}", **{**dur, "T_w": abi.LOSS_MAX_WORDS + 1})
    refused(r"\(-22\).*m2w_ld = 4", **{**dur, "m2w_ld": 4})
    refused(r"\(-22\).*null dur_pred_dev", **{**dur, "dur_pred": None})
    refused(r"\(-22\).*word_len_dev", **{**dur, "word_len": None})
    refused(r"\(-22\).*mel2word_dev", **{**dur, "mel2word": None})
    refused(r"\(-22\).*mel2word_dev = 0x[0-9a-f]+ is not aligned to 8", **{**dur, "mel2word": m.data_ptr() + 4})
    refused(r"\(-22\).*no half requested", **{**mel, "mel_sums": None})
    a = abi.LossArgs(C.sizeof(abi.LossArgs) - 8, 3)
    assert ctx.lib.dtts_text2mel_fetch(ctx.h, abi.OUT_LOSSES, C.byref(a), None) == -22
    assert f"size = {C.sizeof(abi.LossArgs) - 8}" in ctx.last_error()
    # nothing was written by a refused call, and both halves run in one call
    assert not sums.any() and not dsums.any()
    ctx.losses(3, _stream(), **mel, **dur)
    torch.cuda.synchronize()
    want, cnt, _ = lr.mel_sums64(pred, tgt)
    assert (_rel(sums[:9].reshape(3, 3).cpu().numpy()[:, :2], want[:, :2]) <= 1e-6).all() and np.array_equal(count[:3].cpu().numpy(), cnt)
    assert (_rel(dsums[:15].reshape(3, 5).cpu().numpy(), lr.dur_sums64(dp, m2w, wl, "log")[0]) <= 1e-12).all()


def test_memory_safety_losses(ctx, mel_refs):
    """debug_redzone = 1: the workspace of the tile sums and the window sit between red zones; no launch damages one, and the results are
    the plain context's, bit for bit"""
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg = abi.Context(cfg)
    for name in (f"T{2 * R + 3}", f"T{R + 1}_m128", "T1", "ld_poisoned"):
        ref = mel_refs[name]
        T = ls.MEL_BY_NAME[name]["T"]
        s, c, m = _run_mel(dbg, ref["pred"], ref["tgt"], T)
        assert dbg.debug_check(_stream()) == 0, dbg.last_error()
        s0, c0, m0 = _run_mel(ctx, ref["pred"], ref["tgt"], T)
        assert np.array_equal(s.view(np.int64), s0.view(np.int64)) and np.array_equal(c, c0) and np.array_equal(m.view(np.int32), m0.view(np.int32))
    dp, m2w, wl = ls.dur_inputs(ls.DUR_BY_NAME["Tw300_log"])
    got, _ = _run_dur(dbg, dp, m2w, wl, "log")
    assert dbg.debug_check(_stream()) == 0, dbg.last_error()
    assert np.array_equal(got.view(np.int64), _run_dur(ctx, dp, m2w, wl, "log")[0].view(np.int64))
    dbg.close()


def test_validation_losses_mel_and_dur_figures(mel_refs):
    v = L.ValidationLosses(hparams={})
    ref = mel_refs[f"T{R + 1}"]
    out = v.mel(ref["pred"], ref["tgt"], ssim_map=True)
    want = lr.batch_figures(ref["sums"], ref["count"])
    assert np.allclose([float(out[k]) for k in ("l1", "mse", "ssim")], want, rtol=1e-6, atol=0)
    assert np.allclose(out["ssim_utt"].cpu().numpy(), ref["sums"][:, 2] / ref["count"], rtol=1e-6, atol=0)
    assert out["ssim_map"].shape == ref["map"].shape and out["count"].dtype == torch.int64 and out["l1"].dtype == torch.float64
    for scale in ("log", "linear"):
        dp, m2w, wl = ls.dur_inputs(ls.DUR_BY_NAME[f"Tw64_{scale}"])
        d = v.dur(dp, m2w, wl, dur_scale=scale)
        sums, gt = lr.dur_sums64(dp, m2w, wl, scale)
        assert np.allclose([float(d["wdur"]), float(d["sdur"]), float(d["wdur_train"])], lr.dur_figures(sums), rtol=1e-12, atol=0)
        assert np.array_equal(d["dur_gt"].cpu().numpy(), gt)


def _g12_model():
    from dict_tts_amd import model
    m = model.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: T_(v) for k, v in pr.g12_state_dict("plain").items()}, strict=True)
    return m


def test_run_model_on_the_g12_posterior_case_and_the_infer_path_stays(golden_dir):
    g12 = np.load(os.path.join(golden_dir, "g12_posterior.npz"))
    m = _g12_model()
    batch = pr.g12_batch()
    m2w = g12["mel2word_in"]
    mels = pr.tgt_mels_for(m2w)
    b = {k: T_(v) for k, v in batch.items()}
    sample = dict(b, mel2word=T_(m2w), mels=T_(mels), word_lengths=T_((batch["word_tokens"] > 0).sum(1)), eps=T_(g12["plain.eps"]), nsamples=5)
    dm = (b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"])
    z = T_(synth.noise(pr.SEED, 5, mels.shape[1] // 4, "g12.iso"))
    infer = lambda: m((b["word_tokens"], None), b["pron_modified"], (None, None, None), None, None, dm, infer=True, z_p=z, mel2word=T_(m2w))
    before = infer()

    v = L.ValidationLosses(hparams={}, ctx=m.ctx)      # the model's own handle
    losses, out = v.run_model(m, sample)
    assert list(losses.keys()) == ["kl", "ssim", "l1", "wdur", "sdur"]
    kl = float(out["kl"])
    assert abs(kl - float(g12["plain.kl"])) <= 1e-4 * abs(float(g12["plain.kl"]))
    assert float(losses["kl"]) == max(kl * 1.0, 0.002)
    unit = v.mel(out["mel_out"], mels)
    assert float(losses["ssim"]) == float(unit["ssim"]) * 0.5 and float(losses["l1"]) == float(unit["l1"]) * 0.5
    du = v.dur(out["dur"], m2w, sample["word_lengths"])
    assert float(losses["wdur"]) == float(du["wdur"]) and float(losses["sdur"]) == float(du["sdur"])
    # ... and those are the float64 restatement's figures on the returned tensors
    s64, c64, _ = lr.mel_sums64(out["mel_out"].cpu().numpy(), mels)
    fig = lr.batch_figures(s64, c64)
    assert abs(float(unit["l1"]) - fig[0]) <= 1e-6 * fig[0] and abs(float(unit["ssim"]) - fig[2]) <= 1e-6 * fig[2]
    assert np.array_equal(unit["count"].cpu().numpy(), (np.abs(mels).sum(-1) != 0).sum(1) * 80)
    d64, gt = lr.dur_sums64(out["dur"].cpu().numpy(), m2w, sample["word_lengths"].numpy(), "log")
    assert np.allclose([float(du["wdur"]), float(du["sdur"])], lr.dur_figures(d64)[:2], rtol=1e-12, atol=0)
    assert np.array_equal(du["dur_gt"].cpu().numpy(), gt)

    step = v.validation_step(m, sample)
    assert step["nsamples"] == 5 and list(step["losses"].keys()) == list(losses.keys())
    assert step["losses"] == {k: float(x) for k, x in losses.items()}
    assert step["total_loss"] == sum(step["losses"].values())
    floor = L.ValidationLosses(hparams={"lambda_kl": 1e-9}, ctx=m.ctx).run_model(m, sample)[0]
    assert float(floor["kl"]) == 0.002

    after = infer()
    for k in ("mel_out", "dur", "x_mask", "mel2word", "word_encoder_out"):
        assert torch.equal(before[k], after[k]), k
