"""The multi-window mel discriminator on the GPU (dict_tts_amd/mel_discriminator.py, csrc/meldisc.hip) against the float64 restatement
tests/meldisc_ref.py, which tests/test_meldisc_cpu.py holds against the reference.

Gates.
  * D per (utterance, window): max |D - D64| / max |D64| (over both signals' clips) <= 8 x e_ref[run][w], e_ref being the reference's own
    float32 error against its float64 in tests/golden/g17_meldisc.npz, normalised the same way; the hidden maps of the 32-frame window
    likewise against 8 x e_h[run][l].  The kernels and the reference's float32 form the same exact products and differ in summation order
    only (here one fp32 chain over K <= 2304 terms): the margin 8 is test_disc_gpu.py's, not a number chosen from these results.  The
    measured ratios are printed.
  * the fp64 sums: 1e-12 relative of the same sums formed in float64 from the GPU's own D.
  * the figures: a mean of (1 - D)^2 or D^2 moves by at most 2 (1 + max |D|) dD + dD^2 per element.
  * an utterance alone and inside a batch, and a second call after the workspace grew: bit-identical.
"""
import os

import numpy as np
import pytest
import torch

import meldisc_ref as mr
import meldisc_shapes as ms
from dict_tts_amd import abi, synth
from dict_tts_amd import mel_discriminator as M

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_meldisc.npz")
MARGIN = 8.0


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_STATE, _W64, _DISC, _REF = {}, {}, {}, {}


def state(run):
    rid = ms.run_id(run)
    if rid not in _STATE:
        _STATE[rid] = synth.mel_disc_state_dict(ms.SEED, run[0], run[1], run[3], run[2])
    return _STATE[rid]


def w64(run):
    rid = ms.run_id(run)
    if rid not in _W64:
        _W64[rid] = M.fold_state_dict(state(run), np.float64)
    return _W64[rid]


def disc(run):
    rid = ms.run_id(run)
    if rid not in _DISC:
        _DISC[rid] = M.MelDiscriminator.from_checkpoint({"state_dict": {"mel_disc": state(run)}}, hparams={"disc_norm": run[0], "disc_reduction": run[2]})
    return _DISC[rid]


def ref(run, case, b):
    key = (ms.run_id(run), case["name"], b)
    if key not in _REF:
        g, p = ms.utterance(case, b)
        _REF[key] = mr.score_utterance(w64(run), g, p, [ms.starts_of(case, b, win) for win in ms.WINS[:run[3]]])
    return _REF[key]


def score(d, case, pad=3):
    g, p, lens = ms.batch(case, pad)
    kw = {}
    if case.get("extra"):
        kw["starts"] = [ms.case_starts(case, win) for win in ms.WINS[:d.win_num]]
    elif "hop" in case:
        kw["hop"] = case["hop"]
    out = d.scores(torch.from_numpy(g), torch.from_numpy(p), lens, return_d=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)


def clips_of(d, w, s, n_out):
    """the D rows of signal s's clips of window w, in slot order: [n_clips, n_out]"""
    rows = d[w, s]
    live = ~np.isnan(rows[:, 0])
    assert np.all(np.isnan(rows[~live])) and np.all(np.isnan(rows[:, n_out:]))      # nothing written where there is no clip or no output
    return rows[live][:, :n_out]


@pytest.mark.parametrize("run,name", ms.RUN_CASES, ids=[f"{ms.run_id(r)}-{n}" for r, n in ms.RUN_CASES])
def test_case_against_restatement(golden, run, name):
    case, rid, n_win = ms.CASE_BY_NAME[name], ms.run_id(run), run[3]
    got = score(disc(run), case)
    B = len(case["lens"])
    e_ref, d_max = golden["e_ref." + rid], golden["d_max." + rid]
    assert np.all(got["status"] == 0)
    refs = [ref(run, case, b) for b in range(B)]
    for b, r in enumerate(refs):
        for w in range(n_win):
            n_out = ms.WINS[w] // 8 if run[2] == "none" else 1
            dg, dp = clips_of(got["d"], w, b, n_out).astype(np.float64), clips_of(got["d"], w, B + b, n_out).astype(np.float64)
            assert dg.shape == r["d_g"][w].shape and dp.shape == r["d_p"][w].shape, (name, b, w, dg.shape, r["d_g"][w].shape)
            assert got["counts"][b, w] == got["counts"][B + b, w] == r["counts"][0, w]
            for s, d in ((b, dg), (B + b, dp)):
                own = np.array([((1 - d) ** 2).sum(), (d ** 2).sum()])
                assert np.all(np.abs(got["sums"][s, w] - own) <= 1e-12 * own), (name, s, w, got["sums"][s, w], own)   # (0 clips: 0 == 0)
            if dg.size == 0:
                continue
            assert np.all(np.isfinite(dg)) and np.all(np.isfinite(dp))                # the NaN padding never reaches a result
            scale = max(np.abs(r["d_g"][w]).max(), np.abs(r["d_p"][w]).max())
            err = max(np.abs(dg - r["d_g"][w]).max(), np.abs(dp - r["d_p"][w]).max()) / scale
            print(f"{rid} {name}.{b} w{w}: {dg.size} D, error {err:.3e} = {err / e_ref[w]:.2f} x e_ref")
            assert err <= MARGIN * e_ref[w], (rid, name, b, w, err, e_ref[w])
    assert np.all(got["counts"][:, n_win:] == 0) and np.all(np.isnan(got["sums"][:, n_win:]))   # windows the model lacks: untouched
    if name == "short":
        assert np.all(got["counts"] == 0) and np.all(got["sums"][:, :n_win] == 0)
    if case.get("kind") == "same":
        assert np.array_equal(bits(got["sums"][0, :n_win, 0]), bits(got["sums"][B, :n_win, 0]))   # r and a from the same D
        assert np.array_equal(bits(got["d"][:, 0]), bits(got["d"][:, B]))
    want = mr.figures(np.concatenate([np.stack([r["sums"][0] for r in refs]), np.stack([r["sums"][1] for r in refs])]),
                      np.concatenate([np.stack([r["counts"][0] for r in refs]), np.stack([r["counts"][1] for r in refs])]), n_win)
    dD = MARGIN * e_ref * d_max * 2          # (d_max: over the fixture's cases; twice it covers every case's own scale)
    tol = 2 * (1 + 2 * d_max) * dD + dD ** 2
    for n in ("r", "f", "a"):
        assert np.array_equal(np.isnan(got[n]), np.isnan(want[n])), n
        ok = ~np.isnan(want[n])
        assert np.all(np.abs(got[n] - want[n])[ok] <= np.broadcast_to(tol, want[n].shape)[ok]), (n, got[n], want[n])
        okw = ~np.isnan(want[n + "_win"])
        assert np.all(np.abs(got[n + "_win"] - want[n + "_win"])[okw] <= tol[okw])
        if okw.any():
            assert abs(got[n + "_batch"] - want[n + "_batch"]) <= tol.max(), n
        else:
            assert np.isnan(got[n + "_batch"])


@pytest.mark.parametrize("norm", ["in", "bn", "sn"])
def test_hidden_maps_of_the_32_frame_window(golden, norm):
    run = (norm, 128, "stack", 3, None)
    rid = ms.run_id(run)
    g, _ = ms.utterance(ms.CASE_BY_NAME[ms.HIDDEN_CASE], ms.HIDDEN_B)
    ret = disc(run).forward(torch.from_numpy(g)[None], [[ms.HIDDEN_START], [0], [0]])
    torch.cuda.synchronize()
    assert len(ret["h"]) == 9 and ret["y"].shape == (1, 1, 3)
    _, h64 = mr.window_forward(w64(run), 0, g[ms.HIDDEN_START:ms.HIDDEN_START + 32])
    for l in range(3):
        mine = ret["h"][l][0].cpu().numpy().astype(np.float64)
        assert mine.shape == h64[l].shape == (128, 16 >> l, 40 >> l)
        err = np.abs(mine - h64[l]).max() / np.abs(h64[l]).max()
        e_h = golden["e_h." + rid][l]
        print(f"{rid} h{l}: error {err:.3e} = {err / e_h:.2f} x e_h")
        assert err <= MARGIN * e_h, (rid, l, err, e_h)
        sub = mine[ms.HIDDEN_CH]
        assert np.abs(sub - golden[f"h.{rid}.{l}.f64"]).max() <= MARGIN * e_h * np.abs(h64[l]).max()      # and against the reference itself


@pytest.mark.parametrize("run", [r for r in ms.RUNS if r[1] == 128 and r[3] == 3], ids=ms.run_id)
def test_forward_against_the_fixture(golden, run):
    rid, d = ms.run_id(run), disc(run)
    e_ref, d_max = golden["e_ref." + rid], golden["d_max." + rid]
    for fw in ms.FORWARD:
        x = ms.batch(ms.CASE_BY_NAME[fw["case"]], fill=0.0)[0]
        B = x.shape[0]
        ret = d.forward(torch.from_numpy(x), [[s] * B for s in fw["starts"]])
        torch.cuda.synchronize()
        k = f"{rid}.{fw['name']}"
        assert (ret["y"] is None) == bool(golden[k + ".y_none"]) and len(ret["h"]) == int(golden[k + ".n_h"])
        assert ret["start_frames_wins"][:2] == [[fw["starts"][0]] * B, [fw["starts"][1]] * B]
        if ret["y"] is None:
            assert [tuple(t.shape) for t in ret["h"][:3]] == [(B, 128, 16, 40), (B, 128, 8, 20), (B, 128, 4, 10)]
            continue
        y, y64 = ret["y"].cpu().numpy().astype(np.float64), golden[k + ".y.f64"]
        assert y.shape == y64.shape and ret["y"].dtype == torch.float32
        if run[2] == "sum":
            err, bound = np.abs(y - y64).max(), MARGIN * (e_ref * d_max).sum()      # the three windows' errors add
            print(f"{k}: |y - y64| {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            continue
        cols = np.cumsum([0] + [w // 8 for w in ms.WINS]) if run[2] == "none" else np.arange(4)
        for w in range(3):
            a, c = (y[..., cols[w]:cols[w + 1]], y64[..., cols[w]:cols[w + 1]])
            err = np.abs(a - c).max() / np.abs(c).max()
            print(f"{k} w{w}: error {err:.3e} = {err / e_ref[w]:.2f} x e_ref")
            assert err <= MARGIN * e_ref[w], (k, w, err)
    # without starts one start per window is drawn on the host, numpy.random.randint as `clip` draws it
    x = ms.batch(ms.CASE_BY_NAME["mixed"], fill=0.0)[0]
    np.random.seed(11)
    drawn = d.forward(torch.from_numpy(x))
    np.random.seed(11)
    want = [[int(np.random.randint(low=0, high=200 - w + 1))] * 3 for w in ms.WINS]
    assert drawn["start_frames_wins"] == want
    again = d.forward(torch.from_numpy(x), want)
    assert torch.equal(drawn["y"], again["y"])


def test_alone_equals_in_batch():
    run = ms.RUNS[0]
    case = ms.CASE_BY_NAME["mixed"]
    d = disc(run)
    inb = score(d, case, pad=5)
    B = len(case["lens"])
    for b in range(B):
        g, p = ms.utterance(case, b)
        out = d.scores(torch.from_numpy(g)[None], torch.from_numpy(p)[None], return_d=True)
        torch.cuda.synchronize()
        one = {k: v.cpu().numpy() for k, v in out.items()}
        for s1, sb in ((0, b), (1, B + b)):
            assert np.array_equal(bits(one["sums"][s1, :3]), bits(inb["sums"][sb, :3])), b
            assert np.array_equal(one["counts"][s1], inb["counts"][sb]), b
            for w in range(3):
                assert np.array_equal(bits(clips_of(one["d"], w, s1, 1)), bits(clips_of(inb["d"], w, sb, 1))), (b, w)


def test_memory_safety_and_grown_workspace():
    """debug_redzone = 1: every workspace buffer sits between red zones and starts out as 0xFF; no launch damages a zone, no stale word
    reaches an output; and a call after the workspace grew equals the call before"""
    run = ms.RUNS[0]
    cfg = abi.default_config()
    cfg.debug_redzone = 1
    dbg_ctx = abi.Context(cfg)
    dbg = M.MelDiscriminator.from_checkpoint(state(run), ctx=dbg_ctx)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    small, large = ms.CASE_BY_NAME["w32_edge"], ms.CASE_BY_NAME["mixed"]
    first = score(dbg, small)
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    big = score(dbg, large)                                               # the workspace grows
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    second = score(dbg, small)
    assert dbg_ctx.debug_check(stream()) == 0, dbg_ctx.last_error()
    plain_small, plain_big = score(disc(run), small), score(disc(run), large)
    for k in ("sums", "counts", "d"):
        assert np.array_equal(bits(first[k]), bits(second[k])), k
        assert np.array_equal(bits(first[k]), bits(plain_small[k])), k
        assert np.array_equal(bits(big[k]), bits(plain_big[k])), k
    dbg_ctx.close()


def test_validation_losses_report_the_adversarial_terms():
    """losses.ValidationLosses(mel_disc=...).adversarial: the lengths are the target's non-zero frames, the figures are scores' own"""
    from dict_tts_amd import losses
    d = disc(ms.RUNS[0])
    g, p, lens = ms.batch(ms.CASE_BY_NAME["mixed"], pad=4, fill=0.0)
    vl = losses.ValidationLosses(mel_disc=d)
    got = vl.adversarial(torch.from_numpy(p), torch.from_numpy(g))
    want = d.scores(torch.from_numpy(g), torch.from_numpy(p), lens)
    torch.cuda.synchronize()
    for k in ("sums", "counts", "a", "r", "f", "a_batch", "r_batch", "f_batch"):
        assert np.array_equal(bits(got[k].cpu().numpy()), bits(want[k].cpu().numpy())), k
    assert np.isfinite(float(got["a_batch"])) and float(got["f_batch"]) > 0
    with pytest.raises(ValueError, match="without mel_disc="):
        losses.ValidationLosses().adversarial(torch.from_numpy(p), torch.from_numpy(g))


def test_device_lengths_mark_a_bad_length():
    d = disc(ms.RUNS[0])
    g, p, lens = ms.batch(ms.CASE_BY_NAME["w64_edge"], pad=0)
    g, p = np.nan_to_num(g), np.nan_to_num(p)
    bad = torch.tensor([int(lens[0]), 66, int(lens[2])], dtype=torch.int32, device="cuda")
    out = d.scores(torch.from_numpy(g), torch.from_numpy(p), bad)
    good = d.scores(torch.from_numpy(g), torch.from_numpy(p), lens)
    torch.cuda.synchronize()
    assert out["status"].tolist() == [0, abi.MELDISC_BAD_LEN, 0] * 2
    assert out["counts"][1].tolist() == [0, 0, 0] and np.all(out["sums"][1].cpu().numpy() == 0)
    assert np.array_equal(bits(out["sums"][2].cpu().numpy()), bits(good["sums"][2].cpu().numpy()))


def test_finalize_names_what_is_wrong_and_state_before_it():
    w = M.fold_state_dict(state(ms.RUNS[0]))
    stream = torch.cuda.current_stream().cuda_stream
    mel = torch.zeros(1, 64, 80, device="cuda")
    sums, counts, status = torch.zeros(1, 3, 2, dtype=torch.float64, device="cuda"), torch.zeros(1, 3, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = dict(mel=mel.data_ptr(), T_ld=64, n_win=3, clips_ld=1, sums=sums.data_ptr(), counts=counts.data_ptr(), status=status.data_ptr(), hop=(16, 32, 64))

    def refused(weights, match):
        ctx = abi.Context()
        ctx.load_state_dict("meldisc", weights)
        with pytest.raises(abi.DttsError, match=match):
            ctx.finalize(abi.PART_MELDISC)
        with pytest.raises(abi.DttsError, match=r"\(-1\).*before dtts_finalize_weights\(DTTS_PART_MELDISC\)"):     # DTTS_E_STATE
            ctx.meldisc(1, stream, **call)
        ctx.close()

    refused({k: v for k, v in w.items() if k != "1.norm.2.bias"}, r"\(-2\).*missing tensor meldisc\.1\.norm\.2\.bias")
    refused({k: v for k, v in w.items() if k != "2.adv.weight"}, r"\(-2\).*missing tensor meldisc\.2\.adv\.weight")
    refused(M.fold_state_dict(synth.mel_disc_state_dict(1, "in", 48, 1)), r"\(-22\).*mel_disc_hidden_size = 48")
    refused(M.fold_state_dict(synth.mel_disc_state_dict(1, "in", 288, 1)), r"\(-22\).*mel_disc_hidden_size = 288")
    refused({**w, "3.conv.0.weight": w["0.conv.0.weight"]}, r"\(-22\).*4 windows")
    refused({**w, "1.adv.weight": np.zeros((1, 128 * 4 * 10), np.float32)}, r"\(-22\).*meldisc\.1\.adv\.weight is \[1, 5120\].*64-frame window's head has 10240 inputs")
    refused({**w, "1.adv.weight": np.zeros((1, 1280), np.float32)}, r"\(-22\).*meldisc\.1\.adv\.weight is \[1, 1280\]: a head per time row")
    refused({**w, "0.conv.2.weight": np.zeros((128, 64, 3, 3), np.float32)}, r"\(-22\).*meldisc\.0\.conv\.2\.weight is \[128, 64, 3, 3\].*\[128, 128, 3, 3\]")
    # a model of fewer windows or another head than the block asks for
    ctx = abi.Context()
    ctx.load_state_dict("meldisc", w)
    ctx.finalize(abi.PART_MELDISC)
    with pytest.raises(abi.DttsError, match=r"n_win = 2, the loaded discriminator has 3 windows"):
        ctx.meldisc(1, stream, **{**call, "n_win": 2})
    with pytest.raises(abi.DttsError, match=r"reduction = 2, the loaded adv_layer is over the whole map"):
        ctx.meldisc(1, stream, **call, reduction=abi.MELDISC_NONE)
    ctx.close()
