#!/usr/bin/env python3
"""Generate tests/golden/g17_meldisc.npz by running the REFERENCE's modules/fastspeech/multi_window_disc.py::Discriminator on the seeded
mels of tests/meldisc_shapes.py.  TEST INFRASTRUCTURE; needs the reference checkout (DICT_TTS_REFERENCE), runs in the build container
only, on the CPU.

Nothing of the reference is copied: this script imports it (oracle/make_golden.py's stub finder, cwd = reference root), loads
``synth.mel_disc_state_dict`` into its module with strict=True, and runs it in eval mode in float32 and — via ``.double()`` — in float64:
  * per run (norm, hidden, reduction, windows), case, utterance, signal and window: the D of every clip, each clip taken from the utterance
    alone at its own length (``<run>.<case>.<b>.<g|p>.<w>.f32 / .f64``);
  * ``e_ref.<run>`` [n_win]: the reference's own float32 error against its float64, max |D32 - D64| / max |D64| per (case, utterance,
    window), the maximum over the run's cases;  ``e_h.<run>`` [3]: the same for the three hidden maps of the 32-frame window;
  * ``h.<run>.<l>.f32 / .f64``: the hidden maps of ONE clip of the 32-frame window (meldisc_shapes.HIDDEN_*), every 16th channel;
  * ``<run>.<forward case>.y.f32 / .f64`` and ``.h<l>``: ``Discriminator.forward`` on zero-padded batches at given starts.
Data only; no weights are stored.
"""
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)
from oracle.make_golden import REF, OUT, _Finder  # noqa: E402


def main():
    sys.dont_write_bytecode = True
    sys.meta_path.insert(0, _Finder())
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REF)
    os.chdir(REF)
    import warnings
    warnings.filterwarnings("ignore")
    import numpy as np
    import torch
    torch.manual_seed(0)
    torch.set_num_threads(8)

    import meldisc_shapes as ms
    from dict_tts_amd import synth
    from modules.fastspeech.multi_window_disc import Discriminator

    out = {"seed": np.int64(ms.SEED)}
    with torch.no_grad():
        for run in ms.RUNS:
            norm, H, red, n_win, cases = run
            rid = ms.run_id(run)
            sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.mel_disc_state_dict(ms.SEED, norm, H, n_win, red).items()}

            def load():
                m = Discriminator(time_lengths=[32, 64, 128][:n_win], freq_length=80, hidden_size=H, norm_type=norm, reduction=red)
                m.load_state_dict(sd, strict=True)
                return m.eval()

            m32, m64 = load(), load().double()
            e_ref, e_h, dmax = np.zeros(n_win), np.zeros(3), np.zeros(n_win)
            for name in cases:
                case = ms.CASE_BY_NAME[name]
                for b in range(len(case["lens"])):
                    mels = ms.utterance(case, b)
                    for w in range(n_win):
                        win = ms.WINS[w]
                        starts = ms.starts_of(case, b, win)
                        d32, d64, h32, h64 = [], [], [], []
                        for sig, mel in zip("gp", mels):
                            a32, a64 = [], []
                            for s in starts:
                                clip = torch.from_numpy(mel[s:s + win])[None, None]
                                y32, hh32 = m32.discriminator.conv_layers[w](clip)
                                y64, hh64 = m64.discriminator.conv_layers[w](clip.double())
                                a32.append(y32.reshape(-1).numpy())
                                a64.append(y64.reshape(-1).numpy())
                                if w == 0:
                                    h32.append([t[0].numpy() for t in hh32])
                                    h64.append([t[0].numpy() for t in hh64])
                                    if (name, b, s, sig) == (ms.HIDDEN_CASE, ms.HIDDEN_B, ms.HIDDEN_START, "g") and f"h.{rid}.0.f64" not in out:
                                        for l in range(3):
                                            out[f"h.{rid}.{l}.f32"] = hh32[l][0].numpy()[ms.HIDDEN_CH].copy()
                                            out[f"h.{rid}.{l}.f64"] = hh64[l][0].numpy()[ms.HIDDEN_CH].copy()
                            k = f"{rid}.{name}.{b}.{sig}.{w}"
                            out[k + ".f32"] = np.stack(a32) if a32 else np.zeros((0, 1), np.float32)
                            out[k + ".f64"] = np.stack(a64) if a64 else np.zeros((0, 1))
                            d32 += a32
                            d64 += a64
                        if not d64:
                            continue
                        a, c = np.concatenate(d32).astype(np.float64), np.concatenate(d64)
                        e_ref[w] = max(e_ref[w], np.abs(a - c).max() / np.abs(c).max())
                        dmax[w] = max(dmax[w], np.abs(c).max())
                        if w == 0:
                            for l in range(3):
                                a = np.stack([x[l] for x in h32]).astype(np.float64)
                                c = np.stack([x[l] for x in h64])
                                if np.abs(c).max() > 0:
                                    e_h[l] = max(e_h[l], np.abs(a - c).max() / np.abs(c).max())
            out[f"e_ref.{rid}"], out[f"e_h.{rid}"], out[f"d_max.{rid}"] = e_ref, e_h, dmax
            print(rid, "e_ref", e_ref, "e_h", e_h, "max |D64|", dmax)
            assert np.all((dmax >= 1e-3) & (dmax <= 1e3)), f"the synthetic scale is wrong: max |D64| = {dmax}"
            # Discriminator.forward on zero-padded batches at given starts (the full-width `in` runs and the other norms)
            if H == 128 and n_win == 3:
                for fw in ms.FORWARD:
                    x = torch.from_numpy(ms.batch(ms.CASE_BY_NAME[fw["case"]], pad=0, fill=0.0)[0])
                    B = x.shape[0]
                    for prec, m, xx in (("f32", m32, x), ("f64", m64, x.double())):
                        ret = m(xx, start_frames_wins=[[s] * B for s in fw["starts"]])
                        k = f"{rid}.{fw['name']}"
                        out[f"{k}.y_none"] = np.int64(ret["y"] is None)
                        if ret["y"] is not None:
                            out[f"{k}.y.{prec}"] = ret["y"].numpy()
                        out[f"{k}.n_h"] = np.int64(len(ret["h"]))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g17_meldisc.npz")
    np.savez_compressed(path, **out)
    print("g17_meldisc.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
