#!/usr/bin/env python3
"""Timings of the PortaSpeech baseline (dict_tts_amd.model.PortaSpeech) on one MI355X: encode (dtts_text2mel_fetch(DTTS_PS_ENCODE)) and
encode + decode, for one sentence of 364 frames and for the 60 Biaobei sentences of synth.biaobei_batch (1 .. 3 phonemes per word, 22
frames per word teacher-forced, so that no call synchronises: T_mel 596, about 17 000 live frames), beside the
Dict-TTS text-to-mel of the in-tree library (resident table + ids) on the same batch sizes in the same run, and beside the same weights
through the same arithmetic in torch float32 on the same device (the restatement tests/portaspeech_ref.py with the device as torch's
default; it synchronises a few times per call where it derives lengths from values, which is part of what it costs).  Warm-up, then the
median of --reps timings between two events, each over --inner back-to-back calls.  Seeded weights; one line per figure and a JSON line.

    python tools/portaspeech_bench.py [--reps 15] [--inner 5] [--out profiles/ps_bench.txt]
    bash tools/prof_cmd.sh ps60 --detail "ps_|conv1d|vconv|mha|layernorm|flow" -- python tools/portaspeech_bench.py --profile
        (the per-kernel split of three encode + decode calls at 60 utterances, as the table prof_cmd.sh writes: profiles/ps60_kernel_trace.md)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dict_tts_amd import abi, synth  # noqa: E402
from dict_tts_amd import model as M  # noqa: E402

T = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def median_ms(fn, reps, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


class _Dict:
    def __len__(self):
        return synth.PS_N_PHONE


def ps_case(words, frames_per_word=22):
    b = synth.portaspeech_batch(words)
    m2w = synth.ps_spread_mel2word(words, [frames_per_word * len(w) for w in words])
    return b, m2w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile", action="store_true", help="three encode + decode calls of the baseline at 60 utterances and nothing else (for a kernel trace)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch float32 comparison")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    ps = M.PortaSpeech(_Dict(), hparams={})
    ps.load_state_dict({k: T(v) for k, v in synth.portaspeech_state_dict().items()})
    dt = M.PortaSpeech_dict(hparams={})
    dt.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict().items()})
    table = synth.dict_table(1234)
    dt.upload_dict_table(table)
    sents = synth.biaobei_struct()["sentences"]
    words60 = synth.portaspeech_words(0, 60)
    one = [w for w in words60 if 22 * len(w) <= 364][:1] or words60[:1]
    one = [one[0][:364 // 22] + [2] * max(0, 364 // 22 - len(one[0]))]           # 16 words: 352 frames, padded to 364 below
    res, lines = {}, []
    for tag, words, sent in (("1x364", one, None), ("60utt", words60, sents[:60])):
        b, m2w = ps_case(words)
        if tag == "1x364":
            m2w = np.concatenate([m2w, np.full((1, 364 - m2w.shape[1]), m2w[0, -1], np.int64)], 1)
        txt, p2w, m2w_d = T(b["txt_tokens"]).to(dev), T(b["ph2word"]).to(dev), T(m2w).to(dev)
        B, T_ph, T_w = txt.shape[0], txt.shape[1], b["T_w"]
        status = torch.zeros(4, dtype=torch.int64, device=dev)
        enc = lambda: ps.ctx.ps_encode(B, T_ph, T_w, txt.data_ptr(), p2w.data_ptr(), status.data_ptr(), stream, mel2word=(m2w_d.data_ptr(), m2w_d.shape[1]),
                                       want_attn=False)
        T_mel = enc()
        assert status.cpu().tolist() == [0, 0, 0, 0]
        z = torch.randn(B, 16, T_mel // 4, device=dev)
        mel = torch.empty(B, T_mel, 80, device=dev)

        def both():
            enc()
            ps.ctx.text2mel_decode(z.data_ptr(), mel.data_ptr(), stream)
        frames = int((m2w > 0).sum())
        if args.profile:
            if tag == "60utt":
                for _ in range(3):
                    both()
                torch.cuda.synchronize()
            continue
        res[tag] = {"B": B, "T_ph": T_ph, "T_w": T_w, "T_mel": T_mel, "live_frames": frames}
        for what, fn in (("ps_encode", enc), ("ps_encode_decode", both)):
            med, lo, hi = median_ms(fn, args.reps, args.inner)
            res[tag][what + "_ms"] = med
            lines.append(f"{tag:7s} {what:18s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {frames / med * 1e3:12.0f} live frames/s")
        if not args.no_torch:   # the same weights, the same arithmetic, torch float32 on this device
            try:
                import portaspeech_ref as pr
                torch.set_default_device(dev)
                sd = {k: v.to(dev) for k, v in pr.state(synth.portaspeech_state_dict(), torch.float32).items()}
                table_pos = pr._fft.sinusoid_table(pr._fft.DEFAULT_MAX_TARGET_POSITIONS, 192, 0)
                t_enc = lambda: pr.forward(sd, {}, txt, p2w, T_w, m2w_d, decode=False, pos_table=table_pos)
                t_both = lambda: pr.forward(sd, {}, txt, p2w, T_w, m2w_d, z_p=z, pos_table=table_pos)
                err = float((t_both()["mel_out"] - mel).abs().max())
                for what, fn in (("torch_encode", t_enc), ("torch_encode_decode", t_both)):
                    med, lo, hi = median_ms(fn, max(3, args.reps // 3), 1, warmup=2)
                    res[tag][what + "_ms"] = med
                    lines.append(f"{tag:7s} {what:18s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {frames / med * 1e3:12.0f} live frames/s")
                lines.append(f"{tag:7s} max |mel(library) - mel(torch float32)| = {err:.3e}")
            except Exception as e:   # the comparison is a measurement aid: say what happened and go on with the library's own figures
                lines.append(f"{tag:7s} torch float32 comparison failed: {type(e).__name__}: {e}")
            finally:
                torch.set_default_device("cpu")
        # Dict-TTS text-to-mel on the same number of utterances (its own sentences of that count: words, not phonemes), teacher-forced alike
        s = sent if sent is not None else [sents[0][:14]]
        ib = synth.make_id_batch(s, table)
        wt, ids, pm = T(ib["word_tokens"]).to(dev), T(ib["entry_ids"]).to(dev).to(torch.int32), T(ib["pron_modified"]).to(dev)
        dm2w = T(synth.teacher_mel2word(ib["word_tokens"])).to(dev)
        Bd, Twd = wt.shape

        def dict_enc():
            return dt.ctx.text2mel_encode_ids(wt.data_ptr(), ids.data_ptr(), pm.data_ptr(), (dm2w.data_ptr(), dm2w.shape[1]), Bd, Twd, int(ib["L_k"]), int(ib["P"]), stream)
        Td = dict_enc()
        zd = torch.randn(Bd, 16, Td // 4, device=dev)
        meld = torch.empty(Bd, Td, 80, device=dev)

        def dict_both():
            dict_enc()
            dt.ctx.text2mel_decode(zd.data_ptr(), meld.data_ptr(), stream)
        fd = int((dm2w > 0).sum())
        res[tag].update(dict_T_mel=Td, dict_live_frames=fd)
        for what, fn in (("dict_encode", dict_enc), ("dict_encode_decode", dict_both)):
            med, lo, hi = median_ms(fn, args.reps, args.inner)
            res[tag][what + "_ms"] = med
            lines.append(f"{tag:7s} {what:18s} {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {fd / med * 1e3:12.0f} live frames/s")
    if args.profile:
        return
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
