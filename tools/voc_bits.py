#!/usr/bin/env python3
"""Bit-identity record of the vocoder's fused kernels across two builds of the library (a refactor's check: nothing may move).

    tools/voc_bits.py --lib PATH --out FILE      synthetic-checkpoint forwards on the build at PATH: the SHA-256 of every waveform, the always-on
                                                 detector's count (dtts_vocoder_nonfinite) and the range-guard census' count, as JSON
    tools/voc_bits.py --compare A.json B.json    case by case; exit status 1 when a hash or a count differs or a case is missing

The vocoder has no entry point that fetches a stage's tensors: the waveform (every sample depends on every kernel before it), the whole output
buffer (a stray store shows) and the two counters are what a build can be held to.

Cases: the generators `default` (ResBlock1, V1), `v2` (narrow stages: rbn) and `v3` (ResBlock2: rb2x); f16, f16 under the range guard (the census
instantiations) and bf16; on the default generator the schedule / arithmetic switches 9 (the whole stage in one launch, private strips), 14 and 15.
Shapes: B = 1 with 5 and 37 frames (half-size tiles, tiles shorter than the halo), a ragged B = 3 (masked tile edges), and the benchmark's ragged
B = 60, T <= 740 — the smallest batch in which the persistent workgroups of every family walk more than one tile and claim dynamically.  `hot`:
utterance 1 of the ragged batch scaled by 3e6, so that fp16 operands overflow: the poisoned samples and the detector's count are compared too."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    for case in sorted(set(a) | set(b)):
        ra, rb = a.get(case), b.get(case)
        same = ra is not None and ra == rb
        bad += not same
        show = ra or rb
        what = show.get("error") or f"wav {show['wav'][:16]} buf {show['buf'][:16]} nonfinite {show['nonfinite']} nan {show['nan_samples']} clamped {show['clamped']}"
        print(f"{'equal' if same else 'DIFFERENT':9s} {case:44s} {what}")
        if not same:
            print(f"          A: {ra}\n          B: {rb}")
    print(f"{len(set(a) | set(b))} cases, {bad} different: A = {os.path.basename(a_path)}, B = {os.path.basename(b_path)}")
    return 1 if bad else 0


def shapes(rng, np):
    """name -> (mel [B, T, 80] float32, lens [B] int32), the mels in the log10-mel range of the benchmark"""
    mel_of = lambda B, T: np.clip(rng.normal(-3, 1.2, (B, T, 80)), -6, 1.5).astype(np.float32)
    out = {"b1_t5": (mel_of(1, 5), np.array([5], np.int32)), "b1_t37": (mel_of(1, 37), np.array([37], np.int32)),
           "b3_ragged": (mel_of(3, 40), np.array([40, 23, 7], np.int32))}
    lens = np.clip(rng.normal(364, 110, 60), 120, 740).astype(np.int32)   # (tools/voc_bench.py's batch)
    lens[0] = 740
    out["b60_bench"] = (mel_of(60, 740), lens)
    hot = out["b3_ragged"][0].copy()
    hot[1] *= 3e6
    out["b3_hot"] = (hot, out["b3_ragged"][1])
    return out


def record(lib, out_path):
    import numpy as np
    import torch
    from dict_tts_amd import abi, synth, vocoder
    abi.load_library(os.path.abspath(lib))
    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    cfgs = {"default": synth.hifigan_config(), "v2": synth.hifigan_config_v2(), "v3": synth.hifigan_config_v3()}
    shp = {k: (T_(m).cuda(), T_(l).cuda(), l) for k, (m, l) in shapes(np.random.default_rng(0), np).items()}
    plain = ["b1_t5", "b1_t37", "b3_ragged", "b60_bench"]
    models = [(c, prec, guard, 0, plain + (["b3_hot"] if prec == "f16" and not guard else []))
              for c in cfgs for prec, guard in (("f16", False), ("f16", True), ("bf16", False))]
    models += [("default", "f16", False, 1 << 9, plain + ["b3_hot"]), ("default", "f16", False, 1 << 14, plain), ("default", "f16", False, 1 << 15, plain),
               ("default", "f16", True, 1 << 9, ["b3_ragged", "b60_bench"]), ("default", "bf16", False, 1 << 9, plain), ("default", "bf16", False, 1 << 14, plain)]
    res = {}
    stream = torch.cuda.current_stream().cuda_stream
    for c, prec, guard, tune, names in models:
        tag = f"{c}/{prec}{'+guard' if guard else ''}/tune{tune}"
        try:
            sd = {k: T_(v) for k, v in synth.hifigan_state_dict(1234, cfg=cfgs[c]).items()}
            voc = vocoder.HifiGAN(state_dict=sd, config={**cfgs[c], "dtts_tune_flags": tune}, precision=prec, range_guard=guard)
        except abi.DttsError as e:   # (a switch the build refuses for this generator: both builds must refuse it alike)
            res[tag] = {"error": str(e)}
            continue
        for name in names:
            mel, lens_d, lens = shp[name]
            B, T, _ = mel.shape
            wav = torch.zeros(B, T * voc.hop, dtype=torch.float32, device="cuda")
            # (the context's own entry point: HifiGAN.forward_batch raises on a census count instead of returning it.  A failed forward ends the
            # run: nothing more is started on a device that may have faulted)
            seen = int(voc.ctx.vocoder_nonfinite())   # (the counter is cumulative per context: a case records its own delta)
            voc.ctx.hifigan_forward(mel.data_ptr(), lens_d.data_ptr(), B, T, wav.data_ptr(), stream)
            clamped = voc.ctx.vocoder_clamped(stream) if guard else 0
            torch.cuda.synchronize()
            w = wav.cpu().numpy()
            valid = hashlib.sha256()
            for b in range(B):
                valid.update(w[b, :int(lens[b]) * voc.hop].tobytes())
            res[f"{tag}/{name}"] = {"wav": valid.hexdigest(), "buf": hashlib.sha256(w.tobytes()).hexdigest(),
                                    "nonfinite": int(voc.ctx.vocoder_nonfinite()) - seen, "nan_samples": int(np.isnan(w).sum()), "clamped": int(clamped)}
            print(f"{tag}/{name}: {res[f'{tag}/{name}']['wav'][:16]} nonfinite {res[f'{tag}/{name}']['nonfinite']} clamped {clamped}", flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"{len(res)} cases -> {out_path}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="path of the library build to record")
    ap.add_argument("--out", help="JSON file the record goes to")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not (a.lib and a.out):
        ap.error("--lib PATH --out FILE, or --compare A.json B.json")
    record(a.lib, a.out)
