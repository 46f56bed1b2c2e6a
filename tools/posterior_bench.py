#!/usr/bin/env python3
"""B = 60 teacher-forced posterior pass (dtts_text2mel_fetch(DTTS_OUT_POSTERIOR)) against the infer encode + decode of the same batch, same process.

The batch: the first B Biaobei sentences, tensor API, teacher-forced mel2word (tests/posterior_ref.py's tgt_mels), explicit eps / z_p.
Per step: one encode, then either the decode (infer) or the posterior pass, each timed as a host wall span closed by a stream
synchronisation; medians over --steps after --warmup.  The ratio (encode + posterior) / (encode + decode) is what the posterior pass costs
relative to inference.  Under `rocprofv3 --kernel-trace --stats -- python tools/posterior_bench.py` the per-kernel times come with it.
  python tools/posterior_bench.py [--steps 20] [--warmup 5] [--batch 60]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import posterior_ref as pr  # noqa: E402
from dict_tts_amd import model, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=60)
    a = ap.parse_args()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    B = a.batch
    batch = synth.biaobei_batch(0, B, 1234)
    m2w_np = synth.teacher_mel2word(batch["word_tokens"])
    mels_np = pr.tgt_mels_for(m2w_np, name="bench.mel")
    T_mel = mels_np.shape[1]
    b = {k: T(v).contiguous() for k, v in batch.items()}
    m2w, mels = T(m2w_np).long().contiguous(), T(mels_np).float().contiguous()
    eps = T(synth.randn(1234, "bench.eps", (B, 16, T_mel // 4))).float().contiguous()
    z = T(synth.noise(1234, B, T_mel // 4, "bench.z")).float().contiguous()
    m = model.PortaSpeech_dict(hparams={})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dict_tts_state_dict(1234).items()}, strict=True)
    ctx = m.ctx
    s = torch.cuda.current_stream().cuda_stream
    B_, T_w = b["word_tokens"].shape
    L_k, P = b["keys"].shape[2], b["pinyin"].shape[2]
    mel = torch.empty(B, T_mel, 80, device="cuda")
    mq, lq, zp = (torch.empty(B, 16, T_mel // 4, device="cuda") for _ in range(3))
    kl = torch.empty((), device="cuda")

    def encode():
        return ctx.text2mel_encode(*(b[k].data_ptr() for k in ("word_tokens", "keys", "values", "key_map", "pinyin", "pinyin_map",
                                                               "pron_modified")), (m2w.data_ptr(), m2w.shape[1]), B, T_w, L_k, P, s)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    res = {"B": B, "T_w": int(T_w), "T_mel": int(T_mel), "steps": a.steps}
    enc, dec, post = [], [], []
    for i in range(a.warmup + a.steps):
        e1 = timed(encode)
        d = timed(lambda: ctx.text2mel_decode(z.data_ptr(), mel.data_ptr(), s))
        e2 = timed(encode)
        p = timed(lambda: ctx.text2mel_posterior(mels.data_ptr(), T_mel, eps.data_ptr(), T_mel // 4, mel.data_ptr(), T_mel, mq.data_ptr(),
                                                 lq.data_ptr(), zp.data_ptr(), kl.data_ptr(), s))
        if i >= a.warmup:
            enc += [e1, e2]
            dec.append(d)
            post.append(p)
    med = lambda v: float(np.median(v))
    res.update(encode_us_median=med(enc), decode_us_median=med(dec), posterior_us_median=med(post))
    res["infer_encode_plus_decode_us"] = res["encode_us_median"] + res["decode_us_median"]
    res["encode_plus_posterior_us"] = res["encode_us_median"] + res["posterior_us_median"]
    res["ratio_posterior_to_infer"] = res["encode_plus_posterior_us"] / res["infer_encode_plus_decode_us"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
