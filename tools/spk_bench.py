#!/usr/bin/env python3
"""B = 60 text->mel ENCODE time with speakers armed and not armed (dtts_text2mel_speakers + the speaker epilogue of last_ln).

Per variant: the device span of the 'encoder' stage timer (DTTS_TIMER_STAGE_ENCODER, one event pair per encode, T_mel sync wait
included) and the host wall time of (arm +) encode, medians over --steps after --warmup.  Variants: a handle without speaker weights,
the same weights plus spk_embed_proj loaded but nothing armed, and armed with each form.  Resident dictionary + ids, as bench.py runs.
  python tools/spk_bench.py [--steps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dict_tts_amd import abi, model, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=60)
    a = ap.parse_args()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    B = a.batch
    table = synth.dict_table(1234)
    ib = synth.make_id_batch(synth.biaobei_struct()["sentences"][:B], table)
    wt, ids, pm = (T(ib[k]).cuda() for k in ("word_tokens", "entry_ids", "pron_modified"))
    wt, pm, ids = wt.long().contiguous(), pm.long().contiguous(), ids.int().contiguous()
    spk_in = {"embed": T(synth.speaker_inputs(1234, "embed", B)).cuda(), "id": T(synth.speaker_inputs(1234, "id", B, 8)).cuda()}
    s = torch.cuda.current_stream().cuda_stream
    res = {"B": B, "T_w": int(wt.shape[1]), "steps": a.steps}

    def variant(name, hp, speaker, arm):
        m = model.PortaSpeech_dict(hparams=hp)
        m.load_state_dict({k: T(v) for k, v in synth.dict_tts_state_dict(1234, speaker=speaker, num_spk=8).items()}, strict=False)
        m.upload_dict_table(table)
        ctx = m.ctx
        ctx.timer_enable(abi.TIMER_STAGE_ENCODER)
        walls, devs = [], []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            ctx.timer_reset()
            t0 = time.perf_counter()
            if arm:
                ctx.text2mel_speakers(abi.SPK_ID if speaker == "id" else abi.SPK_EMBED, spk_in[speaker].data_ptr(), B, s)
            T_mel = ctx.text2mel_encode_ids(wt.data_ptr(), ids.data_ptr(), pm.data_ptr(), None, B, int(wt.shape[1]), ib["L_k"], ib["P"], s)
            wall = time.perf_counter() - t0
            ms, n = ctx.timer_read(abi.TIMER_STAGE_ENCODER)
            if i >= a.warmup:
                walls.append(wall * 1e6)
                devs.append(ms * 1e3)
        res[name] = {"encode_device_us_median": float(np.median(devs)), "arm_plus_encode_wall_us_median": float(np.median(walls)),
                     "T_mel": int(T_mel)}
        del m

    variant("no_speaker_weights", {}, None, False)
    variant("embed_loaded_not_armed", {"use_spk_embed": True, "num_spk": 4}, "embed", False)
    variant("embed_armed", {"use_spk_embed": True, "num_spk": 4}, "embed", True)
    variant("id_armed", {"use_spk_id": True, "num_spk": 8}, "id", True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
