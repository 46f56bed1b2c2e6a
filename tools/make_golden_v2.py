#!/usr/bin/env python3
"""Generate tests/golden/g14_hifigan_v2.npz by running the REFERENCE HifiGanGenerator in the small V2 configuration (ResBlock1,
upsample_initial_channel 128: dict_tts_amd.synth.hifigan_config_v2).  TEST INFRASTRUCTURE; needs the reference checkout (DICT_TTS_REFERENCE).

Recipe of oracle/make_golden.py's vocoder section (its stub finder, strict load_state_dict, remove_weight_norm) on
tests/golden_cases.g6_mel(): the waveform, per-stage heads and RMS, a few folded-weight heads — g6's shape — plus the sorted list of the
reference generator's state-dict names.  Data only.
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

    import golden_cases as gc
    from dict_tts_amd import synth
    from modules.hifigan.hifigan import HifiGanGenerator

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cfg = dict(synth.hifigan_config_v2(), audio_num_mel_bins=80, use_pitch_embed=False)
    gen = HifiGanGenerator(cfg)
    names = sorted(gen.state_dict().keys())
    hsd = {k: T(v) for k, v in synth.hifigan_state_dict(gc.SEED, cfg=synth.hifigan_config_v2()).items()}
    print("hifigan (V2) load_state_dict(strict=True):", gen.load_state_dict(hsd, strict=True))
    gen.remove_weight_norm()
    gen.eval()
    nup = len(cfg["upsample_rates"])
    with torch.no_grad():
        mel = gc.g6_mel()
        c = torch.FloatTensor(mel).unsqueeze(0).transpose(2, 1)  # vocoders/hifigan.py:57-58
        stages, hooks = {}, []
        for i in range(nup):
            hooks.append(gen.ups[i].register_forward_hook(lambda m, a, o, i=i: stages.__setitem__(f"ups.{i}", o)))
        # (the generator accumulates `xs += resblock(x)` IN PLACE into the first ResBlock's output: the hooks keep copies)
        hooks.append(gen.conv_post.register_forward_hook(lambda m, a, o: stages.__setitem__("post", o)))
        for j in range(len(gen.resblocks)):
            hooks.append(gen.resblocks[j].register_forward_hook(lambda m, a, o, j=j: stages.__setitem__(f"rb.{j}", o.clone())))
        wav = gen(c).view(-1)
        for h in hooks:
            h.remove()
        save = {"wav": wav.numpy(), "folded.conv_pre.weight.head": gen.conv_pre.weight[:8].numpy(),
                "folded.ups.0.weight.head": gen.ups[0].weight[:8].numpy(),
                "folded.resblocks.0.convs1.0.weight.head": gen.resblocks[0].convs1[0].weight[:8].numpy(),
                "folded.resblocks.11.convs2.2.weight.head": gen.resblocks[11].convs2[2].weight[:8].numpy(),
                "state_dict_names": np.array(names)}
        for k, v in stages.items():
            save[k + ".head"] = v[0, :, :64].numpy()
            save[k + ".rms"] = np.array(float(v.pow(2).mean().sqrt()))
        path = os.path.join(OUT, "g14_hifigan_v2.npz")
        np.savez_compressed(path, **save)
        print("G14 wav", wav.shape, "rms", float(wav.pow(2).mean().sqrt()), "absmax", float(wav.abs().max()),
              "frac>0.9", float((wav.abs() > 0.9).float().mean()), {k: float(v.pow(2).mean().sqrt()) for k, v in stages.items()})
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
