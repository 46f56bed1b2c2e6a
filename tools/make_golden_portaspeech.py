#!/usr/bin/env python3
"""Generate tests/golden/g19_portaspeech.npz by running the REFERENCE's PortaSpeech baseline (modules/portaspeech/model.py::PortaSpeech).
TEST INFRASTRUCTURE; needs the reference checkout (DICT_TTS_REFERENCE), runs in the build container only.

Recipe of oracle/make_golden.py (its stub finder, cwd = reference root, strict load_state_dict, remove_weight_norm, fixed prior noise) with
set_hparams(egs/datasets/audio/biaobei/ps_adv.yaml): task_cls tasks.tts.ps_adv.PortaSpeechAdvTask, dur_level word, use_post_glow false.
The ragged batch and the weights are those of tests/portaspeech_shapes.py ("golden": B = 3, 23 / 17 / 1 phonemes) and
dict_tts_amd/synth.portaspeech_state_dict.  Stored: the inputs, mel2word as add_dur returns it (padded as run_text_encoder pads it), the
returned tensors, the prior noise; and a second run with a teacher-forced mel2word whose length (37) is no multiple of 4 ("tf." keys).
Asserts the duration condition the tests rely on: every exp(dur) - 1 the length regulator reads lies >= 1e-3 from a half-integer.
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

    import portaspeech_ref as pr
    import portaspeech_shapes as ps
    from utils.hparams import set_hparams
    from utils.text_encoder import TokenTextEncoder

    hp = set_hparams(config="egs/datasets/audio/biaobei/ps_adv.yaml", exp_name="", hparams_str="", print_hparams=False)
    assert hp["task_cls"] == "tasks.tts.ps_adv.PortaSpeechAdvTask" and hp["dur_level"] == "word" and not hp["use_post_glow"]
    from modules.portaspeech.model import PortaSpeech
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    vocab = [f"p{i}" for i in range(ps.N_PHONE - 3)]   # 3 reserved symbols + these = N_PHONE rows of the embedding
    model = PortaSpeech(TokenTextEncoder(None, vocab_list=vocab, replace_oov=","))
    sd = {k: T(v) for k, v in ps.sd_np().items()}
    print("load_state_dict(strict=True):", model.load_state_dict(sd, strict=True))
    model.eval()

    def remove_weight_norm(m):  # tasks/tts/ps_flow.py:262-268
        try:
            torch.nn.utils.remove_weight_norm(m)
        except ValueError:
            return
    model.apply(remove_weight_norm)
    out = {}
    for name, pre in (("golden", ""), ("golden_tf", "tf.")):
        i = ps.inputs(name)

        class Prior:
            def sample(self, shape, name=name):
                return T(ps.noise(name, shape[0], shape[2]))
        model.fvae.prior_dist = Prior()
        seen = {}
        add_dur = PortaSpeech.add_dur.__get__(model)

        def capture(*a, **k):   # mel2word is not a return key of the reference: take add_dur's result
            seen["m2w"] = add_dur(*a, **k)
            return seen["m2w"]
        model.add_dur = capture
        txt, ph2word = T(i["txt_tokens"]), T(i["ph2word"])
        word_len = ph2word.max(1)[0]
        with torch.no_grad():
            r = model(txt, ph2word, word_len.max(), mel2word=None if i["mel2word"] is None else T(i["mel2word"]), infer=True,
                      forward_post_glow=False, two_stage=True)
        m2w = seen["m2w"]
        if m2w.shape[1] % hp["frames_multiple"]:
            m2w = torch.cat([m2w] + [m2w[:, -1:]] * (hp["frames_multiple"] - m2w.shape[1] % hp["frames_multiple"]), -1)
        out[pre + "mel2word"] = m2w.numpy()
        for k in ("ph_encoder_out", "dur", "attn", "word_encoder_out", "x_mask", "decoder_inp", "mel_out"):
            out[pre + k] = r[k].numpy()
        out[pre + "z_p"] = ps.noise(name, txt.shape[0], r["mel_out"].shape[1] // 4)
        if i["mel2word"] is None:
            out["txt_tokens"], out["ph2word"], out["word_len"] = i["txt_tokens"], i["ph2word"], word_len.numpy()
            gap = pr.min_half_distance(r["dur"].numpy(), ps.live_words(name))
            print("min |exp(dur) - 1 - half-integer| =", gap)
            assert gap >= 1e-3, gap
        else:
            out[pre + "mel2word_in"] = i["mel2word"]
        print(name, "mel", tuple(r["mel_out"].shape), "frames", (m2w > 0).sum(1).tolist())
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "g19_portaspeech.npz")
    np.savez_compressed(path, **out)
    print("g19_portaspeech.npz", os.path.getsize(path))
    assert os.path.getsize(path) < 700 * 1024


if __name__ == "__main__":
    main()
