#!/usr/bin/env python3
"""Generate tests/golden/g11_speaker.npz by running the REFERENCE implementation with speaker conditioning, both forms.
TEST INFRASTRUCTURE; needs the reference checkout (DICT_TTS_REFERENCE), runs in the build container only.

Recipe of oracle/make_golden.py (its stub finder, cwd = reference root, strict load_state_dict, remove_weight_norm, fixed prior noise):
  - "embed": set_hparams(egs/datasets/audio/wenetspeech/dict_tts.yaml, use_word_input=True,word_size=8000,use_dict=True,num_spk=4)
             -> use_spk_embed, spk_embed_proj = nn.Linear(256, 192)
  - "id":    set_hparams(egs/datasets/audio/biaobei/dict_tts.yaml, ...,use_spk_id=True,num_spk=8) -> Embedding(8, 192)
A ragged batch of five utterances with mixed speakers (tests/speaker_ref.py), synthetic weights of dict_tts_amd/synth.py plus
spk_embed_proj.  Only what the reference returns is stored (and the inputs that are cheap to store).
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

    import speaker_ref as sr
    from utils.hparams import set_hparams
    from utils.text_encoder import TokenTextEncoder

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    b = {k: T(v) for k, v in sr.g11_batch().items()}
    B = b["word_tokens"].shape[0]
    out["word_tokens"] = b["word_tokens"].numpy()
    for form, f in sr.FORMS.items():
        hp = set_hparams(config=f["config"], exp_name="", hparams_str=f["hparams_str"], print_hparams=False)
        assert hp["num_spk"] == f["num_spk"] and bool(hp["use_spk_id"]) == (form == "id"), (hp["num_spk"], hp["use_spk_id"])
        assert bool(hp["use_spk_embed"]) == (form == "embed") or form == "id"
        import modules.dict_tts.model as dm
        model = dm.PortaSpeech_dict(TokenTextEncoder(None, vocab_list=["a", "b", "c"], replace_oov=","))
        print(form, "spk_embed_proj:", model.spk_embed_proj)
        sd = {k: T(v) for k, v in sr.g11_state_dict(form).items()}
        print(form, "load_state_dict(strict=True):", model.load_state_dict(sd, strict=True))
        model.eval()

        def remove_weight_norm(m):  # tasks/tts/ps_flow.py:262-268
            try:
                torch.nn.utils.remove_weight_norm(m)
            except ValueError:
                return
        model.apply(remove_weight_norm)

        class LazyPrior:
            def sample(self, shape, form=form):
                return T(sr.g11_noise(form, shape[0], shape[2]))
        model.fvae.prior_dist = LazyPrior()
        spk = T(sr.g11_speakers(form))
        seen = {}
        add_dur = model.add_dur

        def capture(*a, **k):   # mel2word is not a return key of the reference: take add_dur's result
            seen["m2w"] = add_dur(*a, **k)
            return seen["m2w"]
        model.add_dur = capture
        with torch.no_grad():
            r = model((b["word_tokens"], b["word_tokens"]), b["pron_modified"], (None, None, None), ph2word=None, word_len=None,
                      dict_msg=(b["keys"], b["values"], b["key_map"], b["pinyin"], b["pinyin_map"]), infer=True,
                      forward_post_glow=False, spk_embed=spk, two_stage=True, mel2word=None)
        m2w = seen["m2w"]
        if m2w.shape[1] % hp["frames_multiple"]:   # the padding of modules/dict_tts/model.py:98-100
            m2w = torch.cat([m2w] + [m2w[:, -1:]] * (hp["frames_multiple"] - m2w.shape[1] % hp["frames_multiple"]), -1)
        out[form + ".mel2word"] = m2w.numpy()
        out[form + ".spk"] = spk.numpy()
        for k in ("word_encoder_out", "dur", "x_mask", "mel_out"):
            out[f"{form}.{k}"] = r[k].numpy()
        out[form + ".z_p"] = sr.g11_noise(form, B, r["mel_out"].shape[1] // 4)
        print(form, "mel", tuple(r["mel_out"].shape), "frames", (m2w > 0).sum(1).tolist(),
              "durations", torch.clamp(torch.round(r["dur"].exp() - 1), min=0).long().tolist())
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "g11_speaker.npz"), **out)
    print("g11_speaker.npz", os.path.getsize(os.path.join(OUT, "g11_speaker.npz")))


if __name__ == "__main__":
    main()
