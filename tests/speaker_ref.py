"""CPU fp32 restatement of the SPEAKER-conditioned ``PortaSpeech_dict.forward(infer=True)`` and the G11 cases (test infrastructure).

Composed from the oracle's pieces (oracle/dict_tts_ref.py: dict_encoder, add_dur, expand, fvae_infer) plus the two lines the reference
adds for a multi-speaker checkpoint:
  - spk_embed = spk_embed_proj(spk_embed)[:, None, :]              modules/dict_tts/model.py:44-45
      spk_embed_proj = Embedding(num_spk, hidden) with use_spk_id,
                       nn.Linear(256, hidden, bias=True) with use_spk_embed   modules/portaspeech/model.py:159-163
  - word_encoder_out = word_encoder_out + spk_embed (every row)      modules/dict_tts/model.py:94
  - dur_input = word_encoder_out * nonpadding                        modules/dict_tts/model.py:96
  - the decoder condition is gathered from that sum                  modules/dict_tts/model.py:102-107
The inputs are sample['spk_ids'] with use_spk_id, sample['spk_embed'] otherwise (tasks/tts/dict_tts.py:182).

G11 (tests/golden/g11_speaker.npz, written by tools/make_golden_spk.py from the reference itself) pins this restatement, both forms.
"""
import numpy as np
import torch
import torch.nn.functional as F

import golden_cases as gc
from dict_tts_amd import synth
from oracle import dict_tts_ref as ref

SEED = gc.SEED
# the two reference configurations G11 runs (cwd = the reference's root); README command-line overrides as in G1-G6
FORMS = {
    "embed": {"config": "egs/datasets/audio/wenetspeech/dict_tts.yaml", "num_spk": 4,
              "hparams_str": "use_word_input=True,word_size=8000,use_dict=True,num_spk=4",
              "hparams": {"use_spk_embed": True, "num_spk": 4}},
    "id": {"config": "egs/datasets/audio/biaobei/dict_tts.yaml", "num_spk": 8,
           "hparams_str": "use_word_input=True,word_size=8000,use_dict=True,use_spk_id=True,num_spk=8",
           "hparams": {"use_spk_id": True, "num_spk": 8}},
}
G11_SENTENCES = (3, 10, 17, 25, 33)          # Biaobei sentences of 9-25 words: a ragged batch
G11_SPK_IDS = np.array([3, 0, 7, 3, 5], np.int64)   # mixed, one repeated, both ends of [0, num_spk)


def g11_batch():
    st = synth.biaobei_struct()
    return synth.make_batch([st["sentences"][i] for i in G11_SENTENCES], SEED, pron_every=2)


def g11_speakers(form):
    if form == "id":
        return G11_SPK_IDS.copy()
    return synth.speaker_inputs(SEED, "embed", len(G11_SENTENCES), name="g11.spk")


def g11_noise(form, B, T4):
    return synth.noise(SEED, B, T4, f"g11.z.{form}")


def g11_state_dict(form):
    return synth.dict_tts_state_dict(SEED, n_phone=6, speaker=form, num_spk=FORMS[form]["num_spk"])


def project(sd, form, spk):
    """spk_embed_proj(spk) -> [B, hidden] (modules/portaspeech/model.py:159-163), in the state dict's dtype (fp32, or float64 for the
    restatements the GPU is compared with)"""
    if form == "id":
        return F.embedding(spk.long(), sd["spk_embed_proj.weight"])
    return F.linear(spk.to(sd["spk_embed_proj.weight"].dtype), sd["spk_embed_proj.weight"], sd["spk_embed_proj.bias"])


def forward_infer_spk(sd, form, spk, word_tokens, dict_msg, pron_modified, mel2word=None, z_p=None):
    """oracle.dict_tts_ref.forward_infer with the speaker rows of modules/dict_tts/model.py:44-45,94-107.  sd: folded state dict
    (torch), spk: int64 [B] ids (form "id") or fp32 [B, 256] embeddings (form "embed"); z_p as in forward_infer."""
    with torch.no_grad():
        ret = {}
        nonpadding = (1 - word_tokens.eq(0).float())[:, :, None]
        weo, dict_attn, pron_attn, context = ref.dict_encoder(sd, word_tokens, dict_msg, pron_modified)
        weo = weo + project(sd, form, spk)[:, None, :]                       # model.py:94, every row
        ret.update(dict_attn=dict_attn, pron_attn=pron_attn, word_encoder_out=weo, context=context)
        dur, mel2word = ref.add_dur(sd, weo * nonpadding, mel2word)          # model.py:96
        ret["dur"] = dur
        x, tgt_nonpadding, mel2word = ref.expand(weo, mel2word)              # model.py:98-107
        ret["mel2word"] = mel2word
        x = x * tgt_nonpadding
        ret["x_mask"] = tgt_nonpadding
        g = x.transpose(1, 2)
        if callable(z_p):
            z_p = z_p(g.shape[0], g.shape[2] // 4)
        mel, _ = ref.fvae_infer(sd, g, z_p)
        ret["mel_out"] = mel.transpose(1, 2)
        return ret
