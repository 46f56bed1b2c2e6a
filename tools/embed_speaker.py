#!/usr/bin/env python3
"""Speaker embeddings of recordings, on the device: what the reference's binariser stores as ``spk_embed``.

    python tools/embed_speaker.py --ckpt pretrained.pt a.wav [b.wav ...] [--preprocess] [--out spk.npy] [--pad-mode constant|reflect]

--ckpt: Resemblyzer's checkpoint ({"model_state": state_dict, ...}) or a bare state dict.  One recording -> its utterance embedding
[256]; several -> the speaker embedding (the normalised mean of the utterance embeddings).  The result is float32 [1, 256] in --out, what
``PortaSpeech_dict.forward(spk_embed=...)`` takes for a batch of one.

Without --preprocess the samples are taken AS IF at 16 kHz whatever the file's rate, as the reference's binariser takes its 22.05 kHz
waveforms (the form a shipped checkpoint was trained on).  --preprocess resamples to 16 kHz and raises quiet recordings to -30 dBFS
(Resemblyzer's preprocess_wav without its VAD trim, which is not implemented)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np


def read_wav(path):
    """-> (float32 mono in [-1, 1), sample rate)"""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.ndim > 1:
        data = data.mean(axis=1)
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float64) / float(np.iinfo(data.dtype).max + 1)
    return np.asarray(data, np.float32), int(sr)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("wavs", nargs="+")
    ap.add_argument("--preprocess", action="store_true")
    ap.add_argument("--out", default="spk.npy")
    ap.add_argument("--pad-mode", choices=("constant", "reflect"), default="constant")
    a = ap.parse_args()
    from dict_tts_amd import speaker_encoder as E

    enc = E.VoiceEncoder.from_checkpoint(a.ckpt, pad_mode=a.pad_mode)
    wavs = []
    for path in a.wavs:
        w, sr = read_wav(path)
        wavs.append(E.preprocess_wav(w, source_sr=sr) if a.preprocess else w)
    embed = enc.embed_utterance(wavs[0]) if len(wavs) == 1 else enc.embed_speaker(wavs)
    np.save(a.out, np.asarray(embed, np.float32)[None])
    print(json.dumps({"out": a.out, "recordings": len(wavs), "samples": [len(w) for w in wavs], "preprocess": a.preprocess,
                      "finite": bool(np.all(np.isfinite(embed)))}))


if __name__ == "__main__":
    main()
