#!/usr/bin/env python
"""The reference's scripts/pitch_dtw.py on the device: `python tools/pitch_dtw.py DIR` reads DIR/f0/*.npy, pairs NAME.npy (the predicted
F0 track) with NAME_gt.npy (the recording's) by name, and prints the four figures the script prints — the mean pitch DTW per ground-truth
frame and the mean sigma, skewness and kurtosis of the predicted tracks.

`python tools/pitch_dtw.py --wavs DIR` starts from the waveforms instead: NAME.wav (the vocoded prediction) against NAME_gt.wav (the
recording), paired by the same rule; the F0 tracks are extracted on the device (dict_tts_amd/pitch.py, Praat's autocorrelation method with
the reference's get_pitch parameters) and go to the DTW without leaving it."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dict_tts_amd import dtw  # noqa: E402


def from_wavs(wav_dir, sample_rate, hop_size, resample=False):
    from dict_tts_amd import pitch
    from dict_tts_amd.melspec import read_wav
    pairs = dtw.pair_f0_files(os.listdir(wav_dir), ext=".wav")
    if resample:   # librosa.load: files at another rate are resampled on the device (kaiser_best)
        from dict_tts_amd.wavprep import load_wav
        cache = {}
        load = lambda names: [load_wav(os.path.join(wav_dir, n), sample_rate, resampler_cache=cache) for n in names]
    else:
        load = lambda names: [read_wav(os.path.join(wav_dir, n), sample_rate) for n in names]
    pred, gt = load([p for p, _ in pairs]), load([g for _, g in pairs])

    def pad(wavs):
        lens = np.asarray([len(w) for w in wavs], np.int32)
        out = np.zeros((len(wavs), int(lens.max())), np.float32)
        for b, w in enumerate(wavs):
            out[b, :lens[b]] = w
        return out, lens

    return pitch.pitch_dtw_from_wavs(*pad(pred), *pad(gt), sample_rate=sample_rate, hop_size=hop_size)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("dir", help="a generated_<steps>_ directory of the reference: its f0/ holds NAME.npy and NAME_gt.npy; with --wavs, a directory "
                                "of NAME.wav and NAME_gt.wav")
    ap.add_argument("--wavs", action="store_true", help="DIR holds waveforms: extract the F0 tracks on the device first")
    ap.add_argument("--sample-rate", type=int, default=22050, help="audio_sample_rate of the waveforms (--wavs; a file at another rate is refused unless --resample)")
    ap.add_argument("--resample", action="store_true", help="with --wavs: resample files at another rate to --sample-rate on the device")
    ap.add_argument("--hop-size", type=int, default=256, help="hop_size: the tracker's time step in samples (--wavs)")
    args = ap.parse_args()
    if args.wavs:
        res = from_wavs(args.dir, args.sample_rate, args.hop_size, args.resample)
    else:
        f0 = os.path.join(args.dir, "f0")
        pairs = dtw.pair_f0_files(os.listdir(f0))
        res = dtw.pitch_dtw([np.load(os.path.join(f0, p)) for p, _ in pairs], [np.load(os.path.join(f0, g)) for _, g in pairs])
    for k in ("dtw", "std", "skew", "kurtosis"):
        print(res[k])


if __name__ == "__main__":
    main()
