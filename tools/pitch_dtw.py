#!/usr/bin/env python
"""The reference's scripts/pitch_dtw.py on the device: `python tools/pitch_dtw.py DIR` reads DIR/f0/*.npy, pairs NAME.npy (the predicted
F0 track) with NAME_gt.npy (the recording's) by name, and prints the four figures the script prints — the mean pitch DTW per ground-truth
frame and the mean sigma, skewness and kurtosis of the predicted tracks."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dict_tts_amd import dtw  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("dir", help="a generated_<steps>_ directory of the reference: its f0/ holds NAME.npy and NAME_gt.npy")
    args = ap.parse_args()
    f0 = os.path.join(args.dir, "f0")
    pairs = dtw.pair_f0_files(os.listdir(f0))
    res = dtw.pitch_dtw([np.load(os.path.join(f0, p)) for p, _ in pairs], [np.load(os.path.join(f0, g)) for _, g in pairs])
    for k in ("dtw", "std", "skew", "kurtosis"):
        print(res[k])


if __name__ == "__main__":
    main()
