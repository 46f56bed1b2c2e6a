#!/usr/bin/env python3
"""Conflict degree of the frame-fragment read (ds_read_b32) of melspec.hip's contraction, enumerated on the CPU.

Lane l of a wave reads sample a = (32 w + (l & 31)) * hop + k + (l >> 5) of the tile's slab, which lives at LDS dword a + (a >> ps)
(the skew).  The LDS serves a ds_read_b32 in two groups, the 32-lane halves, over 32 banks of one dword; a group's degree is the largest
number of its lanes on one bank (the 32 rows of a half are hop >= 1 samples apart: never the same address); 1 = conflict-free.  The two
halves read addresses one sample apart and never conflict with each other.  Enumerated over every wave of a tile (w = 0 .. 3) and every
phase k of the contraction index, as melspec_conflict_degree (dict_tts_amd/csrc/melspec.hip) does; melspec_skew_shift takes the first of
ps = 31 (no skew), 8, 7, 6, 5 with the smallest degree: ties go to the smaller pad.

usage: lds_conflicts_melspec.py [hop ...]      (default: 128 200 256 300 and the unskewed slab for comparison)"""
import sys


def degree(hop, ps):
    worst = 1
    for w in range(4):
        for k in range(1 << min(ps, 8)):
            banks = {}
            for t in range(32):
                a = (32 * w + t) * hop + k
                banks[(a + (a >> ps)) % 32] = banks.get((a + (a >> ps)) % 32, 0) + 1
            worst = max(worst, max(banks.values()))
    return worst


def skew_shift(hop):
    best, deg = 31, None
    for ps in (31, 8, 7, 6, 5):
        d = degree(hop, ps)
        if deg is None or d < deg:
            best, deg = ps, d
    return best


def main():
    hops = [int(a) for a in sys.argv[1:]] or [128, 200, 256, 300]
    print(f"{'hop':>5} {'no skew':>8} " + " ".join(f"ps={ps:<2}" for ps in (8, 7, 6, 5)) + "  chosen")
    for hop in hops:
        row = [degree(hop, ps) for ps in (8, 7, 6, 5)]
        ps = skew_shift(hop)
        how = "no skew" if ps == 31 else f"ps={ps}, pad {100 / (1 << ps):.2f} %"
        print(f"{hop:>5} {degree(hop, 31):>8} " + " ".join(f"{d:>5}" for d in row) + f"  {how} (degree {degree(hop, ps)})")


if __name__ == "__main__":
    main()
