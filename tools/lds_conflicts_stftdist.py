#!/usr/bin/env python3
"""Conflict degree of the slab read (ds_read_b32) of stftdist.hip's contraction, enumerated on the CPU.

Lane l of a wave reads sample a = (16 w + (l & 15)) * hop + k + (l >> 5) of slab x (lanes with l & 16 == 0) or of slab y (l & 16 != 0); sample a
lives at LDS dword a + (a >> ps) of its slab, slab x starts at dword 0 and slab y at dword ybase.  The LDS serves a ds_read_b32 in two
groups, the 32-lane halves, over 32 banks of one dword; a group's degree is the largest number of its lanes on one bank; 1 = conflict-free.
A half holds 16 rows of slab x and the same 16 rows of slab y: with ybase = 16 (mod 32) the y rows fall half a bank row away from the x rows.
Enumerated over every wave of a tile (w = 0 .. 3) and every phase k, as stft_conflict_degree (dict_tts_amd/csrc/stftdist.hip) does;
stft_layout takes, over ps = 31 (no skew), 8, 7, 6, 5 and ybase = one slab + 0 .. 31, the first pair with the smallest degree.

usage: lds_conflicts_stftdist.py [n_fft:hop ...]      (default: the reference's three resolutions)"""
import sys

WAVES, LDS_BYTES, RED_DWORDS = 4, 160 * 1024, 24


def degree(hop, ps, ybase):
    worst = 1
    for w in range(WAVES):
        for k in range(1 << min(ps, 8)):
            banks = {}
            for t in range(32):
                a = (16 * w + (t & 15)) * hop + k
                bank = ((t >> 4) * ybase + a + (a >> ps)) % 32
                banks[bank] = banks.get(bank, 0) + 1
            worst = max(worst, max(banks.values()))
    return worst


def slab_dwords(tt, hop, n_fft, ps):
    P = (tt - 1) * hop + n_fft
    return P + (P >> ps) + 1


def lds_bytes(tt, hop, n_fft, ps, ybase):
    return ((ybase + slab_dwords(tt, hop, n_fft, ps) + 1) & ~1) * 4 + RED_DWORDS * 4


def layout(hop, n_fft):
    best = None
    for ps in (31, 8, 7, 6, 5):
        tt = 16 * WAVES
        while tt > 1 and lds_bytes(tt, hop, n_fft, ps, slab_dwords(tt, hop, n_fft, ps) + 31) > LDS_BYTES:
            tt -= 1
        S = slab_dwords(tt, hop, n_fft, ps)
        for o in range(32):
            d = degree(hop, ps, S + o)
            if best is None or d < best["degree"]:
                best = dict(ps=ps, tt=tt, ybase=S + o, offset=o, degree=d, lds=lds_bytes(tt, hop, n_fft, ps, S + o), back_to_back=degree(hop, ps, S))
    return best


def main():
    cases = [tuple(int(v) for v in a.split(":")) for a in sys.argv[1:]] or [(1024, 120), (2048, 240), (512, 50)]
    print(f"{'n_fft':>5} {'hop':>5} {'pairs':>5} {'skew':>8} {'ybase':>7} {'(slab +)':>8} {'degree':>6} {'slab y at the end of slab x':>28} {'LDS bytes':>10}")
    for n_fft, hop in cases:
        b = layout(hop, n_fft)
        skew = "none" if b["ps"] == 31 else f"ps={b['ps']}"
        print(f"{n_fft:>5} {hop:>5} {b['tt']:>5} {skew:>8} {b['ybase']:>7} {b['offset']:>8} {b['degree']:>6} {b['back_to_back']:>28} {b['lds']:>10}")


if __name__ == "__main__":
    main()
