#!/usr/bin/env python3
"""Bit-identity record of the three spectral units (log-mel, STFT distance, STFT -> edit -> inverse STFT) across two builds of the library
(a refactor's check: nothing may move).  The sibling of tools/voc_bits.py.

    tools/spectral_bits.py --lib PATH --out FILE      the units on seeded inputs on the build at PATH: the SHA-256 of every WHOLE output buffer, as JSON
    tools/spectral_bits.py --compare A.json B.json    case by case; exit status 1 when a hash differs or a case is missing

Every output buffer is filled with a sentinel before the call, so a stray or a missing store changes its hash.  The cases are small (the run
takes seconds) and each reaches one branch of the shared contraction (csrc/stft_core.h) or of a unit's own code:
  melspec   default front end: B = 1 (two-wave tile), the smallest B of 101-frame utterances that leaves the two-wave tile on this device
            (2 B > CUs, as tests/test_melspec_gpu.py::_full_tiles_need counts), a ragged B = 3 (length 0, not a multiple of hop, full);
            n_fft 512 / win 240 / hop 50 (sg_lo > 0); n_fft 2048 / hop 2048 (fewer than 32 frames per wave); n_mels 1 and 128; with and without `lin`
  stftdist  the three default resolutions together, a ragged B = 3 with one length <= n_fft / 2 (count 0), with and without `mag`;
            n_fft 2048 at hop 512, where stft_layout gives fewer than 64 frame pairs per tile
  spectral  forward alone, inverse alone and both, v = 0 and v = 0.1, n_fft 512 / 1024 / 2048; at n_fft 1024 one-tile utterances from B = 1
            up to the batch at which both launchers hand a tile's blocks to one workgroup (tests/test_spectral_gpu.py::_split restated)"""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SENTINEL = 777.0


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = 0
    for case in sorted(set(a) | set(b)):
        ra, rb = a.get(case), b.get(case)
        same = ra is not None and ra == rb
        bad += not same
        show = ra or rb
        print(f"{'equal' if same else 'DIFFERENT':9s} {case:44s} " + " ".join(f"{k} {v[:12]}" for k, v in sorted(show.items())))
        if not same:
            print(f"          A: {ra}\n          B: {rb}")
    print(f"{len(set(a) | set(b))} cases, {bad} different: A = {os.path.basename(a_path)}, B = {os.path.basename(b_path)}")
    return 1 if bad else 0


def _split(tiles, blocks, want):
    """istft.hip: istft_split"""
    s = 1
    while s < blocks and tiles * s < want:
        s *= 2
    return s


def record(lib, out_path):
    import numpy as np
    import torch
    from dict_tts_amd import abi
    abi.load_library(os.path.abspath(lib))
    from dict_tts_amd import melspec, spectral, stftloss
    dev = torch.device("cuda", torch.cuda.current_device())
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    res = {}
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    full = lambda shape, dtype, v: torch.full(shape, v, dtype=dtype, device=dev)

    def waves(B, L, lens=None):
        w = np.ones((B, L), np.float32)   # samples past a length are 1.0: they must not be read as signal
        for b in range(B):
            n = L if lens is None else lens[b]
            w[b, :n] = 0.1 * rng.standard_normal(n)
        ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        return torch.from_numpy(w).to(dev), ln

    def done(case, **bufs):
        torch.cuda.synchronize()
        res[case] = {k: sha(v) for k, v in bufs.items()}
        print(f"{case}: " + " ".join(f"{k} {h[:12]}" for k, h in res[case].items()), flush=True)

    # ---- melspec: (n_fft, win, hop, n_mels) -> a context with a seeded non-negative mel basis (the filterbank is the Python side's)
    def mel_ctx(n_fft, win, n_mels):
        ctx = abi.Context()
        ctx.load_state_dict("melspec", {"mel_basis": rng.random((n_mels, n_fft // 2 + 1)).astype(np.float32),
                                        "window": melspec.hann_window(win).astype(np.float32)})
        ctx.finalize(abi.PART_MELSPEC)
        return ctx

    def mel_case(case, ctx, n_mels, hop, B, L, lens=None, lin=True):
        wav, ln = waves(B, L, lens)
        T = 1 + L // hop
        mel, mel_lens = full((B, T, n_mels), torch.float32, SENTINEL), full((B,), torch.int32, -1)
        lin_t = full((B, T, n_mels), torch.float32, SENTINEL) if lin else None
        ctx.melspec(wav.data_ptr(), ln.data_ptr() if ln is not None else None, B, L, hop, mel.data_ptr(), T, mel_lens.data_ptr(), stream,
                    lin=lin_t.data_ptr() if lin else None)
        done(case, mel=mel, mel_lens=mel_lens, **({"lin": lin_t} if lin else {}))

    ctx = mel_ctx(1024, 1024, 80)
    mel_case("melspec/default/b1", ctx, 80, 256, 1, 256 * 40 + 77)
    mel_case("melspec/default/b1_nolin", ctx, 80, 256, 1, 256 * 40 + 77, lin=False)
    mel_case(f"melspec/default/b{cus // 2 + 1}_full_tiles", ctx, 80, 256, cus // 2 + 1, 256 * 100)
    mel_case("melspec/default/b3_ragged", ctx, 80, 256, 3, 256 * 140, lens=[0, 256 * 9 + 77, 256 * 140])
    mel_case("melspec/n512_win240_hop50/b2", mel_ctx(512, 240, 40), 40, 50, 2, 50 * 70 + 3)
    mel_case("melspec/n2048_hop2048/b2", mel_ctx(2048, 2048, 80), 80, 2048, 2, 2048 * 45 + 5)
    mel_case("melspec/mels1/b2", mel_ctx(1024, 1024, 1), 1, 256, 2, 256 * 33)
    mel_case("melspec/mels128/b2", mel_ctx(1024, 800, 128), 128, 200, 2, 200 * 70 + 11)

    # ---- stftdist
    def stft_case(case, mr, B, L, lens=None, mag=True):
        mr._plan()
        y, ln = waves(B, L, lens)
        x = y + torch.from_numpy((0.01 * rng.standard_normal((B, L))).astype(np.float32)).to(dev)
        sums, count = full((mr.n_res, B, 3), torch.float64, SENTINEL), full((mr.n_res, B), torch.int64, -1)
        cap = 1 + L // min(mr.hop_sizes)
        mag_t = full((mr.mag_layout(B, cap)[1],), torch.float32, SENTINEL) if mag else None
        mr.ctx.stft_distance(x.data_ptr(), y.data_ptr(), ln.data_ptr() if ln is not None else None, B, L, mr.hop_sizes, sums.data_ptr(),
                             count.data_ptr(), stream, mag=mag_t.data_ptr() if mag else None, mag_cap=cap if mag else 0)
        done(case, sums=sums, count=count, **({"mag": mag_t} if mag else {}))

    mr3 = stftloss.MultiResolutionSTFT()
    stft_case("stftdist/default3/b3_ragged_mag", mr3, 3, 256 * 80, lens=[200, 256 * 30 + 77, 256 * 80])
    stft_case("stftdist/default3/b2", mr3, 2, 256 * 150 + 9, mag=False)
    stft_case("stftdist/n2048_hop512/b2_mag", stftloss.MultiResolutionSTFT((2048,), (512,), (1200,)), 2, 512 * 90 + 5)

    # ---- spectral: forward alone, inverse alone (on the forward's spectrum) and both, every buffer the caller's
    def spec_case(case, sp, B, L, lens, v):
        sp._plan()
        wav, ln = waves(B, L, lens)
        cap = 1 + L // sp.hop
        ptr = lambda t: t.data_ptr() if t is not None else None
        spec, frames = full((B, cap, sp.n_bins, 2), torch.float32, SENTINEL), full((B,), torch.int32, -1)
        sp.ctx.spectral(abi.SPECTRAL_FORWARD, B, L, sp.hop, cap, stream, wav=wav.data_ptr(), lens=ptr(ln), frames=frames.data_ptr(),
                        spec=spec.data_ptr(), floor=v)
        done(f"{case}/fwd", spec=spec, frames=frames)
        out, out_lens = full((B, L), torch.float32, SENTINEL), full((B,), torch.int32, -1)
        sp.ctx.spectral(abi.SPECTRAL_INVERSE, B, L, sp.hop, cap, stream, frames=frames.data_ptr(), spec=spec.data_ptr(), out=out.data_ptr(),
                        out_lens=out_lens.data_ptr())
        done(f"{case}/inv", out=out, out_lens=out_lens)
        spec2, frames2 = full((B, cap, sp.n_bins, 2), torch.float32, SENTINEL), full((B,), torch.int32, -1)
        out2, out_lens2 = full((B, L), torch.float32, SENTINEL), full((B,), torch.int32, -1)
        sp.ctx.spectral(abi.SPECTRAL_FORWARD | abi.SPECTRAL_INVERSE, B, L, sp.hop, cap, stream, wav=wav.data_ptr(), lens=ptr(ln),
                        frames=frames2.data_ptr(), spec=spec2.data_ptr(), out=out2.data_ptr(), out_lens=out_lens2.data_ptr(), floor=v)
        done(f"{case}/both", spec=spec2, frames=frames2, out=out2, out_lens=out_lens2)

    for n_fft, hop, win in ((512, 128, 400), (1024, 256, 1024), (2048, 300, 1200)):
        sp = spectral.Spectral(dict(fft_size=n_fft, hop_size=hop, win_size=win))
        for v in (0.0, 0.1):
            spec_case(f"spectral/n{n_fft}_hop{hop}/b3_ragged/v{v}", sp, 3, hop * 140, [0, hop * 9 + 77, hop * 140], v)
    sp = spectral.Spectral(dict(fft_size=1024, hop_size=256, win_size=1024))
    seen, B = set(), 1
    while True:   # one-tile utterances: B tiles in both launchers; the forward splits until 4 workgroups per CU, the inverse until 16
        split = (_split(B, 16, 4 * cus), _split(B, 16, 16 * cus))
        if split not in seen:
            seen.add(split)
            spec_case(f"spectral/n1024_hop256/b{B}_split{split[0]}_{split[1]}/v0.1", sp, B, 256 * 9, None, 0.1)
        if split == (1, 1):
            break
        B *= 2
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"{len(res)} cases -> {out_path}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="path of the library build to record")
    ap.add_argument("--out", help="JSON file the record goes to")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if not (a.lib and a.out):
        ap.error("--lib PATH --out FILE, or --compare A.json B.json")
    record(a.lib, a.out)
