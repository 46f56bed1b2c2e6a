"""What the fetch units share, without a GPU: every unit that checks its argument block before the handle (items 15 to 21) words a bad
size and a null handle the same way, the units that need the handle first (items 10 to 14) refuse a null one without a message, and
``abi.Context._fetch_block`` can name every block item of include/dicttts_hip.h."""
import ctypes as C
import os
import re

import pytest

from dict_tts_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (item, a block the unit accepts up to the handle): plausible fake device pointers, never dereferenced without a handle
BLOCK_FIRST = [
    (abi.OUT_DTW, lambda: abi.dtw_args(B=2, x=0x1000, y=0x2000, x_ld=40, y_ld=44, dist=0x3000, path=0x4000, path_ld=83, path_len=0x5000)),
    (abi.OUT_PITCH, lambda: abi.pitch_args(B=2, wav=0x1000, wav_ld=4096, frames_ld=13, f0=0x2000, n_frames=0x3000, lens=0x4000)),
    (abi.OUT_RESAMPLE, lambda: abi.resample_args(B=2, wav=0x1000, wav_ld=4096, out=0x2000, out_ld=2000, out_lens=0x3000, sr_in=48000, sr_out=22050)),
    (abi.OUT_LOUDNESS, lambda: abi.loudness_args(B=2, wav=0x1000, wav_ld=48000, blocks_ld=27, sample_rate=16000, lufs=0x2000, gain=0x3000,
                                                 status=0x4000)),
    (abi.OUT_DISC, lambda: abi.disc_args(B=2, y=0x1000, y_hat=0x2000, wav_ld=64, sums=0x3000, counts=0x4000, status=0x5000)),
    (abi.OUT_SPKENC, lambda: abi.spkenc_args(B=1, wav=0x1000, wav_ld=100, embed=0x2000, n_partials=0x3000)),
    (abi.OUT_MELDISC, lambda: abi.meldisc_args(n_sig=2, mel=0x1000, T_ld=200, n_win=3, clips_ld=4, sums=0x2000, counts=0x3000, status=0x4000,
                                               hop=(16, 32, 64))),
]
HANDLE_FIRST = [(abi.OUT_MELSPEC, abi.MelspecArgs), (abi.OUT_STFT_DISTANCE, abi.StftArgs), (abi.OUT_SPECTRAL, abi.SpectralArgs),
                (abi.OUT_GRIFFIN_LIM, abi.GriffinLimArgs), (abi.OUT_LOSSES, abi.LossArgs)]


@pytest.fixture(scope="module")
def lib():
    return abi.load_library()


def fetch(lib, what, block):
    rc = lib.dtts_text2mel_fetch(None, what, C.byref(block), None)
    return rc, lib.dtts_last_error(None).decode()


@pytest.mark.parametrize("what,make", BLOCK_FIRST, ids=[abi.OUT_NAMES[w] for w, _ in BLOCK_FIRST])
def test_block_first_units_word_size_and_handle_alike(lib, what, make):
    a = make()
    a.size -= 8
    rc, msg = fetch(lib, what, a)
    assert rc == -22 and abi.OUT_NAMES[what] in msg and f"size = {C.sizeof(a) - 8}" in msg, (rc, msg)
    rc, msg = fetch(lib, what, make())
    assert rc == -22 and msg == f"dtts_text2mel_fetch({abi.OUT_NAMES[what]}): null handle", (rc, msg)


def test_handle_first_units_refuse_a_null_handle_without_a_message(lib):
    rc, before = fetch(lib, abi.OUT_DTW, abi.dtw_args(B=0, x=0, y=0, x_ld=1, y_ld=1, dist=0))   # leaves a message behind
    assert rc == -22 and "B = 0" in before
    for what, cls in HANDLE_FIRST:
        assert fetch(lib, what, cls(C.sizeof(cls))) == (-22, before), abi.OUT_NAMES[what]
    assert lib.dtts_text2mel_fetch(None, abi.OUT_LOSSES, None, None) == -22
    assert lib.dtts_last_error(None).decode() == before


def test_an_unknown_item_with_a_null_handle_is_invalid(lib):
    block = abi.DtwArgs(C.sizeof(abi.DtwArgs))
    for what in (0, -1, 22, 1000):
        assert what not in abi.OUT_NAMES
        assert lib.dtts_text2mel_fetch(None, what, C.byref(block), None) == -22


def test_fetch_block_can_name_every_block_item_of_the_header():
    with open(os.path.join(ROOT, "include", "dicttts_hip.h")) as f:
        header = {int(v): n for n, v in re.findall(r"^#define (DTTS_OUT_\w+) (\d+)\b", f.read(), re.M)}
    assert len(header) == 21 and set(header) == set(range(1, 22))
    blocks = {v: n for v, n in header.items() if v >= 9}
    assert {v: abi.OUT_NAMES[v] for v in blocks} == blocks
    assert {v: n for v, n in abi.OUT_NAMES.items() if v >= 9} == blocks   # and nothing the header does not know
    assert {w for w, _ in BLOCK_FIRST} | {w for w, _ in HANDLE_FIRST} | {abi.OUT_POSTERIOR} == set(blocks)
