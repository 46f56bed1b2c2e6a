#!/usr/bin/env python3
"""What an in-place edit of the resident dictionary costs (PortaSpeech_dict.edit_dict_table, csrc/dict_edit.hip) against the only way
there was before it: uploading the whole dictionary again.  On the full zh-dict.json table (7,030 entries, 211,072 gloss rows, seeded
embeddings), in ONE process, the variants ALTERNATE call by call; wall time around a call that ends in a device synchronisation, median of
--reps (at least 20) after --warmup:

  (a) upload_dict_table of the whole dictionary                      (host rows -> device, every row projected)
  (b) edit_dict_table replacing 1 / 16 / 256 entries from HOST rows  (each replacement one row longer than its victim: every later row moves)
  (c) the same from DEVICE rows
  (d) the segment-copy kernel alone on the K array (DTTS_TIMER_DICT_SEG_COPY: device events around that one launch): the bytes it reads and
      writes (2 x rows x hidden x 4) over its time, beside the 6.29 TB/s float4-copy figure of the MI355X.

It also CHECKS the edit at this size, where the projection's launch shape differs from the upload's (a few 32-row tiles against 6,596):
after the 256-entry edit every entry of the table equals, bit for bit, a fresh context's upload of the edited dictionary.

    python tools/dict_edit_bench.py [--reps 20] [--warmup 3] [--out profiles/dict_edit_bench.txt]

No gate: figures for LABNOTES.md."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

COPY_PEAK_TBS = 6.29


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def replacement(table, e, rng, D):
    """an item for entry e, one gloss row longer than the entry it replaces"""
    a, b, p, q = table["tok_off"][e], table["tok_off"][e + 1], table["pin_off"][e], table["pin_off"][e + 1]
    key = (0.5 * rng.standard_normal((b - a + 1, D))).astype(np.float32)
    return {"key": key, "key_map": np.concatenate([table["key_map"][a:b], [0]]).astype(np.float32), "pinyin": table["pinyin"][p:q],
            "pinyin_map": table["pinyin_map"][p:q]}


def edited_table(table, rep):
    """the ragged arrays of the dictionary after ``rep`` {entry: item}"""
    n = len(table["L"])
    parts = {k: [] for k in ("keys", "key_map", "pinyin", "pinyin_map")}
    tok_off, pin_off = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    for e in range(n):
        a, b, p, q = table["tok_off"][e], table["tok_off"][e + 1], table["pin_off"][e], table["pin_off"][e + 1]
        it = rep.get(e)
        rows = {"keys": it["key"], "key_map": it["key_map"], "pinyin": it["pinyin"], "pinyin_map": it["pinyin_map"]} if it is not None else \
               {"keys": table["keys"][a:b], "key_map": table["key_map"][a:b], "pinyin": table["pinyin"][p:q], "pinyin_map": table["pinyin_map"][p:q]}
        for k, v in rows.items():
            parts[k].append(v)
        tok_off[e + 1], pin_off[e + 1] = tok_off[e] + len(rows["keys"]), pin_off[e] + len(rows["pinyin"])
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out.update(tok_off=tok_off, pin_off=pin_off, L=np.diff(tok_off), P=np.diff(pin_off), ids=table["ids"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20 (a median of fewer calls is not reported)")
    from dict_tts_amd import abi, synth
    from dict_tts_amd import model as M

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    sd = {k: T(v) for k, v in synth.dict_tts_state_dict(1234).items()}
    table = synth.dict_table(1234, synth.zh_dict_struct()["entries"])
    n, nL, D = len(table["L"]), int(table["tok_off"][-1]), table["keys"].shape[1]
    m = M.PortaSpeech_dict(hparams={})
    m.load_state_dict(sd)
    C = m.cfg.hidden_size
    m.ctx.timer_enable(abi.TIMER_DICT_SEG_COPY)
    say(f"dictionary: {n} entries, {nL} gloss rows x {D} (host rows {nL * D * 4 / 1e6:.0f} MB); resident K + V {2 * nL * C * 4 / 2 ** 20:.0f} MiB; "
        f"device {torch.cuda.get_device_name(0)}")
    rng = np.random.default_rng(7)
    edits = {}
    for k in (1, 16, 256):
        ids = [int(v) for v in np.linspace(n // (2 * k), n - 1 - n // (2 * k), k).round()] if k > 1 else [n // 2]
        assert len(set(ids)) == k
        host = {e: replacement(table, e, rng, D) for e in ids}
        dev = {e: {**it, "key": T(it["key"]).cuda()} for e, it in host.items()}
        edits[k] = (host, dev)
    fns = {"(a) upload_dict_table, whole dictionary": lambda: m.upload_dict_table(table)}
    for k, (host, dev) in edits.items():
        fns[f"(b) edit_dict_table, {k:3d} entries, host rows"] = lambda host=host: m.edit_dict_table(replace=host)
        fns[f"(c) edit_dict_table, {k:3d} entries, device rows"] = lambda dev=dev: m.edit_dict_table(replace=dev)
    m.upload_dict_table(table)
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    seg = {k: [] for k in fns}   # (d): the K array's segment-copy launch of each edit, ms
    for _ in range(a.reps):
        for k, fn in fns.items():
            m.ctx.timer_reset()
            ms[k].append(timed(fn))
            t, launches = m.ctx.timer_read(abi.TIMER_DICT_SEG_COPY)
            if launches:
                assert launches == 1
                seg[k].append(t)
    say(f"median (min .. max) ms over {a.reps} calls, variants alternating; each call ends in a device synchronisation")
    base = float(np.median(ms["(a) upload_dict_table, whole dictionary"]))
    for k, v in ms.items():
        say(f"  {k:52s} {np.median(v):9.2f} ({np.min(v):.2f} .. {np.max(v):.2f})   x{base / np.median(v):.1f} vs (a)")
    say("(d) the segment-copy launch on the K array (device events), bytes read + written over its time")
    for k, v in seg.items():
        if not v:
            continue
        rows = nL + (int(k.split(",")[1].split()[0]))   # every replacement is one row longer
        tbs = 2 * rows * C * 4 / (np.median(v) * 1e-3) / 1e12
        say(f"  {k:52s} {np.median(v) * 1e3:8.1f} us  {2 * rows * C * 4 / 1e6:6.1f} MB  {tbs:5.2f} TB/s = {100 * tbs / COPY_PEAK_TBS:4.1f} % of the "
            f"{COPY_PEAK_TBS} TB/s float4 copy")
    # ---- the check at this size: the 256-entry edit from device rows against a fresh upload of the edited dictionary
    host, dev = edits[256]
    m.upload_dict_table(table)
    m.edit_dict_table(replace=dev)
    fresh = M.PortaSpeech_dict(hparams={})
    fresh.load_state_dict(sd)
    fresh.upload_dict_table(edited_table(table, host))
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    bad = 0
    for e in range(n):
        x, y = m.dict_entry(e), fresh.dict_entry(e)
        ok = (x["L"], x["P"]) == (y["L"], y["P"]) and all(torch.equal(bits(x[k]), bits(y[k])) for k in ("K", "V", "key_map", "pinyin", "pinyin_map"))
        bad += 0 if ok else 1
    say(f"check: after the 256-entry edit {n - bad} of {n} entries equal a fresh upload of the edited dictionary bit for bit"
        + ("" if not bad else "  <-- MISMATCH"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
