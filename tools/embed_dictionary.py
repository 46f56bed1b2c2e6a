#!/usr/bin/env python3
"""Gloss embeddings of a tokenised dictionary on the device: what the reference's binariser writes as ``dict_embed``.

    python tools/embed_dictionary.py --model pretrained/roformer-chinese-base --glosses glosses.json --out table.npz
    python tools/embed_dictionary.py --model ... --glosses glosses.json --out dict_embed.pt --items

glosses.json: {"n_words": N, "entries": {"<word id>": [{"pinyin": ["<initial>", "<final_tone3>"], "ids": [101, ..., 102]}, ...]}} — per word
the glosses of its pronunciations in dictionary order, tokenised by the caller (INTEGRATION.md "Gloss encoder": which ``transformers`` call
gives the ids).  Words without an entry get the binariser's ``<UNK>`` item.

--out table.npz: the ragged arrays of dtts_dict_table_upload (dict_embed.table_from_items) + ``pinyin_encoder``; --items: the item dicts
themselves (``torch.save``), as ``dict_embed.read_indexed_dataset`` returns them."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, help="directory with config.json and pytorch_model.bin")
    ap.add_argument("--glosses", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--items", action="store_true", help="write the dict_embed item dicts instead of the table")
    ap.add_argument("--n-hidden", type=int, default=8)
    ap.add_argument("--row-budget", type=int, default=16384)
    a = ap.parse_args()
    from dict_tts_amd import gloss_encoder as G

    with open(a.glosses) as f:
        spec = json.load(f)
    entries = {int(w): [((g["pinyin"][0], g["pinyin"][1]), g["ids"]) for g in gl] for w, gl in spec["entries"].items()}
    enc = G.GlossEncoder.from_pretrained(a.model, n_hidden=a.n_hidden, row_budget=a.row_budget)
    if a.items:
        torch.save(enc.build_items(entries, spec["n_words"]), a.out)
    else:
        t = enc.build_table(entries, spec["n_words"])
        np.savez(a.out, **{k: v for k, v in t.items() if k not in ("ids", "values", "pinyin_encoder")}, pinyin_encoder=np.array(t["pinyin_encoder"]))
    print(f"{a.out}: {spec['n_words']} words, {sum(len(g) for g in entries.values())} glosses")


if __name__ == "__main__":
    main()
