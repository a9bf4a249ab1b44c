#!/usr/bin/env python3
"""Time spelling suggestions (sme_index_suggest_terms_device) at c2 size: the
trigram table's build if the index does not have it yet, and a batch of misspelt
words answered from the table ("fuzzy_scan" 0) and by taking the whole vocabulary
as candidates per word ("fuzzy_scan" 1), with sme_index_suggest_stats of both.

The words are drawn from the vocabulary with a fixed seed, each with one or two
random unit edits (substitution, insertion, deletion); max_dist 2, m 10.  Every
figure is the median of `--reps` runs after a warm-up.  A scan leg whose warm-up
shows that `--reps` runs would pass `--scan-budget-s` seconds runs fewer times,
and the output says how many.  Both legs must return the same arrays.

Writes profiles/fuzzy_c2.json.  A report: no figure here is a pass/fail bound.

    python tools/fuzzy_bench.py [--docs 1000000] [--vocab 1048576] [--words 10000] [--reps 5]
"""
import argparse
import importlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHABET = "abcdefghijklmnopqrstuvwxyz0123456789"


def make_words(ix, n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        w = ix.term(rng.randrange(ix.V))
        if not 3 <= len(w) <= 60:
            continue
        for _ in range(1 + len(out) % 2):  # one edit, two edits, alternating
            p = rng.randrange(len(w))
            kind = rng.randrange(3)
            if kind == 0:
                w = w[:p] + rng.choice(ALPHABET) + w[p + 1:]
            elif kind == 1:
                w = w[:p] + rng.choice(ALPHABET) + w[p:]
            elif len(w) > 1:
                w = w[:p] + w[p + 1:]
        out.append(w)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--words", type=int, default=10_000)
    p.add_argument("--max-dist", type=int, default=2)
    p.add_argument("--m", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--scan-budget-s", type=float, default=120.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuzzy_c2.json"))
    a = p.parse_args()

    import torch
    torch.cuda.init()
    sme = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd")
    synth = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd.synth")

    corpus = sme.DeviceCorpus(a.docs, V=a.vocab, seed=42, len_lo=400, len_hi=600)
    ctx = sme.Context(1, 10)
    ctx.load_docno_mapping(synth.mapping_bytes(a.docs))
    ctx.build_device(corpus.ptr, corpus.nbytes).close()  # warm-up: workspace allocation
    ix = ctx.build_device(corpus.ptr, corpus.nbytes)
    table_ms = ix.prepare_wildcards()  # not there yet on a fresh index: this is its build
    G, pairs = ix.wildcard_stats()
    V = ix.V
    words = make_words(ix, a.words, 1)

    def run(scan, reps):
        ctx.set_option("fuzzy_scan", scan)
        t0 = time.perf_counter()
        first = ix.suggest_terms(words, a.max_dist, a.m)  # warm-up; also the arrays to compare
        warm = time.perf_counter() - t0
        if scan and warm * reps > a.scan_budget_s:
            reps = max(1, int(a.scan_budget_s / warm))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ix.suggest_terms_device(words, a.max_dist, a.m)
            ts.append((time.perf_counter() - t0) * 1e3)
        return first, ts, ix.suggest_stats()

    tab, tab_ts, tab_stats = run(0, a.reps)
    scn, scn_ts, scn_stats = run(1, a.reps)
    ctx.set_option("fuzzy_scan", 0)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(tab, scn))
    t_tab, t_scn = statistics.median(tab_ts), statistics.median(scn_ts)
    out = {
        "config": {"docs": a.docs, "vocab": a.vocab, "words": len(words), "max_dist": a.max_dist, "m": a.m,
                   "reps": a.reps, "scan_reps": len(scn_ts), "wild_chunk": 1024},
        "index": {"N": ix.N, "V": V, "P": ix.P},
        "table_build_ms": table_ms,
        "table": {"grams": G, "pairs": pairs, "bytes": 8 * G + 4 * (G + 1) + 4 * pairs},
        "suggestions": int(tab[0][-1]),
        "words_without_suggestion": int(np.sum(np.diff(tab[0]) == 0)),
        "words_with_exact_term": int(np.sum(tab[2][tab[0][:-1][np.diff(tab[0]) > 0]] == 0)),
        "suggest_table_ms": t_tab,
        "suggest_table_runs_ms": tab_ts,
        "suggest_table_stats": {"scanned_words": tab_stats[0], "candidates": tab_stats[1]},
        "suggest_scan_ms": t_scn,
        "suggest_scan_runs_ms": scn_ts,
        "suggest_scan_stats": {"scanned_words": scn_stats[0], "candidates": scn_stats[1]},
        "paths_identical": bool(same),
        "table_faster_than_scan": bool(t_tab < t_scn),
        "what": "suggest_*_ms: host wall time of one sme_index_suggest_terms_device call (parse, upload, plan, "
                "count, emit, two sorts, cut; outputs left in HBM); table_build_ms: device time of the trigram "
                "table's build on the fresh index; *_stats: sme_index_suggest_stats after the leg",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    assert same, "table and scan paths disagree"


if __name__ == "__main__":
    main()
