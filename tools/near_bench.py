#!/usr/bin/env python3
"""Time proximity queries (sme_query_near_device) at c2 size beside phrase queries
(sme_query_phrase_device) over the same batches, in one process.

The batches are tools/phrase_bench.py's: hit2 / hit3 / hit5, phrases of 2, 3 and 5
terms sampled from the term streams of the corpus's first documents, and miss3,
random term triples drawn proportional to df, which mostly miss.  Each batch runs
as

  phrase     sme_query_phrase_device: the baseline, code this feature does not change
  od1        ordered window, N = 1: the same predicate, so the same answers
  od8        ordered window, N = 8
  uw8        unordered window, N = 8

order 1 (score descending), m 10.  After one warm-up call of each, the four run in
turn `--reps` times (alternating, so drift hits all alike); a figure is the median
host wall time of one call, which ends in a device synchronize.  The three stats of
each are sme_query_near_stats' / sme_query_phrase_stats'.

Writes profiles/near_c2.json.  A report: no figure here is a pass/fail bound.

    python tools/near_bench.py [--docs 1000000] [--vocab 1048576] [--phrases 1024] [--reps 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--phrases", type=int, default=1024)
    p.add_argument("--m", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--width", type=int, default=8)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "near_c2.json"))
    a = p.parse_args()

    import torch
    torch.cuda.init()
    sme = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd")
    synth = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd.synth")
    from phrase_bench import sample_phrases

    corpus = sme.DeviceCorpus(a.docs, V=a.vocab, seed=42, len_lo=400, len_hi=600)
    ctx = sme.Context(1, 10)
    ctx.load_docno_mapping(synth.mapping_bytes(a.docs))
    ctx.set_option("positions", 1)
    ix = ctx.build_device(corpus.ptr, corpus.nbytes)
    records, positions, nbytes = ix.positions()
    out = {"config": {"docs": a.docs, "vocab": a.vocab, "phrases": a.phrases, "order": 1, "m": a.m, "reps": a.reps,
                      "width": a.width, "bool_chunk": 1024},
           "index": {"N": ix.N, "V": ix.V, "P": ix.P, "stream_records": records, "stream_positions": positions},
           "what": ("ms: median host wall time of one sme_query_near_device / sme_query_phrase_device call (validate, "
                    "upload, plan, filter, verify, compact, score, order, cut; outputs left in HBM), the four variants "
                    "of a batch alternating; candidates / verified / matches: the call's stats"),
           "batches": {}}

    texts = sample_phrases(ctx, synth, a.vocab, a.phrases, 1)
    batches = {}
    for name, phs in texts.items():
        words = sorted({t for ph in phs for t in ph})
        table = dict(zip(words, ix.lookup(words).tolist()))
        batches[name] = [[table[t] for t in ph] for ph in phs]
    df = np.diff(ix.offsets())
    terms, _ = synth.queries_by_df(df, a.phrases, seed=4, qlen_lo=3, qlen_hi=3)
    batches["miss3"] = [[int(t) for t in terms[3 * q:3 * q + 3]] for q in range(a.phrases)]

    for name, phs in batches.items():
        pa = sme.Index.phrase_arrays(phs)
        variants = {
            "phrase": (lambda: ix.query_phrase_device(None, 1, a.m, arrays=pa),
                       lambda: ix.query_phrase(None, 1, a.m, arrays=pa), ix.phrase_stats),
        }
        for key, width, ordered in (("od1", 1, True), ("od%d" % a.width, a.width, True),
                                    ("uw%d" % a.width, a.width, False)):
            na = sme.Index.near_arrays([(ph, width, ordered) for ph in phs])
            variants[key] = (lambda na=na: ix.query_near_device(None, 1, a.m, arrays=na),
                             lambda na=na: ix.query_near(None, 1, a.m, arrays=na), ix.near_stats)
        rows, res = {}, {}
        for key, (dev, host, stats) in variants.items():  # warm-up, and the answers' sizes
            res[key] = host()
            s = stats()
            rows[key] = {"runs_ms": [], "candidates": s[0], "verified": s[1], "matches": s[2],
                         "results": int(res[key][0][-1]), "queries_with_a_match": int((np.diff(res[key][0]) > 0).sum())}
        same = all(np.array_equal(x, y) for x, y in zip(res["phrase"][:3], res["od1"][:3])) and \
            res["phrase"][3].tobytes() == res["od1"][3].tobytes()
        for _ in range(a.reps):
            for key, (dev, _, _) in variants.items():
                t0 = time.perf_counter()
                dev()
                rows[key]["runs_ms"].append((time.perf_counter() - t0) * 1e3)
        for key, row in rows.items():
            row["ms"] = statistics.median(row["runs_ms"])
            row["queries_per_s"] = len(phs) / (row["ms"] * 1e-3)
            print("%-6s %-7s %9.3f ms  cands %11d verified %10d matches %9d" % (
                name, key, row["ms"], row["candidates"], row["verified"], row["matches"]), flush=True)
        out["batches"][name] = {"queries": len(phs), "od1_equals_phrase": bool(same), **rows}
    ix.close()
    # what other measurements left in the profile (the phrase path on the parent commit
    # and on this one, tools/phrase_bench.py) stays: this tool owns the keys above only
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = {**{k: v for k, v in json.load(f).items() if k not in out}, **out}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
