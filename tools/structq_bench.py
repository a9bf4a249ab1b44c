#!/usr/bin/env python3
"""Time structured queries (sme_query_structured) at c2 size: a phrase AND-ed with one
required term, as one call with narrowing, as one call without, and as the three-call
host composition the entry replaces.

The phrases are tools/phrase_bench.py's hit2 and hit3 batches (phrases of 2 and 3
terms sampled from the term streams of the corpus's first documents).  Each phrase is
paired with one required term, drawn
  (a) bydf   proportional to df -- a frequent term, which cuts little;
  (b) rare   uniformly from the terms with df <= 100 -- a selective term.
Each of the four batches runs as

  narrow1    one sme_query_structured call, "struct_narrow" 1
  narrow0    the same call, "struct_narrow" 0: every phrase evaluated whole
  compose    sme_query_near (docno order, uncut), sme_query_boolean on the terms
             (docno order, uncut), then per query a numpy intersection, the sum of
             the two scores and the first m by score: what a caller did before

order 1 (score descending), m 10, host entries (the results end on the host in all
three).  After one warm-up of each, the three run in turn `--reps` times
(alternating, so drift hits all alike); a figure is the median host wall time with
the smallest and largest run beside it.  The stats are sme_query_structured_stats'
(leaves, verified, candidates, matches); compose reports sme_query_near_stats' and
sme_query_boolean_stats'.  The tool asserts that the three give the same docnos and
that verified with narrowing is at most verified without.

Writes profiles/structq_c2.json.  A report: apart from those two assertions no
figure here is a pass/fail bound.

    python tools/structq_bench.py [--docs 1000000] [--vocab 1048576] [--queries 1024] [--reps 5]
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


def compose(ix, phrases, terms, m):
    """The host composition: -> (res_off, docno) of phrase AND term, score descending."""
    noff, ndn, _, nsc = ix.query_near([(ph, 1, True) for ph in phrases], 0, 0)
    boff, bdn, bsc = ix.query_boolean([[([t], False)] for t in terms], 0, 0)
    off, out = [0], []
    for i in range(len(phrases)):
        a, b = slice(noff[i], noff[i + 1]), slice(boff[i], boff[i + 1])
        dn, ia, ib = np.intersect1d(ndn[a], bdn[b], assume_unique=True, return_indices=True)
        sc = nsc[a][ia] + bsc[b][ib]
        keep = np.lexsort((dn, -sc))[:m] if m > 0 else np.lexsort((dn, -sc))
        out.append(dn[keep])
        off.append(off[-1] + len(keep))
    return np.array(off, np.int64), (np.concatenate(out) if out else np.zeros(0, np.int32))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--queries", type=int, default=1024)
    p.add_argument("--m", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "structq_c2.json"))
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
    out = {"config": {"docs": a.docs, "vocab": a.vocab, "queries": a.queries, "order": 1, "m": a.m, "reps": a.reps,
                      "bool_chunk": 1024},
           "index": {"N": ix.N, "V": ix.V, "P": ix.P},
           "what": ("ms: median host wall time (min, max beside it) of one sme_query_structured call with "
                    "struct_narrow 1 / 0, and of sme_query_near + sme_query_boolean + a numpy intersection, the "
                    "three alternating; stats: leaves, verified, candidates, matches of the structured calls"),
           "batches": {}}

    texts = sample_phrases(ctx, synth, a.vocab, a.queries, 1)
    df = np.diff(ix.offsets())
    bydf, _ = synth.queries_by_df(df, a.queries, seed=11, qlen_lo=1, qlen_hi=1)
    rng = np.random.default_rng(12)
    rare = rng.choice(np.nonzero((df > 0) & (df <= 100))[0], a.queries)
    for pname in ("hit2", "hit3"):
        phs = texts[pname]
        words = sorted({t for ph in phs for t in ph})
        table = dict(zip(words, ix.lookup(words).tolist()))
        phrases = [[table[t] for t in ph] for ph in phs]
        for tname, terms in (("bydf", bydf), ("rare", rare)):
            terms = [int(t) for t in terms[:len(phrases)]]
            sa = sme.Index.structured_arrays([[([(ph, 1, 1)], False), ([([t], 0, 0)], False)]
                                              for ph, t in zip(phrases, terms)])

            def structured(narrow):
                ctx.set_option("struct_narrow", narrow)
                try:
                    return ix.query_structured(None, 1, a.m, arrays=sa)
                finally:
                    ctx.set_option("struct_narrow", 1)

            variants = {"narrow1": lambda: structured(1), "narrow0": lambda: structured(0),
                        "compose": lambda: compose(ix, phrases, terms, a.m)}
            rows, res = {}, {}
            for key, run in variants.items():  # warm-up, the answers and the stats
                res[key] = run()
                rows[key] = {"runs_ms": [], "results": int(res[key][0][-1])}
                if key == "compose":
                    rows[key]["near_stats"] = list(ix.near_stats())
                    rows[key]["boolean_stats"] = list(ix.boolean_stats())
                else:
                    rows[key]["stats"] = dict(zip(("leaves", "verified", "candidates", "matches"),
                                                  ix.structured_stats()))
            for key in ("narrow0", "compose"):
                assert np.array_equal(res[key][0], res["narrow1"][0]) and np.array_equal(res[key][1], res["narrow1"][1]), key
            assert res["narrow0"][2].tobytes() == res["narrow1"][2].tobytes()
            assert rows["narrow1"]["stats"]["verified"] <= rows["narrow0"]["stats"]["verified"]
            for _ in range(a.reps):
                for key, run in variants.items():
                    t0 = time.perf_counter()
                    run()
                    rows[key]["runs_ms"].append((time.perf_counter() - t0) * 1e3)
            for key, row in rows.items():
                row["ms"] = statistics.median(row["runs_ms"])
                row["min_ms"], row["max_ms"] = min(row["runs_ms"]), max(row["runs_ms"])
                print("%-10s %-8s %9.3f ms (%.3f .. %.3f)  %s" % (
                    pname + "+" + tname, key, row["ms"], row["min_ms"], row["max_ms"],
                    row.get("stats", row.get("near_stats"))), flush=True)
            rows["narrow0_over_narrow1"] = rows["narrow0"]["ms"] / rows["narrow1"]["ms"]
            out["batches"][pname + "+" + tname] = {"queries": len(phrases), **rows}
    ix.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
