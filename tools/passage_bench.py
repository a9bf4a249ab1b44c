#!/usr/bin/env python3
"""Time best passages (sme_query_passages_device) at c2 size, built with "positions" 1,
over two candidate sets that are other features' order 0 device results as they stand:

  or_large   the Boolean OR batch of tools/rescore_bench.py: `--or-queries` queries of
             one OR group of 2-8 terms drawn proportional to df; the query terms are
             the group's
  phrase     tools/phrase_bench.py's `hit3` batch, `--phrases` 3-term windows of
             document streams: few candidates per query; the query terms the phrase's

Legs of a set, alternating, every figure the median of `--reps` host wall times of one
call ending in a device synchronize, after a warm-up call of each: widths 16 and 64,
order 0, min_cover 0, without window terms (m 0: every candidate a row) and with them.
With terms the rows are cut to m = `--terms-m` per query on or_large, where every
candidate's window would pass the limit of 2^31 window term entries; on phrase m is 0.
positions_per_s = the stream positions of the candidates' records (the call's
"positions" count, each position once per candidate) over the call's time; spread_ms is
max - min of a leg's runs.  For scale, the rate of k_phrase_verify's whole call over its
own batch, from profiles/phrase_c2.json (it reads the same streams): verified documents
times the mean record length over the call's time.  Writes profiles/passage_c2.json.

    python tools/passage_bench.py [--docs 1000000] [--vocab 1048576] [--or-queries 256]
                                  [--phrases 1024] [--reps 5]

Kernel time comes from a run of its own under the profiler, one set and width per run:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/passage_bench.py --profile-run or_large:16
    python tools/passage_bench.py --kernel-stats or_large:16=DIR/.../run_kernel_stats.csv [...]

The second command needs no device: it adds k_pw_best's times to the JSON.
"""
import argparse
import csv
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
OUT = os.path.join(ROOT, "profiles", "passage_c2.json")
WIDTHS = (16, 64)


def add_kernel_stats(path, pairs):
    with open(path) as f:
        out = json.load(f)
    for pair in pairs:
        name, csv_path = pair.split("=", 1)
        batch, width = name.split(":")
        with open(csv_path, newline="") as f:
            hit = [r for r in csv.DictReader(f) if "k_pw_best" in r["Name"]]
        assert len(hit) == 1, csv_path
        k = {"calls": int(hit[0]["Calls"]), "avg_ms": float(hit[0]["AverageNs"]) / 1e6,
             "min_ms": float(hit[0]["MinNs"]) / 1e6, "max_ms": float(hit[0]["MaxNs"]) / 1e6}
        row = out["sets"][batch]
        k["positions_per_s"] = row["positions"] / (k["avg_ms"] * 1e-3)
        row.setdefault("best_kernel", {})["width%s" % width] = k
        print(name, k)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def phrase_scale():
    """k_phrase_verify's call over its own batch, from the recorded phrase profile."""
    try:
        with open(os.path.join(ROOT, "profiles", "phrase_c2.json")) as f:
            ph = json.load(f)
    except OSError:
        return None
    mean_len = ph["build"]["stream_positions"] / ph["build"]["stream_records"]
    out = {}
    for name in ("hit2", "hit3"):
        b = ph["batches"][name]
        out[name] = {"verified": b["verified"], "ms": b["ms"],
                     "positions_per_s": b["verified"] * mean_len / (b["ms"] * 1e-3)}
    out["what"] = "verified documents x mean record length / the whole sme_query_phrase_device call's time"
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--or-queries", type=int, default=256)
    p.add_argument("--phrases", type=int, default=1024)
    p.add_argument("--terms-m", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--profile-run", default=None, metavar="SET:WIDTH", help="only that leg's calls, untimed")
    p.add_argument("--kernel-stats", nargs="*", default=None, metavar="SET:WIDTH=CSV")
    p.add_argument("--out", default=OUT)
    a = p.parse_args()
    if a.kernel_stats is not None:
        return add_kernel_stats(a.out, a.kernel_stats)

    import torch
    torch.cuda.init()
    sme = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd")
    synth = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd.synth")
    from phrase_bench import sample_phrases
    from rescore_bench import make_batches

    corpus = sme.DeviceCorpus(a.docs, V=a.vocab, seed=42, len_lo=400, len_hi=600)
    ctx = sme.Context(1, 10)
    ctx.load_docno_mapping(synth.mapping_bytes(a.docs))
    ctx.set_option("positions", 1)
    ix = ctx.build_device(corpus.ptr, corpus.nbytes)
    records, positions, nbytes = ix.positions()
    out = {"config": {"docs": a.docs, "vocab": a.vocab, "widths": list(WIDTHS), "order": 0, "min_cover": 0,
                      "terms_m_or_large": a.terms_m, "reps": a.reps},
           "index": {"N": ix.N, "V": ix.V, "P": ix.P, "stream_records": records, "stream_positions": positions},
           "what": "*_ms: median host wall time of one sme_query_passages_device call ending in a device synchronize, "
                   "the legs alternating; *_spread_ms: max - min of the leg's runs; candidates / with_record / positions "
                   "/ kept / chunk: sme_query_passages_stats; *_positions_per_s: positions / the leg's median time",
           "phrase_verify_scale": phrase_scale(), "sets": {}}
    print("index N %d V %d P %d, %d stream positions" % (ix.N, ix.V, ix.P, positions), flush=True)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def keep(ptr_off, ptr_dn, nq, total):
        """The candidates in tensors of the bench's own (the features reuse the index's buffers)."""
        d_off = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        d_dn = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
        sme.memcpy(d_off.data_ptr(), ptr_off, 8 * (nq + 1))
        sme.memcpy(d_dn.data_ptr(), ptr_dn, 4 * total)
        last = np.zeros(1, np.int64)  # a copy to the host behind the device-to-device copies: they are done
        sme.memcpy(last.ctypes.data, d_off.data_ptr() + 8 * nq, 8)
        assert int(last[0]) == total
        return d_off, d_dn

    sets = {}
    if not a.profile_run or a.profile_run.startswith("or_large"):
        queries = make_batches(ix, synth, a.or_queries, 1, 1)["or_large"]
        r = ix.query_boolean_device(None, 0, 0, arrays=sme.Index.boolean_arrays(queries))
        sets["or_large"] = ([g[0][0] for g in queries], keep(r[0], r[1], len(queries), r[3]), a.terms_m)
    if not a.profile_run or a.profile_run.startswith("phrase"):
        texts = sample_phrases(ctx, synth, a.vocab, a.phrases, 1)["hit3"]
        phrases = [[int(t) for t in ix.lookup(ph)] for ph in texts]
        r = ix.query_phrase_device(phrases, 0, 0)
        sets["phrase"] = (phrases, keep(r[0], r[1], len(phrases), r[4]), 0)

    for name, (listed, (d_off, d_dn), terms_m) in sets.items():
        nq = len(listed)
        ids, qoff = sme.Index.phrase_arrays(listed)

        def call(width, with_terms):
            return ix.passages_device(ids, qoff, d_dn, d_off, width, min_cover=0, order=0,
                                      m=terms_m if with_terms else 0, with_terms=with_terms)

        if a.profile_run:
            for _ in range(a.reps + 1):
                call(int(a.profile_run.split(":")[1]), False)
            torch.cuda.synchronize()
            continue
        legs = {"width%d%s" % (w, "_terms" if t else ""): (lambda w=w, t=t: call(w, t)) for w in WIDTHS
                for t in (False, True)}
        row = {"queries": nq, "listed_ids": int(len(ids))}
        for leg, fn in legs.items():  # (the warm-up; and each leg's rows)
            r = fn()
            row[leg + "_rows"], row[leg + "_window_terms"] = r.total, r.win_total
        row.update(ix.passages_stats())
        runs = {leg: [] for leg in legs}
        for _ in range(a.reps):
            for leg, fn in legs.items():
                runs[leg].append(timed(fn))
        for leg in legs:
            row[leg + "_ms"] = statistics.median(runs[leg])
            row[leg + "_runs_ms"] = runs[leg]
            row[leg + "_spread_ms"] = max(runs[leg]) - min(runs[leg])
            row[leg + "_positions_per_s"] = row["positions"] / (row[leg + "_ms"] * 1e-3)
        out["sets"][name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if not k.endswith("_runs_ms")}}), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (after every set: a long later set loses nothing)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
