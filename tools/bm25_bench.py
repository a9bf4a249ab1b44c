#!/usr/bin/env python3
"""Time BM25 ranking (sme_query_topk_bm25_device) at c2 size against the exhaustive
streaming TF-IDF scorer (sme_query_topk_device under "query_kernel" 1), which reads
the same posting lists once per query: code the BM25 feature does not touch.

Batches of 2-8 term queries drawn by df (synth.queries_by_df), k = 10, k1 1.2, b 0.75.
Per batch the two scorers alternate; every figure is the median of `--reps` host wall
times of one call ending in a device synchronize, after a warm-up call of each.  The
smallest batch is also run under "bm25_split" 1.  sme_query_bm25_stats of each leg
gives the skip rate (skipped / windows) and the postings scored.

Writes profiles/bm25_c2.json.  A report: no figure here is a pass/fail bound.

    python tools/bm25_bench.py [--docs 1000000] [--vocab 1048576] [--batches 256,100000] [--reps 5]

Kernel time comes from a run of its own under the profiler, one batch per run:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/bm25_bench.py --profile-run --batches 256
    python tools/bm25_bench.py --kernel-stats 256=DIR/.../run_kernel_stats.csv [...]

The second command needs no device: it adds to the JSON, per batch, the scorer
kernel's average time and its achieved bytes/s, (8 B x postings scored) / kernel time.
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
OUT = os.path.join(ROOT, "profiles", "bm25_c2.json")
K, K1, B = 10, 1.2, 0.75


def add_kernel_stats(path, pairs):
    with open(path) as f:
        out = json.load(f)
    for pair in pairs:
        name, csv_path = pair.split("=", 1)
        row = out["batches"][name]
        with open(csv_path, newline="") as f:
            hit = [r for r in csv.DictReader(f) if "k_bm_score" in r["Name"]]
        assert len(hit) == 1, csv_path
        avg_ms = float(hit[0]["AverageNs"]) / 1e6
        row["score_kernel"] = {"calls": int(hit[0]["Calls"]), "avg_ms": avg_ms, "min_ms": float(hit[0]["MinNs"]) / 1e6,
                               "max_ms": float(hit[0]["MaxNs"]) / 1e6,
                               "bytes_per_s": 8.0 * row["bm25_stats"]["postings"] / (avg_ms / 1e3)}
        print(name, row["score_kernel"])
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--batches", default="256,100000")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--profile-run", action="store_true", help="only the BM25 calls, untimed (for the profiler)")
    p.add_argument("--kernel-stats", nargs="*", default=None, metavar="BATCH=CSV")
    p.add_argument("--out", default=OUT)
    a = p.parse_args()
    if a.kernel_stats is not None:
        return add_kernel_stats(a.out, a.kernel_stats)

    import torch
    torch.cuda.init()
    sme = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd")
    synth = importlib.import_module("simple-mapreduce-search-engine-information-retrieval-_amd.synth")

    corpus = sme.DeviceCorpus(a.docs, V=a.vocab, seed=42, len_lo=400, len_hi=600)
    ctx = sme.Context(1, 10)
    ctx.load_docno_mapping(synth.mapping_bytes(a.docs))
    ix = ctx.build_device(corpus.ptr, corpus.nbytes)
    prepare_ms = ix.prepare_bm25()
    st = ix.bm25_stats()
    df = np.diff(ix.offsets())
    out = {"config": {"docs": a.docs, "vocab": a.vocab, "k": K, "k1": K1, "b": B, "reps": a.reps},
           "index": {"N": ix.N, "V": ix.V, "P": ix.P}, "collection": st, "prepare_ms": prepare_ms,
           "what": "bm25_ms / topk_stream_ms: median host wall time of one sme_query_topk_bm25_device / "
                   "sme_query_topk_device (query_kernel 1) call ending in a device synchronize, the two alternating; "
                   "ratio: bm25_ms / topk_stream_ms; list_postings: the postings of the batch's term slots; "
                   "bm25_stats: sme_query_bm25_stats of the leg; skip_rate: skipped / windows",
           "batches": {}}
    print("index N %d V %d P %d, prepare %.3f ms, %s" % (ix.N, ix.V, ix.P, prepare_ms, st), flush=True)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for i, nq in enumerate(int(x) for x in a.batches.split(",")):
        terms, qoff = synth.queries_by_df(df, nq, seed=7)
        d_t = torch.from_numpy(np.ascontiguousarray(terms, np.int32)).cuda()
        d_q = torch.from_numpy(np.ascontiguousarray(qoff, np.int64)).cuda()
        od, os_ = torch.empty(nq * K, dtype=torch.int32, device="cuda"), torch.empty(nq * K, dtype=torch.float64, device="cuda")
        td, ts = torch.empty_like(od), torch.empty_like(os_)

        def bm25(split=0):
            ctx.set_option("bm25_split", split)
            ix.query_bm25_device(d_t.data_ptr(), d_q.data_ptr(), nq, K, od.data_ptr(), os_.data_ptr(), K1, B)
            ctx.set_option("bm25_split", 0)

        def stream():
            ctx.set_option("query_kernel", 1)
            ix.query_topk_device(d_t.data_ptr(), d_q.data_ptr(), nq, K, td.data_ptr(), ts.data_ptr())
            ctx.set_option("query_kernel", 0)

        if a.profile_run:
            for _ in range(a.reps + 1):
                bm25()
            torch.cuda.synchronize()
            continue
        row = {"queries": nq, "slots": int(len(terms)), "list_postings": int(df[terms].sum())}
        legs = {"bm25": bm25, "topk_stream": stream}
        if i == 0:
            legs["bm25_split1"] = lambda: bm25(1)
        warm = {name: timed(call) for name, call in legs.items()}
        row["bm25_stats"] = None
        runs = {name: [] for name in legs}
        reps = {name: max(1, min(a.reps, int(120e3 / max(w, 1e-3)))) for name, w in warm.items()}  # (a leg of minutes: fewer)
        for r in range(a.reps):
            for name, call in legs.items():
                if r < reps[name]:
                    runs[name].append(timed(call))
                    if name.startswith("bm25"):
                        s = ix.query_bm25_stats()
                        s["skip_rate"] = s["skipped"] / max(s["windows"], 1)
                        row[name + "_stats"] = s
        for name in legs:
            row[name + "_ms"] = statistics.median(runs[name])
            row[name + "_runs_ms"] = runs[name]
            row[name + "_warmup_ms"] = warm[name]
        row["ratio"] = row["bm25_ms"] / row["topk_stream_ms"]
        if i == 0:
            row["split1_over_auto"] = row["bm25_split1_ms"] / row["bm25_ms"]
        out["batches"][str(nq)] = row
        print(json.dumps({str(nq): row}), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (after every batch: a long later batch loses nothing)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
