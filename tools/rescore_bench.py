#!/usr/bin/env python3
"""Time scoring given documents (sme_query_rescore_device) at c2 size: the order 0
device result of a Boolean batch, rescored under BM25 over the batch's own terms with
"rescore_path" 0 (automatic), 1 (always search) and 2 (always scan).

  or_large    `--or-queries` queries of one OR group of 2-8 terms drawn proportional
              to df: large results
  and_small   `--and-queries` queries of two single-term groups drawn likewise:
              small results

Legs of a batch, alternating, every figure the median of `--reps` host wall times of
one call ending in a device synchronize, after a warm-up call of each:

  boolean_order0      the sme_query_boolean_device call (order 0, m 0) that produces
                      the candidates
  boolean_ranked      the same call with order 1, m = k: the one way to rank those
                      documents without this feature (by the Boolean TF-IDF sum)
  topk_bm25           sme_query_topk_bm25_device over the same term lists, k = k: the
                      one way to rank those terms by BM25 without it (whole collection)
  rescore_path0/1/2   sme_query_rescore_device, model BM25, order 1, m = k, min_hits 0
  rescore_path0_again the automatic leg a second time: what repeating one
                      configuration moves the median by

spread_ms of a leg is max - min of its runs.  The three paths must return the same
arrays.  Writes profiles/rescore_c2.json.  A report: the one comparison drawn is
automatic against the faster forced path, beside the spread.

    python tools/rescore_bench.py [--docs 1000000] [--vocab 1048576] [--or-queries 256]
                                  [--and-queries 100000] [--reps 5]

Kernel time comes from a run of its own under the profiler, one batch and path per run:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
        python tools/rescore_bench.py --profile-run or_large:2
    python tools/rescore_bench.py --kernel-stats or_large:2=DIR/.../run_kernel_stats.csv [...]

The second command needs no device: it adds k_rs_score's times to the JSON.
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
OUT = os.path.join(ROOT, "profiles", "rescore_c2.json")
K, K1, B = 10, 1.2, 0.75


def add_kernel_stats(path, pairs):
    with open(path) as f:
        out = json.load(f)
    for pair in pairs:
        name, csv_path = pair.split("=", 1)
        batch, leg = name.split(":")
        with open(csv_path, newline="") as f:
            hit = [r for r in csv.DictReader(f) if "k_rs_score" in r["Name"]]
        assert len(hit) == 1, csv_path
        k = {"calls": int(hit[0]["Calls"]), "avg_ms": float(hit[0]["AverageNs"]) / 1e6,
             "min_ms": float(hit[0]["MinNs"]) / 1e6, "max_ms": float(hit[0]["MaxNs"]) / 1e6}
        out["batches"][batch].setdefault("score_kernel", {})["path" + leg] = k
        print(name, k)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def make_batches(ix, synth, n_or, n_and, seed):
    df = np.diff(ix.offsets())
    terms, qoff = synth.queries_by_df(df, n_or, seed=seed, qlen_lo=2, qlen_hi=8)
    or_large = [[([int(t) for t in terms[qoff[q]:qoff[q + 1]]], False)] for q in range(n_or)]
    two, _ = synth.queries_by_df(df, n_and, seed=seed + 2, qlen_lo=2, qlen_hi=2)
    and_small = [[([int(two[2 * q])], False), ([int(two[2 * q + 1])], False)] for q in range(n_and)]
    return {"or_large": or_large, "and_small": and_small}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--or-queries", type=int, default=256)
    p.add_argument("--and-queries", type=int, default=100_000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--profile-run", default=None, metavar="BATCH:PATH", help="only that leg's rescore calls, untimed")
    p.add_argument("--kernel-stats", nargs="*", default=None, metavar="BATCH:PATH=CSV")
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
    batches = make_batches(ix, synth, a.or_queries, a.and_queries, 1)
    out = {"config": {"docs": a.docs, "vocab": a.vocab, "k": K, "k1": K1, "b": B, "reps": a.reps},
           "index": {"N": ix.N, "V": ix.V, "P": ix.P}, "prepare_bm25_ms": prepare_ms,
           "what": "*_ms: median host wall time of one call ending in a device synchronize, the legs alternating; "
                   "*_spread_ms: max - min of the leg's runs; candidates / found / matches: sme_query_rescore_stats; "
                   "auto_over_best: rescore_path0_ms / min(rescore_path1_ms, rescore_path2_ms); "
                   "repeat_over_first: rescore_path0_again_ms / rescore_path0_ms",
           "batches": {}}
    print("index N %d V %d P %d" % (ix.N, ix.V, ix.P), flush=True)

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, queries in batches.items():
        if a.profile_run and a.profile_run.split(":")[0] != name:
            continue
        nq = len(queries)
        arrays = sme.Index.boolean_arrays(queries)
        slots = [t for groups in queries for ids, _ in groups for t in ids]
        qoff = np.zeros(nq + 1, np.int64)
        qoff[1:] = np.cumsum([sum(len(ids) for ids, _ in groups) for groups in queries])
        ids = np.array(slots, np.int32)
        d_t, d_q = torch.from_numpy(ids).cuda(), torch.from_numpy(qoff).cuda()
        od = torch.empty(nq * K, dtype=torch.int32, device="cuda")
        os_ = torch.empty(nq * K, dtype=torch.float64, device="cuda")

        def boolean0():
            return ix.query_boolean_device(None, 0, 0, arrays=arrays)

        # the candidates in tensors of the bench's own: the Boolean legs below reuse the index's buffers
        c_off, c_dn, _, c_total = boolean0()
        d_coff = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
        d_cdn = torch.empty(max(c_total, 1), dtype=torch.int32, device="cuda")
        sme.memcpy(d_coff.data_ptr(), c_off, 8 * (nq + 1))
        sme.memcpy(d_cdn.data_ptr(), c_dn, 4 * c_total)
        # a device-to-device copy may return before it is done: a copy to the host behind it does not
        last = np.zeros(1, np.int64)
        sme.memcpy(last.ctypes.data, d_coff.data_ptr() + 8 * nq, 8)
        assert int(last[0]) == c_total
        if c_total:
            sme.memcpy(last.ctypes.data, d_cdn.data_ptr() + 4 * (c_total - 1), 4)

        def rescore(path):
            ctx.set_option("rescore_path", path)
            r = ix.rescore_device(ids, qoff, d_cdn, d_coff, model="bm25", order=1, m=K, min_hits=0, k1=K1, b=B)
            ctx.set_option("rescore_path", 0)
            return r

        if a.profile_run:
            for _ in range(a.reps + 1):
                rescore(int(a.profile_run.split(":")[1]))
            torch.cuda.synchronize()
            continue
        legs = {
            "boolean_order0": boolean0,
            "boolean_ranked": lambda: ix.query_boolean_device(None, 1, K, arrays=arrays),
            "topk_bm25": lambda: ix.query_bm25_device(d_t.data_ptr(), d_q.data_ptr(), nq, K, od.data_ptr(),
                                                      os_.data_ptr(), K1, B),
            "rescore_path0": lambda: rescore(0), "rescore_path1": lambda: rescore(1),
            "rescore_path2": lambda: rescore(2), "rescore_path0_again": lambda: rescore(0),
        }
        row = {"queries": nq, "slots": int(len(ids))}
        same = []
        for path in (0, 1, 2):  # the arrays to compare (also a warm-up)
            r = rescore(path)
            cols = [np.zeros(nq + 1, np.int64)] + [np.zeros(max(r[4], 1), dt) for dt in (np.int32, np.int32, np.float64)]
            for c, ptr, cnt in zip(cols, r[:4], (nq + 1, r[4], r[4], r[4])):
                if cnt:
                    sme.memcpy(c.ctypes.data, ptr, c[:cnt].nbytes)
            same.append(b"".join(c.tobytes() for c in cols))
        row.update(ix.rescore_stats())
        row["paths_identical"] = same[0] == same[1] == same[2]
        warm = {leg: timed(call) for leg, call in legs.items()}
        runs = {leg: [] for leg in legs}
        reps = {leg: max(1, min(a.reps, int(60e3 / max(w, 1e-3)))) for leg, w in warm.items()}  # (a leg of minutes: fewer)
        for r in range(a.reps):
            for leg, call in legs.items():
                if r < reps[leg]:
                    runs[leg].append(timed(call))
        for leg in legs:
            row[leg + "_ms"] = statistics.median(runs[leg])
            row[leg + "_runs_ms"] = runs[leg]
            row[leg + "_spread_ms"] = max(runs[leg]) - min(runs[leg])
        row["auto_over_best"] = row["rescore_path0_ms"] / min(row["rescore_path1_ms"], row["rescore_path2_ms"])
        row["repeat_over_first"] = row["rescore_path0_again_ms"] / row["rescore_path0_ms"]
        out["batches"][name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if not k.endswith("_runs_ms")}}), flush=True)
        assert row["paths_identical"], name + ": the paths disagree"
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (after every batch: a long later batch loses nothing)
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
