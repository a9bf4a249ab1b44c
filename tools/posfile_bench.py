#!/usr/bin/env python3
"""Time the positions file at c2 size (1 M documents, "positions" 1).

One index of --docs documents built with positions writes its file in HBM
(sme_index_positions_file_device); an index of the same corpus built without the
option attaches it from there (sme_index_attach_positions_device), with the
cross-check.  Reported, each the median of --reps calls after one warm-up call, with
the smallest and largest:

  encode_ms, decode_ms, crosscheck_ms   sme_index_posfile_stats' device times
  digest_ms, records_ms                 the stages of the attach's profile beside them
  write_wall_ms, attach_wall_ms         host wall time of the whole call

and two yardsticks from the same process: floor_ms, the bytes each kernel must move
at the rate sme_hbm_copy_bench gives (encode: 4 B per position read, bits / 8 B
written; decode the other way round; cross-check: ids and counters, see
crosscheck_bytes), and the build's own "positions" stage and total.

Writes profiles/posfile_c2.json.  A report: no figure here is a pass/fail bound.

    python tools/posfile_bench.py [--docs 1000000] [--vocab 1048576] [--reps 5] [--bits 0]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "simple-mapreduce-search-engine-information-retrieval-_amd"


def spread(runs):
    return {"ms": statistics.median(runs), "min_ms": min(runs), "max_ms": max(runs), "runs_ms": runs}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--docs", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=1 << 20)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--bits", type=int, default=0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "posfile_c2.json"))
    a = p.parse_args()

    import torch
    torch.cuda.init()
    sme = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    L = sme.lib()
    cal = C.c_double(0.0)
    copy_gbps = cal.value if L.sme_hbm_copy_bench(0, 4 << 30, 10, C.byref(cal)) == 0 else None
    mapping = synth.mapping_bytes(a.docs)

    def ctx_of(positions):
        ctx = sme.Context(1, 10)
        ctx.load_docno_mapping(mapping)
        ctx.set_option("positions", positions)
        return ctx

    corpus = sme.DeviceCorpus(a.docs, V=a.vocab, seed=42, len_lo=400, len_hi=600, d0=0)
    with_ctx, plain_ctx = ctx_of(1), ctx_of(0)
    with_ctx.build_device(corpus.ptr, corpus.nbytes).close()  # warm-up: the workspace is allocated
    whole = with_ctx.build_device(corpus.ptr, corpus.nbytes)
    build_prof = with_ctx.last_build_profile()
    records, T, stream_bytes = whole.positions()

    enc, wall_w = [], []
    for i in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ptr, nbytes = whole.positions_file_device(a.bits)
        if i:
            wall_w.append((time.perf_counter() - t0) * 1e3)
            enc.append(whole.posfile_stats()["encode_ms"])
    bits = whole.posfile_stats()["bits"]

    dec, cross, dig, rec, wall_a, checked = [], [], [], [], [], 0
    for i in range(a.reps + 1):
        plain = plain_ctx.build_device(corpus.ptr, corpus.nbytes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.attach_positions_device(ptr, nbytes)
        ms = (time.perf_counter() - t0) * 1e3
        st, prof = plain.posfile_stats(), plain_ctx.last_build_profile()
        assert plain.positions() == whole.positions()
        checked = st["checked_postings"]
        if i:
            wall_a.append(ms)
            dec.append(st["decode_ms"])
            cross.append(st["crosscheck_ms"])
            dig.append(prof["digest"])
            rec.append(prof["records"])
        plain.close()

    P = whole.P
    word_bytes = (T * bits + 63) // 64 * 8
    moved = {"encode_bytes": 4 * T + word_bytes, "decode_bytes": word_bytes + 4 * T,
             # ids and the records' tables read, the counters zeroed, added to (read and written) and read
             # again beside the tfs, one docno probed per position at least
             "crosscheck_bytes": 4 * T + 12 * records + 4 * P + 8 * P + 8 * P + 4 * T}

    def floor(nbytes_):
        return nbytes_ / (copy_gbps * 1e9) * 1e3 if copy_gbps else None

    out = {"config": {"docs": a.docs, "vocab": a.vocab, "reps": a.reps, "bits_asked": a.bits},
           "hbm_copy_GBps": copy_gbps,
           "input": {"N": whole.N, "V": whole.V, "P": P, "records": records, "positions": T,
                     "stream_bytes": stream_bytes},
           "file": {"bytes": nbytes, "bits": bits, "checked_postings": checked},
           "what": ("ms: median of the reps after one warm-up call (min_ms / max_ms: smallest and largest); encode, "
                    "decode, crosscheck: sme_index_posfile_stats; digest, records: the attach's profile; *_wall: host "
                    "wall time of the call; floor_ms: *_bytes at hbm_copy_GBps; build: the profile of the "
                    "\"positions\" 1 build of the same corpus in the same process"),
           "encode": {**spread(enc), "floor_ms": floor(moved["encode_bytes"])},
           "decode": {**spread(dec), "floor_ms": floor(moved["decode_bytes"])},
           "crosscheck": {**spread(cross), "floor_ms": floor(moved["crosscheck_bytes"])},
           "digest": spread(dig), "records": spread(rec),
           "write_wall": spread(wall_w), "attach_wall": spread(wall_a),
           "moved": moved,
           "build": {"positions_ms": build_prof.get("positions"), "total_ms": build_prof.get("total")}}
    for k in ("encode", "decode", "crosscheck"):
        if out[k]["floor_ms"]:
            out[k]["ratio_to_copy_rate"] = out[k]["ms"] / out[k]["floor_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("hbm_copy_GBps", "input", "file", "encode", "decode", "crosscheck", "digest",
                                          "records", "write_wall", "attach_wall", "build")}))


if __name__ == "__main__":
    main()
