"""bench.py's launch contract: `--gpus N` must run N ranks and say so.

The driver runs `bench.py --gpus N` either under torch.distributed.run (WORLD_SIZE
set) or directly; directly, bench.py starts the N rank processes itself.  The
world size the ranks agree on must equal --gpus, so an N-GPU line cannot
silently measure one GPU.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_gpus_mismatch_refused():
    """WORLD_SIZE from a launcher that disagrees with --gpus: refused before any
    GPU work (no torch import on this path)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--gpus 2 but WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_steps_must_be_positive():
    """--steps sets the number of timed steps; none is refused by the parser."""
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_index(sme, synth, tmp_path):
    """A plain run prints the headline line only (no query / checks / CPU legs,
    which need --full) with the steps it was given, and --dump-outputs writes the
    index of the last timed step: float64 arrays equal to an index built here
    from the same corpus (2,000 docs: every array is below the sample size, so
    it is dumped whole)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    cmd = [sys.executable, BENCH, "--gpus", "1", "--docs", "2000", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    d = json.loads(line[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["unit"] == "GB/s" and d["higher_is_better"] is True
    for key in ("query", "checks", "cpu_baseline", "c1_sample", "value_true_df", "value_with_records",
                "value_query_ready", "end_to_end_ms", "hbm_copy_GBps"):
        assert key not in d, key
    c = bench_config("c2")
    corpus = sme.DeviceCorpus(2000, V=c["vocab"], seed=c["seed"], len_lo=c["lo"], len_hi=c["hi"])
    ctx = sme.Context(1, 1, 0)
    ctx.load_docno_mapping(synth.mapping_bytes(2000))
    ix = ctx.build_device(corpus.ptr, corpus.nbytes)
    corpus.close()
    off, dn, tf, _ = ix.csr()
    _, wd, w = ix.weights()
    want = {"stats": np.array([ix.N, ix.V, ix.P]), "offsets": off, "docno": dn, "tf": tf, "weight_docno": wd,
            "weight": w}
    ix.close()
    ctx.close()
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    assert (d["config"]["N"], d["config"]["V"], d["config"]["P"]) == tuple(int(x) for x in want["stats"])
    for name, arr in want.items():
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == arr.shape, name
        assert np.array_equal(got, arr.astype(np.float64)), name


def bench_config(name):
    """bench.py's CONFIGS[name], read without running the benchmark."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("sme_bench", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.CONFIGS[name]


@pytest.mark.gpu
def test_gpus2_rehearsal_spawns_two_ranks():
    """`bench.py --gpus 2` with no launcher, rehearsed on one GPU
    (SME_BENCH_REHEARSE=1: two ranks share the device, gloo collectives): the
    line says n_gpus 2 and every full-size check of the sharded run holds."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["SME_BENCH_REHEARSE"] = "1"
    cmd = [sys.executable, BENCH, "--gpus", "2", "--full", "--docs", "2000", "--queries", "200", "--steps", "1",
           "--warmup", "1", "--cpu-docs", "0", "--no-e2e"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and "rehearsal" in d
    assert d["config"]["docs_this_gpu"] == 2000
    assert d["query"]["queries"] == 200
    bad = [k for k, v in d["checks"].items() if v is False]
    assert not bad, bad
