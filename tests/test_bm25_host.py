"""The BM25 header's host check (tools/bm25_check.cc, built with the address and
undefined-behaviour sanitizers by `make bm25-check`) as a test: its own cases -- valid
batches, every malformed one, every truncation, the limits, the parameter rule -- and
the bits of the weight and the bound of csrc/sme_bm25.hpp, the functions the kernels
call, held to bm25_ref's.  Stand-alone host program only.  Skips where no host C++
compiler is found."""
import itertools
import os
import shutil
import subprocess

import pytest

import bm25_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-mapreduce-search-engine-information-retrieval-_amd")

D = 1000
K1, B = (0.0, 0.9, 1.2, 2.0), (0.0, 0.75, 1.0)
TF = (1, 2, 1023, 1 << 24)
AVGDL = (100.0, 7.0 / 3.0)
DL = (1, 2, 80, 100, 2500)  # below and above both averages
DF = (1, D // 2, D)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("bm25") / "bm25_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tools", "bm25_check.cc"), "-o", exe])
    return exe


def test_builtin_cases(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


@pytest.fixture(scope="module")
def grid(checker):
    """{(k1, b, tf, dl, avgdl, df): (idf, norm, weight, bound) bits from the header}."""
    tuples = list(itertools.product(K1, B, TF, DL, AVGDL, DF))
    args = ["%016x,%016x,%d,%d,%016x,%d,%d" % (R.bits(k1), R.bits(b), tf, dl, R.bits(avg), df, D)
            for k1, b, tf, dl, avg, df in tuples]
    r = subprocess.run([checker, "--weight"] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(tuples)
    return {t: tuple(int(x, 16) for x in ln.split()) for t, ln in zip(tuples, lines)}


def test_weight_bits_equal_the_restatement(grid):
    for (k1, b, tf, dl, avg, df), got in grid.items():
        idf = R.idf_value(D, df)
        norm = R.doc_norm(k1, b, dl, avg)
        want = (R.bits(idf), R.bits(norm), R.bits(R.weight(idf, tf, k1, norm)),
                R.bits(R.bound_term(idf, tf, k1, b, dl, avg)))
        assert got == want, (k1, b, tf, dl, avg, df)


def test_bound_covers_its_weights(grid):
    """The bound term at (largest tf, shortest document) is no less than the weight of
    any posting with a tf no larger in a document no shorter."""
    import numpy as np
    val = {t: float(np.uint64(g[2]).view(np.float64)) for t, g in grid.items()}
    bound = {t: float(np.uint64(g[3]).view(np.float64)) for t, g in grid.items()}
    for k1, b, avg, df in itertools.product(K1, B, AVGDL, DF):
        for maxtf, mindl in itertools.product(TF, DL):
            top = bound[(k1, b, maxtf, mindl, avg, df)]
            for tf, dl in itertools.product(TF, DL):
                if tf <= maxtf and dl >= mindl:
                    assert val[(k1, b, tf, dl, avg, df)] <= top, (k1, b, maxtf, mindl, tf, dl)
