"""The passages header's host check (tools/passage_check.cc, built with the address and
undefined-behaviour sanitizers by `make passage-check`) as a test: its own cases -- valid
batches, every malformed one, every truncation, the limits, the slot normaliser and the
one-record best window against hand-worked windows and a second count.  Stand-alone host
program only; skips where no host C++ compiler is found."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-mapreduce-search-engine-information-retrieval-_amd")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("passage") / "passage_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tools", "passage_check.cc"), "-o", exe])
    return exe


def test_builtin_cases(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_makefile_has_the_target():
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "\npassage-check: build/passage_check\n" in mk
    phony = [ln for ln in mk.split("\n") if ln.startswith(".PHONY:")]
    assert len(phony) == 1 and "passage-check" in phony[0].split()
    assert "csrc/sme_passage.hip" in [ln for ln in mk.split("\n") if ln.startswith("SRC =")][0].split()


def test_the_header_needs_no_device():
    """The checked header is plain C++: it includes nothing of HIP."""
    src = open(os.path.join(PKG, "csrc", "sme_passage.hpp")).read()
    assert "#include <hip" not in src and "__device__" not in src
