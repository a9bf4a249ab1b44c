"""The record parser's host check (tools/recparse_check.cc, built with the address
and undefined-behaviour sanitizers by `make recparse-check`) as a test: its own
cases, then the very streams test_gpu_load.py sends to the device.  Skips where
no host C++ compiler is found."""
import os
import shutil
import struct
import subprocess

import pytest

import load_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-mapreduce-search-engine-information-retrieval-_amd")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = os.environ.get("HOSTCXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("recparse") / "recparse_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tools", "recparse_check.cc"),
                           "-o", exe])
    return exe


def test_builtin_cases(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_loader_test_streams(checker, tmp_path):
    cases = [("valid", S.VALID, S.RP_OK, 0)] + S.refused()
    for name, parts, code, _ in cases:
        offs = [0]
        for p in parts:
            offs.append(offs[-1] + len(p))
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(parts)) + struct.pack("<%dQ" % len(offs), *offs) + b"".join(parts))
        r = subprocess.run([checker, "--file", path, "--expect", str(code)], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout + r.stderr)
