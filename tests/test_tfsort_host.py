"""The tf-desc segment sort's test wrapper (tests/native/prims_tfsort.hip) is in
libsme_prims.so and nowhere in the product; its host-only entry answers (no
device calls here)."""
import ctypes
import os
import re

import prims_lib as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tfsort_symbols():
    src = open(os.path.join(ROOT, "tests", "native", "prims_tfsort.hip")).read()
    return sorted(set(re.findall(r"^SMEP_API [^(]*?\b(smep_[a-z0-9_]+)\(", src, flags=re.M)))


def test_tfsort_wrapper_is_exported():
    syms = tfsort_symbols()
    assert "smep_tf_sort_segments" in syms and "smep_tfsort_last_error" in syms
    L = ctypes.CDLL(PL.LIB_PATH)
    for s in syms:
        assert hasattr(L, s), s
    L.smep_tfsort_max_tf.restype = ctypes.c_int
    assert L.smep_tfsort_max_tf() == 1023


def test_tfsort_wrapper_is_not_in_the_product(sme):
    L = sme.lib()
    for s in tfsort_symbols():
        assert not hasattr(L, s), s
        assert s not in sme.EXPORTS
