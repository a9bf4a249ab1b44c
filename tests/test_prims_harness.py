"""The primitive test harness (libsme_prims.so) loads without a GPU and exports
every wrapper the loader declares; its host-only entry points answer (no device
calls here)."""
import ctypes
import os
import re

import prims_lib as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def harness_symbols():
    src = open(os.path.join(ROOT, "tests", "native", "prims_harness.hip")).read()
    return sorted(set(re.findall(r"^SMEP_API [^(]*?\b(smep_[a-z0-9_]+)\(", src, flags=re.M)))


def test_harness_exports_all():
    L = ctypes.CDLL(PL.LIB_PATH)
    assert set(harness_symbols()) == set(PL.WRAPPERS)  # the loader declares what the source exports
    for s in PL.WRAPPERS:
        assert hasattr(L, s), s
    for must in ("smep_term_sort", "smep_kv_sort", "smep_sort_pairs", "smep_sort_pairs_v64", "smep_excl_scan",
                 "smep_select_flagged", "smep_reduce_max", "smep_reduce_by_key_sum"):
        assert must in PL.WRAPPERS


def test_harness_is_not_in_the_product(sme):
    L = sme.lib()
    for s in PL.WRAPPERS:
        assert not hasattr(L, s), s
        assert s not in sme.EXPORTS


def test_scratch_sizes_and_guard():
    """the documented scratch: 2048 u32 per 8192-item tile, 2048 * 1024 group sums
    and 1024 scan sums; the term sort adds one int64 per 1024 pairs and one"""
    L = PL.lib()
    assert L.smep_guard_elems() >= 256
    assert L.smep_fill_byte() == PL.FILL_BYTE
    fixed = 2048 * 1024 + 1024
    for n in (0, 1, 8192, 8193, 4097 * 8192, (1 << 32) - 1):
        tiles = max(1, -(-n // 8192))
        assert PL.kv_sort_scratch(n) == 4 * (tiles * 2048 + fixed)
        assert PL.term_sort_scratch(n) == 4 * (tiles * 2048 + fixed) + 8 * (-(-max(n, 1) // 1024) + 1)
