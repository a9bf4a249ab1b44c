"""The chunk kernel of csrc/sme_chunks.hpp where a workgroup takes more than one
chunk: its grid-stride loop and the restaging of LDS between chunks.  Wildcard,
fuzzy and Boolean launch one workgroup per chunk up to 2^20 chunks, so their
tests never get there; here the grid is 1, 2 or NC workgroups, through
libsme_prims.so (tests/native/prims_chunks.hip) with the guard discipline of the
other primitive tests.  The Op: the candidates are the integers 0, 1, 2 ... cut
into ranges, a range's modulus is staged in LDS (0 rejects its chunks), a hit is
value % modulus == 0, the value is emitted.  Every range has another modulus, so
a chunk filtered with stale staged data gives other numbers.  Match counts per
chunk, their offsets and the emitted values equal a numpy restatement exactly."""
import ctypes as C

import numpy as np
import pytest

import prims_lib as PL

pytestmark = pytest.mark.gpu

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
GUARDS = ("moff", "values")

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(PL.LIB_PATH)
        L.smep_chunks_last_error.restype, L.smep_chunks_last_error.argtypes = C.c_char_p, []
        L.smep_chunks_filter.restype = _int
        L.smep_chunks_filter.argtypes = [_vp, _vp, _i64, _int, _i64, _vp, _vp, _i64, _vp, C.POINTER(C.c_int)]
        _lib = L
    return _lib


def chunks_filter(rcnt, mod, chunk, grid, NC, cap):
    """-> (moff[NC + 1], the emitted values, total)"""
    rcnt, mod = PL._c(rcnt, np.int32), PL._c(mod, np.int32)
    moff, vals, total = np.empty(NC + 1, np.int64), np.full(cap, -1, np.int32), np.zeros(1, np.int64)
    guard = C.c_int(0)
    rc = lib().smep_chunks_filter(PL._p(rcnt), PL._p(mod), len(rcnt), chunk, grid, PL._p(moff), PL._p(vals), cap,
                                  PL._p(total), C.byref(guard))
    if rc != 0:
        msg = lib().smep_chunks_last_error().decode()
        if rc == -2:  # SME_EHIP: the device context may be lost, so nothing more is started on it
            pytest.exit("HIP error in the primitive harness: " + msg, returncode=3)
        raise PL.PrimsError(rc, msg)
    if guard.value:
        raise PL.GuardError("changed: " + ", ".join(n for i, n in enumerate(GUARDS) if guard.value >> i & 1))
    return moff, vals, int(total[0])


def reference(rcnt, mod, chunk):
    """-> (matches of every chunk in chunk order, all matches in emit order)"""
    counts, vals, base = [], [], 0
    for n, m in zip(rcnt, mod):
        for c0 in range(0, n, chunk):
            v = np.arange(base + c0, base + min(c0 + chunk, n), dtype=np.int64)
            hits = v[v % m == 0] if m else v[:0]
            counts.append(len(hits))
            vals.append(hits)
        base += n
    return np.array(counts, np.int64), np.concatenate(vals + [np.zeros(0, np.int64)]).astype(np.int32)


# one modulus per range; 257 candidates that all match; in "reject", two ranges whose chunks stage() rejects
MODULI = {"distinct": [13, 2, 3, 5, 7, 4, 6, 1, 9, 10, 11, 8], "reject": [13, 2, 3, 0, 7, 4, 6, 1, 9, 0, 11, 8]}


@pytest.mark.parametrize("moduli", sorted(MODULI))
@pytest.mark.parametrize("chunk", [64, 128])
def test_grid_stride_and_restaging(chunk, moduli):
    rcnt = [0, 1, 63, 64, 65, 255, 256, 257, chunk, chunk + 1, 0, 3 * chunk]
    mod = MODULI[moduli]
    counts, want = reference(rcnt, mod, chunk)
    NC = len(counts)
    assert NC == sum(-(-n // chunk) for n in rcnt) and NC > 2
    want_moff = np.concatenate([[0], np.cumsum(counts)])
    for grid in (1, 2, NC):
        moff, vals, total = chunks_filter(rcnt, mod, chunk, grid, NC, len(want) + 64)
        print("chunk %d grid %d: NC %d total %d (want %d)" % (chunk, grid, NC, total, len(want)))
        assert np.array_equal(moff, want_moff), grid
        assert total == len(want), grid
        assert np.array_equal(vals[:total], want), grid
        assert (vals[total:] == -1).all(), grid
