"""The gathering passes of term_sort (csrc/sme_sort.hip: gather_fill /
gather_addr) at the record layouts their addressing makes special.  A wave finds
the record of each of its 1024 items from a mask of the record starts among them
and a table of the records that own those starts; a wave with more starts than
the table holds, or with a run of empty records longer than one table fill
reads, walks the rest.  Nothing here knows the table's size: the number of
records that start in one wave is swept from 1 to 1024, with the wave's first
item inside a record and on a record's first pair.

Every case runs in the packed form (tests/native/prims_packed.hip: base values
that differ per record, the tf field filled to its top, so a wrong record shows
in docno as well as in the order) and in the two-array form
(tests/native/prims_harness.hip), each with one pass (gathering and last), two
passes and four, and is held bit for bit to numpy's stable sort.  Regions have
gaps, are not in ascending address order and lie in junk; the harness guards
and fills every buffer."""
import numpy as np
import pytest

from test_gpu_prims import TILE, check_term_sort, gather_layout, term_case
from test_gpu_term_sort_packed import PASSES, check_packed, small_records

pytestmark = pytest.mark.gpu

WAVE = 1024
# (bits, maxbits, F, dmin) of the two-array form: one, two and four passes, as
# test_term_sort_gather
PASSES2 = ((11, 11, 1000, 0), (13, 11, 65537, 2_000_000_000), (22, 6, 1000, 17))


def check_both(rng, cnt):
    cnt = [int(c) for c in cnt]
    P = sum(cnt)
    for bits, maxbits, F, dmin in PASSES:
        check_packed(rng, cnt, bits, maxbits, F, dmin, with_w=False)
    for bits, maxbits, F, dmin in PASSES2:
        keys, vals = term_case(rng, P, bits, garbage=bits == 13)
        check_term_sort(keys, vals, bits, maxbits, dmin, F, src=gather_layout(rng, cnt, keys, vals))


def cut(rng, n, r):
    """n items cut into r records of at least one pair"""
    at = np.sort(rng.choice(np.arange(1, n), r - 1, replace=False)) if r > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], at, [n]])).tolist()


STARTS = [1, 2, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024]


@pytest.mark.parametrize("r", STARTS)
def test_starts_per_wave(r):
    """1024 items cut into r records: after a record of 300 pairs, so the wave's
    first item lies inside a record, and from a wave's first item, a record start
    on bit 0 of its mask; a record of 2000 follows"""
    rng = np.random.default_rng(11000 + r)
    check_both(rng, [300] + cut(rng, WAVE, r) + [2000])
    check_both(rng, [WAVE] + cut(rng, WAVE, r) + [2000])


def test_wave_and_tile_edges():
    rng = np.random.default_rng(11100)
    check_both(rng, [1023, 1, 1024, 1, 1023, 8191, 1, 8192, 8193])
    # records that start on the last item of a wave (1023) and of a tile (8191)
    check_both(rng, [1023, 5, TILE - 1 - 1028, 7, 100])


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193])
def test_sizes(P):
    rng = np.random.default_rng(11200 + P)
    check_both(rng, [P])
    check_both(rng, small_records(rng, P))


def test_no_start_in_a_wave():
    """one record over three tiles and five pairs: 24 waves without a start"""
    rng = np.random.default_rng(11300)
    check_both(rng, [3 * TILE + 5] + small_records(rng, 900))


@pytest.mark.parametrize("E", [70, 1100])
def test_empty_runs(E):
    """runs of records without pairs, the longer one longer than a wave's items: at
    the very start, between two records that meet on a wave edge and on a tile
    edge, inside a wave, and at the very end"""
    rng = np.random.default_rng(11400 + E)
    Z = [0] * E
    check_both(rng, Z + [700, 1500, 3])
    check_both(rng, [WAVE] + Z + [1500, 3])
    check_both(rng, [TILE] + Z + [1500, 3])
    check_both(rng, [700] + Z + [1500, 3] + Z + [40])
    check_both(rng, [700, 1500] + Z)
    check_both(rng, Z + [900])  # all records empty but the last


def test_alternating_empty_records():
    """empty and one-pair records in turn across a whole wave and more"""
    rng = np.random.default_rng(11500)
    check_both(rng, [0, 1] * WAVE)
    check_both(rng, [300] + [0, 1] * 1100 + [50])


@pytest.mark.parametrize("r", [49, 513])
def test_starts_per_wave_docid_slots(r):
    """K6b (xw, Pout) over the start sweep: 11-bit words in one, two and four passes"""
    rng = np.random.default_rng(11600 + r)
    W, bits, F = 1 << 11, 11, 65537
    for cnt in ([300] + cut(rng, WAVE, r) + [2000], [WAVE] + cut(rng, WAVE, r) + [2000]):
        P = sum(cnt)
        for maxbits in (11, 6, 3):
            check_packed(rng, cnt, bits, maxbits, F, 5, W=W)
            keys = rng.integers(0, W, P, dtype=np.uint32)
            vals = rng.integers(0, 1 << 32, P, dtype=np.uint32)
            ins = rng.integers(0, 4, W) * (rng.random(W) < 0.3)
            xw = np.empty((W, 2), np.uint32)
            xw[:, 0] = np.cumsum(ins)
            xw[:, 1] = rng.integers(0, 0xFFFFFFFF, W, dtype=np.uint32)
            Pout = P + int(xw[-1, 0]) + 3
            check_term_sort(keys, vals, bits, maxbits, 5, F, lut=1.0 + rng.random(F), idf=2.5,
                            src=gather_layout(rng, cnt, keys, vals), xw=xw, Pout=Pout)
