"""The device sort, scan and compaction primitives of csrc/sme_sort.hip, each
against numpy, bit-exact, at the sizes their own constants make special: the
8192-item sort tile, 1024 items per wave, the 4096-item scan tile, the
48-record gather table, the 32768-sum switch of the (digit, group) scan and the
4096-tile switch of the tile groups.  They run through libsme_prims.so
(tests/native/prims_harness.hip linked with the product's build/sme_sort.o):
every buffer a primitive writes is followed by guard elements, sort scratch is
exactly term_sort_scratch / kv_sort_scratch bytes, and a changed guard fails the
call (prims_lib.GuardError).  References: np.argsort(kind="stable") on the
masked key, np.cumsum in the same dtype, np.flatnonzero, np.maximum.reduce,
np.add.reduceat.  No tolerance anywhere."""
import time

import numpy as np
import pytest

import prims_lib as PL

pytestmark = pytest.mark.gpu

TILE = 8192
SMALL = [1, 2, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193]
TILES = [t * TILE + d for t in (7, 8, 9, 17) for d in (0, 1)]
SIZES = SMALL + TILES
BITS = {4: [1, 6, 11, 12, 22, 23, 32], 8: [33, 44, 63, 64]}
KEY_DT = {4: np.uint32, 8: np.uint64}


def _npass(bits, key_bytes, maxbits=11):
    return (min(max(bits, 1), 8 * key_bytes) + maxbits - 1) // maxbits


def _mask(bits, dt):
    return dt((1 << bits) - 1)


def make_keys(rng, n, bits, dt, dist, garbage=True):
    """n keys whose low `bits` bits follow `dist`; random bits above them"""
    width = 8 * np.dtype(dt).itemsize
    hi = 1 << bits
    if dist == "uniform":
        k = rng.integers(0, hi, n, dtype=np.uint64)
    elif dist == "equal":
        k = np.full(n, rng.integers(0, hi, dtype=np.uint64), np.uint64)
    elif dist == "two":
        k = np.where(np.arange(n) & 1, np.uint64(hi - 1), np.uint64(hi >> 1))
    elif dist == "sorted":
        k = np.sort(rng.integers(0, hi, n, dtype=np.uint64))
    elif dist == "reverse":
        k = np.sort(rng.integers(0, hi, n, dtype=np.uint64))[::-1].copy()
    elif dist == "zipf":
        k = np.minimum(rng.zipf(1.3, n), min(hi, 1 << 62)).astype(np.uint64) - np.uint64(1)
    else:
        raise ValueError(dist)
    if garbage and bits < width:
        k = k | (rng.integers(0, 1 << (width - bits), n, dtype=np.uint64) << np.uint64(bits))
    return k.astype(dt)


def stable_perm(keys, bits):
    dt = keys.dtype.type
    width = 8 * keys.dtype.itemsize
    masked = keys if bits >= width else keys & _mask(bits, dt)
    if bits <= 16:
        masked = masked.astype(np.uint16)  # numpy's stable sort of 16-bit keys is a radix sort
    return np.argsort(masked, kind="stable")


def check_kv_sort(keys, bits, perm):
    n = len(keys)
    kb = keys.dtype.itemsize
    iota = np.arange(n, dtype=np.uint32)
    want = 0 if n <= 1 else _npass(bits, kb) % 2
    for keys_out in (False, True):
        ok, ov, which = PL.kv_sort(keys, iota, bits, keys_out)
        # contract: ping-pong from (k0, v0); an even pass count ends in the input pair
        assert which == want, (n, bits, keys_out, which)
        assert np.array_equal(ov, perm), (n, bits, keys_out)
        if keys_out or n <= 1:
            assert np.array_equal(ok, keys[perm]), (n, bits)  # whole keys, bits above `bits` included


def check_sort_pairs(keys, bits, perm):
    ok, ov = PL.sort_pairs(keys, np.arange(len(keys), dtype=np.uint32), bits)
    assert np.array_equal(ov, perm), (len(keys), bits)
    assert np.array_equal(ok, keys[perm]), (len(keys), bits)


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_kv_sort_sizes_and_widths(key_bytes):
    """every size x every width (odd and even pass counts), uniform keys with
    random bits above `bits`; kv_sort with and without keys_out, and sort_pairs"""
    rng = np.random.default_rng(1000 + key_bytes)
    dt = KEY_DT[key_bytes]
    for n in SIZES:
        for bits in BITS[key_bytes]:
            keys = make_keys(rng, n, bits, dt, "uniform")
            perm = stable_perm(keys, bits)
            check_kv_sort(keys, bits, perm)
            check_sort_pairs(keys, bits, perm)


@pytest.mark.parametrize("dist", ["equal", "two", "sorted", "reverse", "zipf"])
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_kv_sort_distributions(key_bytes, dist):
    """stability: whole tiles of one digit (the per-wave 16-bit counters reach
    1024), two alternating values, presorted and reversed input, a Zipf skew"""
    rng = np.random.default_rng(2000 + key_bytes)
    dt = KEY_DT[key_bytes]
    widths = {4: [1, 11, 12, 23, 32], 8: [33, 44, 64]}[key_bytes]
    for n in (65, 1025, TILE, TILE + 1, 9 * TILE + 1):
        for bits in widths:
            keys = make_keys(rng, n, bits, dt, dist)
            perm = stable_perm(keys, bits)
            check_kv_sort(keys, bits, perm)
            check_sort_pairs(keys, bits, perm)


def test_kv_sort_trivial_sizes():
    """n = 0 and n = 1 return the input pair untouched"""
    for dt in (np.uint32, np.uint64):
        ok, ov, which = PL.kv_sort(np.zeros(0, dt), np.zeros(0, np.uint32), 11, True)
        assert which == 0 and len(ov) == 0
        ok, ov, which = PL.kv_sort(np.array([77], dt), np.array([5], np.uint32), 11, True)
        assert which == 0 and ok[0] == 77 and ov[0] == 5
        ok, ov = PL.sort_pairs(np.array([77], dt), np.array([5], np.uint32), 22)
        assert ok[0] == 77 and ov[0] == 5


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_kv_sort_scan_paths(key_bytes):
    """the (digit, group) scan: 17 tiles x 2048 digits = 16 groups, 32768 sums (the
    one-block scan's four rounds); 66 tiles = 32 groups, 65536 sums (device-wide)"""
    rng = np.random.default_rng(3000 + key_bytes)
    dt = KEY_DT[key_bytes]
    for n in (17 * TILE, 65 * TILE + 1):
        for dist in ("uniform", "zipf"):
            keys = make_keys(rng, n, 11, dt, dist)
            perm = stable_perm(keys, 11)
            check_kv_sort(keys, 11, perm)
        keys = make_keys(rng, n, 22, dt, "uniform")
        check_sort_pairs(keys, 22, stable_perm(keys, 22))


def test_kv_sort_many_tiles_per_group(record_property):
    """4097 tiles: 5 tiles per group (rs_groups past 4 * 1024 tiles), 832 groups.
    The one large sort: 33.6 M pairs, about 0.6 GB of device memory."""
    n = 4097 * TILE
    rng = np.random.default_rng(4000)
    t0 = time.perf_counter()
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint32)  # 11 key bits, 21 random bits above
    perm = np.argsort((keys & np.uint32(0x7FF)).astype(np.uint16), kind="stable")
    t1 = time.perf_counter()
    ok, ov, which = PL.kv_sort(keys, np.arange(n, dtype=np.uint32), 11, True)
    t2 = time.perf_counter()
    assert which == 1
    assert np.array_equal(ov, perm)
    assert np.array_equal(ok, keys[perm])
    t3 = time.perf_counter()
    print("kv_sort 4097 tiles: host reference %.2f s, harness call (copies + device) %.2f s, compare %.2f s"
          % (t1 - t0, t2 - t1, t3 - t2))
    record_property("host_reference_s", round(t1 - t0 + t3 - t2, 3))
    record_property("harness_s", round(t2 - t1, 3))


@pytest.mark.parametrize("key_bytes", [4, 8])
def test_sort_pairs_v64(key_bytes):
    """64-bit values above 2^32 through the sorted index + gather; vals_in ==
    nullptr sorts the keys and leaves vals_out alone"""
    rng = np.random.default_rng(5000 + key_bytes)
    dt = KEY_DT[key_bytes]
    for n in (1, 65, 1025, TILE + 1, 9 * TILE + 1):
        for bits in {4: [11, 22, 32], 8: [33, 44, 64]}[key_bytes]:
            keys = make_keys(rng, n, bits, dt, "zipf" if n % 2 else "uniform")
            vals = rng.integers(1 << 32, 1 << 63, n, dtype=np.uint64) | np.uint64(1 << 63)
            perm = stable_perm(keys, bits)
            ok, ov = PL.sort_pairs_v64(keys, vals, bits)
            assert np.array_equal(ok, keys[perm]) and np.array_equal(ov, vals[perm]), (n, bits)
            ok, ov = PL.sort_pairs_v64(keys, None, bits)
            assert np.array_equal(ok, keys[perm]), (n, bits)
            assert np.all(ov == PL.FILL_U64), (n, bits)


# ---------------------------------------------------------------------------
# term_sort

def term_case(rng, P, bits, garbage):
    keys = make_keys(rng, P, bits, np.uint32, "zipf" if P % 3 == 0 else "uniform", garbage)
    vals = rng.integers(0, 1 << 32, P, dtype=np.uint32)
    return keys, vals


def check_term_sort(keys, vals, bits, maxbits, dmin, F, lut=None, idf=0.0, src=None, xw=None, Pout=0):
    """keys / vals: the P pairs in docno order; src: (source keys, source vals,
    reg, xoff) of gather mode"""
    P = len(keys)
    perm = stable_perm(keys, bits)
    if src is None:
        r = PL.term_sort(keys, vals, P, bits, dmin, F, lut=lut, idf=idf, maxbits=maxbits, xw=xw, Pout=Pout)
    else:
        r = PL.term_sort(src[0], src[1], P, bits, dmin, F, reg=src[2], xoff=src[3], lut=lut, idf=idf,
                         maxbits=maxbits, xw=xw, Pout=Pout)
    assert r["which"] == _npass(bits, 4, maxbits) % 2, (P, bits, maxbits, r["which"])
    sk, sv = keys[perm], vals[perm].astype(np.int64)
    docno, tf = (sv // F + dmin).astype(np.int32), (sv % F).astype(np.int32)
    if xw is None:
        slot = np.arange(P)
        assert np.array_equal(r["keys"], sk), (P, bits, maxbits)
    else:
        slot = np.arange(P) + xw[sk, 0].astype(np.int64)
        ek = np.full(Pout, 0xFFFFFFFF, np.uint32)
        ek[slot] = xw[sk, 1]
        assert np.array_equal(r["keys"], ek), (P, bits, maxbits)
    ed, et = np.full(max(P, Pout), PL.FILL_I32, np.int32), np.full(max(P, Pout), PL.FILL_I32, np.int32)
    ed[slot], et[slot] = docno, tf
    assert np.array_equal(r["docno"], ed), (P, bits, maxbits)
    assert np.array_equal(r["tf"], et), (P, bits, maxbits)
    if lut is not None:
        ew = np.full(max(P, Pout), PL.FILL_U64, np.uint64)
        ew[slot] = (lut[tf] * np.float64(idf)).view(np.uint64)  # one fp64 multiply, no FMA
        assert np.array_equal(r["w"].view(np.uint64), ew), (P, bits, maxbits)


TERM_SIZES = [1, 2, 63, 65, 1023, 1025, 8191, 8192, 8193, 7 * TILE, 8 * TILE + 1, 9 * TILE, 17 * TILE + 1]


@pytest.mark.parametrize("maxbits", [6, 8, 11])
def test_term_sort_direct(maxbits):
    """direct mode: digit widths x key widths x sizes; unpacking with F not a power
    of two and dmin 0 / large; the fused weights bit-equal to lut[tf] * idf"""
    rng = np.random.default_rng(6000 + maxbits)
    luts = {F: 1.0 + rng.random(F) * 9.0 for F in (1000, 65537)}
    i = 0
    for P in TERM_SIZES:
        for bits in (1, 13, 21, 22):
            F = (1000, 65537)[i % 2]
            dmin = (0, 2_000_000_000)[(i // 2) % 2]
            keys, vals = term_case(rng, P, bits, garbage=i % 3 == 0)
            lut = luts[F] if i % 4 != 3 else None
            check_term_sort(keys, vals, bits, maxbits, dmin, F, lut=lut, idf=float(np.log10(12345.0 + i)))
            i += 1


def gather_layout(rng, cnt, keys, vals):
    """regions with gaps between them, not in ascending address order"""
    cnt = np.asarray(cnt, np.int64)
    xoff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    order = rng.permutation(len(cnt))
    gaps = rng.integers(0, 8, len(cnt))
    reg = np.zeros(len(cnt), np.int64)
    pos = 3
    for j in order:
        reg[j] = pos
        pos += int(cnt[j]) + int(gaps[j])
    nslots = pos + 5
    sk = rng.integers(0, 1 << 32, nslots, dtype=np.uint32)  # the gaps hold junk
    sv = rng.integers(0, 1 << 32, nslots, dtype=np.uint32)
    rec = np.repeat(np.arange(len(cnt)), cnt)
    at = reg[rec] + np.arange(len(keys)) - xoff[rec]
    sk[at], sv[at] = keys, vals
    return sk, sv, reg, xoff


GATHER_CASES = {
    "one_record_over_tiles": [3 * TILE + 5],
    "records_of_1024": [1024] * 20,
    "empty_runs": [0] * 5 + [700, 0, 0, 0, 2000, 1] + [0] * 100 + [5000, 1024, 3] + [0] * 7,
    "many_small_records": None,  # 3000 records of 1 to 20 pairs: more than 48 per wave's 1024 items
    "mix": None,
}


def gather_counts(rng, name):
    if GATHER_CASES[name] is not None:
        return GATHER_CASES[name]
    small = rng.integers(1, 21, 3000).tolist()
    if name == "many_small_records":
        return small
    return ([0] * 3 + small[:700] + [2 * TILE + 77] + [0] * 60 + [1024] * 9 + small[700:1500] + [0, 0, 5000] +
            [1] * 2100 + [0] * 4)


@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_term_sort_gather(name):
    """gather mode (reg / xoff): pair x of record i at reg[i] + x - xoff[i]; one,
    two and four passes (the only pass is then both the gathering and the last)"""
    rng = np.random.default_rng(7000)
    cnt = gather_counts(rng, name)
    P = int(np.sum(cnt))
    for bits, maxbits, F, dmin in ((11, 11, 1000, 0), (13, 11, 65537, 2_000_000_000), (22, 6, 1000, 17)):
        keys, vals = term_case(rng, P, bits, garbage=bits == 13)
        lut = 1.0 + rng.random(F)
        check_term_sort(keys, vals, bits, maxbits, dmin, F, lut=lut, idf=3.25, src=gather_layout(rng, cnt, keys, vals))


@pytest.mark.parametrize("gather", [False, True])
def test_term_sort_docid_slots(gather):
    """K6b (xw, Pout): word i's postings land shifted by xw[i].x and keyed xw[i].y;
    every other key slot is 0xFFFFFFFF and its docno / tf / w slots are untouched"""
    rng = np.random.default_rng(8000 + gather)
    for P, W, maxbits in ((1, 1, 11), (1025, 37, 11), (TILE + 1, 5000, 11), (9 * TILE + 1, 1 << 13, 11),
                          (8 * TILE, 3000, 6)):
        bits = max(1, int(W - 1).bit_length())
        keys = rng.integers(0, W, P, dtype=np.uint32)
        vals = rng.integers(0, 1 << 32, P, dtype=np.uint32)
        ins = rng.integers(0, 4, W) * (rng.random(W) < 0.3)
        xw = np.empty((W, 2), np.uint32)
        xw[:, 0] = np.cumsum(ins)                            # slots inserted before word i: nondecreasing
        xw[:, 1] = rng.integers(0, 0xFFFFFFFF, W, dtype=np.uint32)  # merged ids, any order
        Pout = P + int(xw[-1, 0]) + 3
        src = None
        if gather:
            cnt = np.diff(np.concatenate([[0], np.sort(rng.integers(0, P + 1, 40)), [P]]))
            src = gather_layout(rng, cnt, keys, vals)
        F = 65537
        check_term_sort(keys, vals, bits, maxbits, 5, F, lut=1.0 + rng.random(F), idf=2.5, src=src, xw=xw, Pout=Pout)


def test_term_sort_empty():
    """P = 0 returns k0 and touches nothing"""
    keys = np.arange(100, dtype=np.uint32) * 7
    r = PL.term_sort(keys, keys, 0, 11, 0, 1000, lut=np.ones(1000), idf=1.0, nout=100)
    assert r["which"] == 0
    assert np.array_equal(r["keys"], keys)
    assert np.all(r["docno"] == PL.FILL_I32) and np.all(r["tf"] == PL.FILL_I32)
    assert np.all(r["w"].view(np.uint64) == PL.FILL_U64)


# ---------------------------------------------------------------------------
# excl_scan

SCAN_SIZES = [1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1, 1_000_003]


def excl_ref(a):
    out = np.zeros_like(a)
    np.cumsum(a[:-1], dtype=a.dtype, out=out[1:])
    return out


def check_scan(a):
    ref = excl_ref(a)
    for inplace in (False, True):
        got = PL.excl_scan(a, inplace)
        assert got.dtype == a.dtype and np.array_equal(got, ref), (a.dtype, len(a), inplace)


@pytest.mark.parametrize("dt", [np.int32, np.uint32, np.int64])
def test_excl_scan_sizes(dt):
    """in != out and in == out at the 16-item, 256-thread and 4096-item tile edges;
    uint32 sums that wrap, int64 sums past 2^40"""
    rng = np.random.default_rng(9000)
    for n in SCAN_SIZES:
        if dt == np.int32:
            a = rng.integers(-1000, 1001, n).astype(np.int32)
        elif dt == np.uint32:
            a = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        else:
            a = rng.integers(-(1 << 36), 1 << 40, n, dtype=np.int64)
        check_scan(a)
        if dt == np.int64 and n >= 16:
            assert excl_ref(a)[-1] > 1 << 40
        if dt == np.uint32 and n >= 16:
            assert int(a[:-1].astype(np.uint64).sum()) >= 1 << 32  # the sum wraps


@pytest.mark.parametrize("dt", [np.int32, np.uint32, np.int64])
def test_excl_scan_sparse(dt):
    """all zeros; a single nonzero at the first, the last and tile-boundary positions"""
    n = 2 * 4096 + 1
    check_scan(np.zeros(n, dt))
    for at in (0, 15, 16, 255, 256, 4095, 4096, 4097, 8191, 8192):
        a = np.zeros(n, dt)
        a[at] = 12345
        check_scan(a)


def test_excl_scan_carry_second_round(record_property):
    """n = 4096 * 4096 + 1: 4097 tile sums, the smallest n at which k_sc_carry
    takes a second round of 4096"""
    n = 4096 * 4096 + 1
    rng = np.random.default_rng(9100)
    t0 = time.perf_counter()
    a = rng.integers(0, 256, n, dtype=np.uint32)
    ref = excl_ref(a)
    t1 = time.perf_counter()
    got = PL.excl_scan(a, False)
    got2 = PL.excl_scan(a, True)
    t2 = time.perf_counter()
    assert np.array_equal(got, ref)
    assert np.array_equal(got2, ref)
    t3 = time.perf_counter()
    print("excl_scan 16.7 M: host reference %.2f s, two harness calls (copies + device) %.2f s, compare %.2f s"
          % (t1 - t0, t2 - t1, t3 - t2))
    record_property("host_reference_s", round(t1 - t0 + t3 - t2, 3))
    record_property("harness_s", round(t2 - t1, 3))


# ---------------------------------------------------------------------------
# select_flagged

def check_select(flag):
    out, count = PL.select_flagged(flag)
    ref = np.flatnonzero(flag).astype(np.int32)
    assert count == len(ref), (len(flag), count)
    assert np.array_equal(out[:count], ref), len(flag)
    assert np.all(out[count:] == PL.FILL_I32), len(flag)  # nothing written past the count


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097, 16384 * 256 + 1])
def test_select_flagged(n):
    """flag patterns at every size; 16384 * 256 + 1 is past the grid cap, so the
    stride loop runs; any nonzero flag byte counts as set"""
    rng = np.random.default_rng(10000 + n % 1000)
    pats = [np.zeros(n, np.uint8), np.ones(n, np.uint8)]
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[0], last[-1] = 1, 0x80
    pats += [first, last]
    for p in (0.01, 0.5, 0.99):
        f = (rng.random(n) < p).astype(np.uint8)
        pats.append(f)
    pats.append(pats[5] * rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), n))  # bytes other than 0 / 1
    for f in pats:
        check_select(f)


def test_select_flagged_empty():
    out, count = PL.select_flagged(np.zeros(0, np.uint8))
    assert count == 0 and len(out) == 0


# ---------------------------------------------------------------------------
# reduce_max

@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_reduce_max(dt):
    rng = np.random.default_rng(11000)
    top = (1 << 31) - 1 if dt == np.int32 else (1 << 62)
    assert PL.reduce_max(np.zeros(0, dt)) == 0
    for n in (1, 63, 64, 65, 2048 * 256 + 1):
        assert PL.reduce_max(np.zeros(n, dt)) == 0
        a = rng.integers(0, top, n).astype(dt)
        assert PL.reduce_max(a) == np.maximum.reduce(a), n
        for at in sorted({0, n - 1, min(63, n - 1), min(64, n - 1), min(2048 * 256, n - 1)}):
            b = rng.integers(0, 1000, n).astype(dt)
            b[at] = top  # int64: above 2^32
            assert PL.reduce_max(b) == top, (n, at)
            b[at] = 1001
            assert PL.reduce_max(b) == 1001, (n, at)


# ---------------------------------------------------------------------------
# reduce_by_key_sum

def check_rbk(keys, vals):
    keys, vals = np.asarray(keys, np.uint64), np.asarray(vals, np.int32)
    uk, sums, runs = PL.reduce_by_key_sum(keys, vals)
    n = len(keys)
    if n == 0:
        assert runs == 0
        return
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    assert runs == len(heads), (n, runs)
    assert np.array_equal(uk[:runs], keys[heads]), n
    assert np.array_equal(sums[:runs], np.add.reduceat(vals, heads, dtype=np.int32)), n


def test_reduce_by_key_sum_shapes():
    """distinct keys, one run, runs across the 256- and 4096-element boundaries,
    keys differing only above bit 32, both signs in one run"""
    rng = np.random.default_rng(12000)
    check_rbk([], [])
    check_rbk([9], [-4])
    n = 3 * 4096 + 17
    vals = rng.integers(-1000, 1001, n)
    check_rbk(np.arange(n) * 3, vals)
    check_rbk(np.full(n, 1 << 40), vals)
    cuts = np.array([250, 260, 4090, 4100, 8191, 8193])  # runs [250, 260) ... straddle the boundaries
    check_rbk(np.searchsorted(cuts, np.arange(n), side="right"), vals)
    hi = (np.arange(n, dtype=np.uint64) // np.uint64(5)) << np.uint64(32)
    check_rbk(hi | np.uint64(7), vals)
    check_rbk(np.repeat(np.arange(n // 64 + 1), 64)[:n], np.where(np.arange(n) & 1, 1 << 30, -(1 << 30)))


def test_reduce_by_key_sum_grid_stride():
    """16384 * 256 + 1 items: past the grid cap"""
    n = 16384 * 256 + 1
    rng = np.random.default_rng(12100)
    keys = np.cumsum(rng.random(n) < 0.2).astype(np.uint64) << np.uint64(20)
    check_rbk(keys, rng.integers(-50, 51, n))
