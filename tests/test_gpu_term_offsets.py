"""term_sort's offset output (csrc/sme_sort.hip: off_out / write_keys,
k_rs_term_off) against numpy's stable sort, bit-exact: the first slot of every
term id that has pairs, read out of the last pass's (tile, digit) offset table
and a per-tile digit histogram in front of each low-part segment's start, with no
pass over the sorted keys.  Through libsme_prims.so (tests/native/prims_termoff.hip)
with the guard and fill discipline of the other primitive tests.

Every case runs the sort twice, with write_keys true and false.  Both must give
the reference's docno / tf / w and offsets; with write_keys false the returned
key buffer must hold exactly what the passes before the last left there (the
fill pattern after one pass, the source after two, an earlier pass's output
after three or four), so the last pass stored no key."""
import ctypes as C

import numpy as np
import pytest

import prims_lib as PL
from test_gpu_prims import GATHER_CASES, TILE, gather_counts, gather_layout, stable_perm
from test_gpu_term_sort_packed import packed_layout, small_records

pytestmark = pytest.mark.gpu

_vp, _i64, _int = C.c_void_p, C.c_int64, C.c_int
_ip = C.POINTER(C.c_int)
GUARDS = ("k0", "k1", "v0", "v1", "docno", "tf", "w", "scratch", "off")
FILL_U32 = np.uint32(0xA5A5A5A5)
FILL_I64 = np.frombuffer(bytes([PL.FILL_BYTE] * 8), np.int64)[0]

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(PL.LIB_PATH)
        L.smep_termoff_last_error.restype, L.smep_termoff_last_error.argtypes = C.c_char_p, []
        L.smep_term_sort_off.restype = _int
        L.smep_term_sort_off.argtypes = [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _int, _i64, _int, _i64, C.c_uint32, _vp,
                                         _i64, C.c_double, _int, _vp, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp,
                                         _vp, _vp, _vp, _ip, _ip]
        _lib = L
    return _lib


def term_sort_off(keys, vals, P, bits, dmin, F, V, vend, write_keys, reg=None, xoff=None, rec_val=None, tf_shift=0,
                  lut=None, idf=0.0, maxbits=11, xw=None, Pout=0):
    keys, vals, rec_val = PL._c(keys, np.uint32), PL._c(vals, np.uint32), PL._c(rec_val, np.uint32)
    reg, xoff, lut, xw = PL._c(reg, np.int64), PL._c(xoff, np.int64), PL._c(lut, np.float64), PL._c(xw, np.uint32)
    nout = max(P, Pout)
    ok, od, ot = np.empty(nout, np.uint32), np.empty(nout, np.int32), np.empty(nout, np.int32)
    ow = None if lut is None else np.empty(nout, np.float64)
    off = np.empty(vend + 1, np.int64)
    which, guard = C.c_int(-2), C.c_int(0)
    p = PL._p
    rc = lib().smep_term_sort_off(p(keys), p(vals), len(keys), 0 if reg is None else len(reg), p(reg), p(xoff),
                                  p(rec_val), tf_shift, P, bits, dmin, F, p(lut), 0 if lut is None else len(lut), idf,
                                  maxbits, p(xw), 0 if xw is None else len(xw), Pout, nout, V, vend, int(write_keys),
                                  p(ok), p(od), p(ot), p(ow), p(off), C.byref(which), C.byref(guard))
    if rc != 0:
        msg = lib().smep_termoff_last_error().decode()
        if rc == -2:  # SME_EHIP: the device context may be lost, so nothing more is started on it
            pytest.exit("HIP error in the primitive harness: " + msg, returncode=3)
        raise PL.PrimsError(rc, msg)
    if guard.value:
        raise PL.GuardError("changed: " + ", ".join(n for i, n in enumerate(GUARDS) if guard.value >> i & 1))
    return dict(keys=ok, docno=od, tf=ot, w=ow, off=off, which=which.value)


def digit_widths(bits, maxbits):
    """the passes' digit widths, as term_sort splits them (near-equal, wider first)"""
    npass = (max(bits, 1) + maxbits - 1) // maxbits
    out, shift = [], 0
    for p in range(npass):
        nb = (bits - shift + (npass - p) - 1) // (npass - p)
        out.append(nb)
        shift += nb
    return out


# ---------------------------------------------------------------------------
# key sets (each returns P keys below 2^bits)

def keys_uniform(rng, P, bits, shift):
    return rng.integers(0, 1 << bits, P, dtype=np.uint64).astype(np.uint32)


def keys_zipf(rng, P, bits, shift):
    """a few frequent ids and many absent ones, spread over the id range"""
    k = np.minimum(rng.zipf(1.3, P), 1 << bits).astype(np.uint64) - np.uint64(1)
    return ((k * np.uint64(2654435761)) & np.uint64((1 << bits) - 1)).astype(np.uint32)


def keys_one(rng, P, bits, shift):
    return np.full(P, rng.integers(0, 1 << bits), np.uint32)


def keys_perm(rng, P, bits, shift):
    """a permutation of 0 .. P - 1 (wrapped at 2^bits): every item its own segment"""
    return (rng.permutation(P).astype(np.uint64) & np.uint64((1 << bits) - 1)).astype(np.uint32)


def keys_tile_edges(rng, P, bits, shift):
    """low parts 0 and 1 hold exactly 8192 items each: the segments of low parts 1
    and 2 start on positions 8192 and 16384 of the last pass's input"""
    if shift < 2:
        return keys_uniform(rng, P, bits, shift)
    low = np.full(P, 2, np.uint32)
    low[:min(P, TILE)] = 0
    low[TILE:min(P, 2 * TILE)] = 1
    if P > 2 * TILE:
        low[2 * TILE:] = 2 + rng.integers(0, min(1 << shift, 64) - 2, P - 2 * TILE)
    low = rng.permutation(low)
    digit = rng.integers(0, 1 << (bits - shift), P, dtype=np.uint32)
    return (digit << np.uint32(shift)) | low


def keys_span3(rng, P, bits, shift):
    """low part 1's segment starts inside a tile and spans three more, and its top
    digit first appears in the last of them: the term's first slot is counted from
    the segment's first tile, not from the tile the digit is first seen in"""
    nd = 1 << (bits - shift)
    if shift < 2 or nd < 2:
        return keys_uniform(rng, P, bits, shift)
    n0 = min(100, P // 4)
    n1 = min(3 * TILE, P - n0)
    late = min(n1 - 1, 2 * TILE + 500)  # positions of segment 1 before the top digit appears
    d1 = rng.integers(0, nd - 1, n1, dtype=np.uint32)
    d1[late:] = np.where(rng.random(n1 - late) < 0.5, nd - 1, d1[late:])
    d1[late] = nd - 1
    nrest = P - n0 - n1
    label = rng.permutation(np.repeat(np.arange(3), [n0, n1, nrest]))
    keys = np.empty(P, np.uint32)
    keys[label == 0] = rng.integers(0, nd, n0, dtype=np.uint32) << np.uint32(shift)
    keys[label == 1] = (d1 << np.uint32(shift)) | np.uint32(1)
    keys[label == 2] = ((rng.integers(0, nd, nrest, dtype=np.uint32) << np.uint32(shift)) |
                        rng.integers(2, min(1 << shift, 40), nrest).astype(np.uint32))
    return keys


KEY_SETS = (keys_uniform, keys_zipf, keys_one, keys_perm, keys_tile_edges, keys_span3)
# (17 tiles and one item: a second workgroup of k_rs_term_off, which takes 16 tiles each)
SIZES = [1, 2, 8191, 8192, 8193, 2 * TILE, 9 * TILE + 1, 17 * TILE + 1]
# one pass with shift 0 (two widths), two passes, 11 + 10, three passes, four passes
PASSES = ((1, 11), (11, 11), (12, 11), (21, 11), (22, 8), (22, 6))
_ids = ["%d_%d" % p for p in PASSES]


# ---------------------------------------------------------------------------

def expected_unwritten(src, nslots, nout, P, pass_keys, widths):
    """the first nout elements of the returned key buffer when the last pass
    stores no keys.  pass_keys: the P keys as a pass writes them"""
    npass = len(widths)
    if npass % 2 == 1:  # k1: nout elements, written by the passes 1, 3, ...
        buf = np.full(nout, FILL_U32, np.uint32)
        done = sum(widths[:npass - 2]) if npass >= 3 else 0
    else:  # k0: the source, then fill; written by the passes 2, 4, ...
        buf = np.full(max(nslots, nout), FILL_U32, np.uint32)
        buf[:nslots] = src
        buf = buf[:nout]
        done = sum(widths[:npass - 2]) if npass >= 4 else 0
    if done:
        buf[:P] = pass_keys[stable_perm(pass_keys, done)]
    return buf


def check(rng, keys, bits, maxbits, mode, cnt=None, holes=False):
    """keys: P keys below 2^bits in docno order.  mode: direct / gather / packed;
    cnt: the records' pair counts of the gather modes; holes: K6b (xw, Pout)"""
    P = len(keys)
    widths = digit_widths(bits, maxbits)
    mask = np.uint32((1 << bits) - 1)
    dmin = 2_000_000_000
    if mode == "packed":
        F = min(1 << (32 - bits), 1 << 16)
        tfs = rng.integers(0, F, P, dtype=np.uint32)
        words = keys | (tfs.astype(np.uint64) << np.uint64(bits)).astype(np.uint32)
        src, reg, xoff, rec = packed_layout(rng, cnt, words)
        rec_val = (rng.integers(0, ((1 << 32) - F) // F + 1, len(cnt)) * F).astype(np.uint32)
        vals = rec_val[rec].astype(np.int64) + tfs
        srcv, raw = None, keys
        kw = dict(reg=reg, xoff=xoff, rec_val=rec_val, tf_shift=bits)
    else:
        F = 65537
        raw = keys
        # junk above the key in every other case (never with xw: the last pass indexes
        # xw by the whole key word, and the build's word ranks have nothing above them)
        if bits < 32 and P % 2 and not holes:
            raw = keys | (rng.integers(0, 1 << (32 - bits), P, dtype=np.uint64) << np.uint64(bits)).astype(np.uint32)
        vals = rng.integers(0, 1 << 32, P, dtype=np.uint32).astype(np.int64)
        if mode == "gather":
            src, srcv, reg, xoff = gather_layout(rng, cnt, raw, vals.astype(np.uint32))
            kw = dict(reg=reg, xoff=xoff)
        else:
            src, srcv, kw = raw, vals.astype(np.uint32), {}
    lut = 1.0 + rng.random(F)
    V = 1 << bits
    xw, Pout, vend = None, 0, V
    if holes:
        ins = rng.integers(0, 4, V) * (rng.random(V) < 0.3)
        vend = V + V // 3 + 5
        xw = np.empty((V, 2), np.uint32)
        xw[:, 0] = np.cumsum(ins)
        xw[:, 1] = np.sort(rng.choice(vend, V, replace=False))  # distinct merged ids, ids between them unused
        Pout = P + int(xw[-1, 0]) + 3
    nout = max(P, Pout)
    perm = stable_perm(keys, bits)
    sk, sv = keys[perm], vals[perm]
    docno, tf = (sv // F + dmin).astype(np.int32), (sv % F).astype(np.int32)
    slot = np.arange(P) if xw is None else np.arange(P) + xw[sk, 0].astype(np.int64)
    ed, et = np.full(nout, PL.FILL_I32, np.int32), np.full(nout, PL.FILL_I32, np.int32)
    ew = np.full(nout, PL.FILL_U64, np.uint64)
    ed[slot], et[slot] = docno, tf
    ew[slot] = (lut[tf] * np.float64(3.25)).view(np.uint64)
    if xw is None:
        ek = np.full(nout, FILL_U32, np.uint32)
        ek[:P] = (raw if mode != "packed" else keys)[perm]
    else:
        ek = np.full(Pout, 0xFFFFFFFF, np.uint32)
        ek[slot] = xw[sk, 1]
    ids, first = np.unique(sk, return_index=True)  # every id with pairs and its first sorted position
    eoff = first.astype(np.int64)
    at = ids.astype(np.int64)
    if xw is not None:
        eoff = eoff + xw[ids, 0]
        at = xw[ids, 1].astype(np.int64)
    tag = (P, bits, maxbits, mode, holes)
    for write_keys in (True, False):
        r = term_sort_off(src, srcv, P, bits, dmin, F, V, vend, write_keys, lut=lut, idf=3.25, maxbits=maxbits, xw=xw,
                          Pout=Pout, **kw)
        assert r["which"] == len(widths) % 2, tag
        assert np.array_equal(r["off"][at], eoff), (tag, write_keys)
        assert r["off"][vend] == (Pout if holes else P), (tag, write_keys)
        assert np.array_equal(r["docno"], ed), (tag, write_keys)
        assert np.array_equal(r["tf"], et), (tag, write_keys)
        assert np.array_equal(r["w"].view(np.uint64), ew), (tag, write_keys)
        if write_keys:
            assert np.array_equal(r["keys"], ek), tag
        else:
            pk = raw if mode != "packed" else keys
            assert np.array_equal(r["keys"], expected_unwritten(src, len(src), nout, P, pk, widths)), tag
        if holes:  # merged ids that are no word's stay untouched
            unused = np.setdiff1d(np.arange(vend), xw[:, 1])
            assert np.all(r["off"][unused] == FILL_I64), (tag, write_keys)


@pytest.mark.parametrize("bits,maxbits", PASSES, ids=_ids)
def test_offsets_direct(bits, maxbits):
    rng = np.random.default_rng(9400 + 32 * bits + maxbits)
    shift = sum(digit_widths(bits, maxbits)[:-1])
    for P in SIZES:
        for ks in KEY_SETS:
            check(rng, ks(rng, P, bits, shift), bits, maxbits, "direct")


@pytest.mark.parametrize("bits,maxbits", PASSES, ids=_ids)
@pytest.mark.parametrize("name", ["empty_runs", "many_small_records"])
def test_offsets_gather(name, bits, maxbits):
    """the first pass gathers; with one pass it is also the last and no key is read
    for the offsets"""
    rng = np.random.default_rng(9500 + 32 * bits + maxbits)
    cnt = gather_counts(rng, name)
    P = int(np.sum(cnt))
    shift = sum(digit_widths(bits, maxbits)[:-1])
    for ks in KEY_SETS:
        check(rng, ks(rng, P, bits, shift), bits, maxbits, "gather", cnt=cnt)


@pytest.mark.parametrize("bits,maxbits", PASSES, ids=_ids)
def test_offsets_packed_gather(bits, maxbits):
    rng = np.random.default_rng(9600 + 32 * bits + maxbits)
    shift = sum(digit_widths(bits, maxbits)[:-1])
    for cnt in (GATHER_CASES["empty_runs"], small_records(rng, TILE + 1), [9 * TILE + 1]):
        P = int(np.sum(cnt))
        for ks in KEY_SETS:
            check(rng, ks(rng, P, bits, shift), bits, maxbits, "packed", cnt=cnt)


@pytest.mark.parametrize("bits,maxbits", [(1, 11), (11, 11), (13, 11), (13, 6), (13, 4)],
                         ids=["1_11", "11_11", "13_11", "13_6", "13_4"])
def test_offsets_docid_slots(bits, maxbits):
    """K6b (xw, Pout): word k's entry lands at its merged id xw[k].y, shifted by the
    slots xw[k].x inserted before it; the merged ids of no word are not written"""
    rng = np.random.default_rng(9700 + 32 * bits + maxbits)
    shift = sum(digit_widths(bits, maxbits)[:-1])
    for P in (1, 8193, 9 * TILE + 1):
        for ks in KEY_SETS:
            keys = ks(rng, P, bits, shift)
            check(rng, keys, bits, maxbits, "direct", holes=True)
            check(rng, keys, bits, maxbits, "packed", cnt=small_records(rng, P), holes=True)


def test_offsets_empty():
    """P = 0: only the end entry is written, 0 (Pout with xw)"""
    keys = np.arange(100, dtype=np.uint32)
    r = term_sort_off(keys, keys, 0, 11, 0, 1000, 2048, 2048, False, lut=np.ones(1000), idf=1.0)
    assert r["which"] == 0 and r["off"][2048] == 0 and np.all(r["off"][:2048] == FILL_I64)
    xw = np.zeros((2048, 2), np.uint32)
    r = term_sort_off(keys, keys, 0, 11, 0, 1000, 2048, 3000, True, lut=np.ones(1000), idf=1.0, xw=xw, Pout=7)
    assert r["off"][3000] == 7 and np.all(r["off"][:3000] == FILL_I64)
