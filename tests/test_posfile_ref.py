"""The Python restatement of the positions file (tests/posfile_ref.py) against
itself and against literals: round trips for every width at the sizes where a
64-bit word fills up, a hand-built three-record file byte for byte, and the digest
constants tools/posfile_check.cc holds the C++ to.  No GPU."""
import random
import struct

import pytest

import posfile_ref as R

VOCAB3 = ["apple", "berry", "café€"]
DIGEST3 = 0xa9603576f19cd8fd


@pytest.mark.parametrize("b", range(1, 32))
def test_round_trip_every_width(b):
    rng = random.Random(b)
    for T in (0, 1, 63, 64, 65):
        ids = [rng.randrange(1 << b) for _ in range(T)]
        if T:
            ids[0], ids[-1] = (1 << b) - 1, (1 << b) - 1  # every bit of the width, first and last
        words = R.pack_ids(ids, b)
        assert len(words) == (T * b + 63) // 64 * 8
        assert R.unpack_ids(words, T, b) == ids
        # bit by bit: bit k of id p is bit p b + k of the little-endian string
        big = int.from_bytes(words, "little")
        assert all((big >> (p * b + k)) & 1 == (ids[p] >> k) & 1 for p in range(T) for k in range(b))
        assert big >> (T * b) == 0  # the unused high bits are zero
        # a whole file: two records around an empty one
        cut = T // 2
        recs = [(-5, ids[:cut]), (0, []), (0, ids[cut:])]
        V = 1 << b
        data = R.encode(recs, V, 77, bits=b)
        h, back = R.decode(data)
        assert back == recs and h == {"version": 1, "bits": b, "records": 3, "positions": T, "V": V, "digest": 77}


def test_need_bits():
    assert [R.need_bits(v) for v in (0, 1, 2, 3, 4, 5, 256, 257, 300, 1 << 31)] == [1, 1, 1, 2, 2, 3, 8, 9, 9, 31]
    assert R.encode([], 300, 0)[12:16] == struct.pack("<I", 9)  # bits = 0 writes need


def test_hand_built_file():
    """Three records: docno -3 holds ids 2 0, docno 7 an empty record and then 1 2 2;
    V = 3, so two bits: 2 | 0 << 2 | 1 << 4 | 2 << 6 | 2 << 8 = 0x292."""
    data = R.encode([(-3, [2, 0]), (7, []), (7, [1, 2, 2])], 3, R.digest(VOCAB3))
    want = bytes.fromhex(
        "534d45504f530001" "01000000" "02000000"          # magic, version 1, bits 2
        "0300000000000000" "0500000000000000"             # 3 records, 5 positions
        "0300000000000000" "fdd89cf1763560a9"             # V = 3, the digest
        "00000000000000000000000000000000"                # reserved
        "fdffffff" "07000000" "07000000" "00000000"       # docno -3 7 7, padding
        "02000000" "00000000" "03000000" "00000000"       # len 2 0 3, padding
        "9202000000000000")                               # one word
    assert data == want and len(data) == 104


def test_digest_constants():
    """The constants of tools/posfile_check.cc's check_digest."""
    assert R.digest([]) == 0
    assert R.term_hash(0, "a") == R.digest(["a"]) == 0x6962e1cc2097a744
    assert R.term_hash(0, "apple") == 0x7e1fe7371f310b95 and R.term_hash(2, VOCAB3[2]) == 0xfef24425352306e6
    assert R.digest(VOCAB3) == DIGEST3
    assert R.digest(["berry", "apple", VOCAB3[2]]) == 0xd3ea7f7a6af6f91d  # the id is hashed in: the order counts
    assert R.digest(["", "\U0001F600"]) == 0xd926a30c124dd904            # the empty term, a surrogate pair
    # FNV-1a-64 by the book for one term
    h = 0xcbf29ce484222325
    for byte in bytes(8) + b"a\x00":
        h = ((h ^ byte) * 0x100000001b3) % (1 << 64)
    assert h == 0x6962e1cc2097a744
