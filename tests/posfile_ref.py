"""The positions file restated in plain Python, from its specification in
include/sme.h (not from the C++): header, sections, the little-endian bit string
of the ids, and the vocabulary digest.

  offset 0   magic 53 4D 45 50 4F 53 00 01          40  u64 vocabulary digest
         8   u32 version = 1                        48  16 reserved zero bytes
        12   u32 bits b (need <= b <= 31)           64  int32 docno[Rn], padded to 8 bytes
        16   u64 records Rn                       then  u32 len[Rn], padded to 8 bytes
        24   u64 positions T                      then  u64 word[ceil(T b / 64)]
        32   u64 V
Position p's id occupies bits [p b, (p + 1) b) of the words seen as one
little-endian bit string; all integers are little-endian.

Expected streams come from phrase_ref.Streams.records, stably sorted by signed
docno, with term ids from Index.lookup (streams_of)."""
import struct

MAGIC = bytes([0x53, 0x4D, 0x45, 0x50, 0x4F, 0x53, 0x00, 0x01])
VERSION = 1
HEADER = 64
FNV_BASIS, FNV_PRIME, M64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1


def need_bits(V):
    """max(1, bit length of (V - 1))."""
    return max(1, (V - 1).bit_length()) if V > 0 else 1


def term_hash(t, term):
    """FNV-1a-64 over the 8 bytes of t (little-endian), then the term's UTF-16 code
    units, each low byte first.  term: a str (surrogates as they stand)."""
    h = FNV_BASIS
    for byte in struct.pack("<Q", t) + term.encode("utf-16-le", "surrogatepass"):
        h = ((h ^ byte) * FNV_PRIME) & M64
    return h


def digest(terms):
    """Sum over t < V of h_t mod 2^64; terms in id order."""
    return sum(term_hash(t, s) for t, s in enumerate(terms)) & M64


def pack_ids(ids, b):
    """The word section: ceil(T b / 64) little-endian u64 words."""
    big = 0
    for p, v in enumerate(ids):
        assert 0 <= v < (1 << b)
        big |= v << (p * b)
    nwords = (len(ids) * b + 63) // 64
    return big.to_bytes(nwords * 8, "little")


def unpack_ids(words, T, b):
    big = int.from_bytes(words, "little")
    return [(big >> (p * b)) & ((1 << b) - 1) for p in range(T)]


def _pad8(data):
    return data + b"\x00" * (-len(data) % 8)


def header(bits, records, positions, V, dig, version=VERSION, magic=MAGIC, reserved=b"\x00" * 16):
    return magic + struct.pack("<IIQQQQ", version, bits, records, positions, V, dig) + reserved


def encode(records, V, dig, bits=0):
    """records: [(docno, [term id, ...])] in file order (docno ascending)."""
    b = bits or need_bits(V)
    ids = [t for _, s in records for t in s]
    out = header(b, len(records), len(ids), V, dig)
    out += _pad8(b"".join(struct.pack("<i", d) for d, _ in records))
    out += _pad8(b"".join(struct.pack("<I", len(s)) for _, s in records))
    return out + pack_ids(ids, b)


def sections(data):
    """(header fields dict, docno offset, len offset, word offset) of a well-formed file."""
    version, b, Rn, T, V, dig = struct.unpack_from("<IIQQQQ", data, 8)
    sec = (4 * Rn + 7) // 8 * 8
    return ({"version": version, "bits": b, "records": Rn, "positions": T, "V": V, "digest": dig},
            HEADER, HEADER + sec, HEADER + 2 * sec)


def decode(data):
    """-> (header fields, [(docno, [term id, ...])]) of a well-formed file."""
    h, d_at, l_at, w_at = sections(data)
    Rn, T, b = h["records"], h["positions"], h["bits"]
    assert data[:8] == MAGIC and len(data) == w_at + (T * b + 63) // 64 * 8
    docnos = struct.unpack_from("<%di" % Rn, data, d_at)
    lens = struct.unpack_from("<%dI" % Rn, data, l_at)
    ids = unpack_ids(data[w_at:], T, b)
    assert sum(lens) == T
    out, p = [], 0
    for d, n in zip(docnos, lens):
        out.append((d, ids[p:p + n]))
        p += n
    return h, out


def streams_of(ix, stream_records):
    """phrase_ref.Streams.records ([(docno, [term string, ...])] in file order) as
    the index holds them: stably sorted by signed docno, terms as Index.lookup's ids."""
    words = sorted(set(t for _, s in stream_records for t in s))
    ids = dict(zip(words, ix.lookup(words).tolist())) if words else {}
    assert all(v >= 0 for v in ids.values())
    return [(d, [ids[t] for t in s]) for d, s in sorted(stream_records, key=lambda r: r[0])]


def file_of(ix, stream_records, bits=0):
    """The file the library must write for an index over those records."""
    return encode(streams_of(ix, stream_records), ix.V, digest(ix.terms()), bits)
