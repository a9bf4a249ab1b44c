"""Phrase queries restated in plain Python over per-record term streams.

A record's stream is oracle_lib.process_content of its text: the tokens the
reference's mapper makes its k-grams from.  The docno of a record is the one the
oracle's own map step gave it -- the oracle's " " doc-counter term posts, record
after record, the docno of the record BEFORE (MyMapper's shared posting), so
posting r + 1 is record r's docno; only the last record's never appears there and
is looked up as TrecDocnoMapping.getDocno does (and every other record's is held
to that lookup too).

A phrase of m terms then matches document d with frequency pf iff the reference's
K = m index holds that gram with posting (d, pf): test_phrase_ref.py holds
Streams.grams(m) to OracleIndex(..., K=m).terms() gram by gram."""
import math
import struct
from collections import defaultdict

import numpy as np

import oracle_lib as O


def mapping_ids(mapping):
    """The docids of a mapping file: int32 N, N x writeUTF(docid)."""
    n = struct.unpack_from(">i", mapping, 0)[0]
    p, ids = 4, []
    for _ in range(n):
        ln = struct.unpack_from(">H", mapping, p)[0]
        ids.append(O.mutf8_decode(mapping[p + 2:p + 2 + ln]))
        p += 2 + ln
    return ids


def _units(s):
    return s.encode("utf-16-be", "surrogatepass")  # String.compareTo order


def get_docid(text):
    """TrecDocument.getDocid: trimmed text between the first <DOCNO> and the next </DOCNO>."""
    a = text.find(b"<DOCNO>")
    if a < 0:
        return ""
    b = text.index(b"</DOCNO>", a)
    return text[a + 7:b].decode("utf-8", "replace").strip("".join(chr(c) for c in range(0x21)))


def get_docno(ids, docid):
    """Arrays.binarySearch over {"", docids...}."""
    keys = [b""] + [_units(i) for i in ids]
    k = _units(docid)
    lo, hi = 0, len(keys) - 1
    while lo <= hi:
        mid = (lo + hi) >> 1
        if keys[mid] < k:
            lo = mid + 1
        elif keys[mid] > k:
            hi = mid - 1
        else:
            return mid
    return -(lo + 1)


def phrase_count(stream, phrase):
    """Occurrences of the phrase in one record's stream: overlaps all count."""
    L = len(phrase)
    if L == 0:
        return 0
    phrase = list(phrase)
    return sum(1 for s in range(len(stream) - L + 1) if stream[s:s + L] == phrase)


class Streams:
    """records: [(docno, [term, ...])] in file order."""

    def __init__(self, corpus, mapping, oracle_k1=None):
        ids = mapping_ids(mapping)
        spans = O.split_records(corpus)
        texts = [corpus[o:o + n] for o, n in spans]
        docnos = [get_docno(ids, get_docid(t)) for t in texts]
        ref = oracle_k1 if oracle_k1 is not None else O.OracleIndex(corpus, mapping, 1, 1)
        space = [t for t in ref.terms() if t[0] == (" ",)]
        if texts:
            posts = space[0][3]
            assert len(posts) == len(texts) and posts[0] == (0, 0)
            assert [p[0] for p in posts[1:]] == docnos[:-1]  # the oracle's own docnos
        self.N = len(texts)
        self.records = [(d, O.process_content(t)) for d, t in zip(docnos, texts)]

    def grams(self, m):
        """{gram tuple: {docno: tf}} of every window of m terms: the reference's K = m index."""
        out = defaultdict(lambda: defaultdict(int))
        for d, s in self.records:
            for i in range(len(s) - m + 1):
                out[tuple(s[i:i + m])][d] += 1
        return {g: dict(p) for g, p in out.items()}

    def match(self, phrase):
        """{docno: freq} of a phrase of term strings (freq > 0 only)."""
        out = defaultdict(int)
        for d, s in self.records:
            c = phrase_count(s, phrase)
            if c:
                out[d] += c
        return dict(out)

    def run(self, phrases, order=0, m=0, idf_mode=0, N=None):
        """The answer of sme_query_phrase for phrases of term strings (None = an
        unknown term): (res_off, docno, freq, score) numpy arrays."""
        N = self.N if N is None else N
        off, dn, fq, sc = [0], [], [], []
        for ph in phrases:
            hits = {} if (not ph or any(t is None for t in ph)) else self.match(ph)
            df = len(hits)
            rows = []
            for d, f in hits.items():
                idf = math.log10(float(N // (1 if idf_mode == 0 else df)))
                rows.append((d, f, (1.0 + math.log(float(f))) * idf))
            rows.sort(key=(lambda r: r[0]) if order == 0 else (lambda r: (-r[2], r[0])))
            if m > 0:
                rows = rows[:m]
            dn += [r[0] for r in rows]
            fq += [r[1] for r in rows]
            sc += [r[2] for r in rows]
            off.append(len(dn))
        return (np.array(off, np.int64), np.array(dn, np.int32), np.array(fq, np.int32), np.array(sc, np.float64))
