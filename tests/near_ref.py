"""Proximity queries restated by brute force over phrase_ref.Streams' per-record
term streams (include/sme.h has the two definitions).

Ordered window (#od:N): a memoised existence search -- reach(j, p) iff the stream
holds term j at p and, for j > 0, some q in [p - N, p - 1] has reach(j - 1, q);
the count is the number of p with reach(L - 1, p).  Unordered window (#uw:N): the
positions e on a query term whose slice [max(0, e - N + 1), e] holds every
distinct term, by set containment.  Neither knows tiles or carries.

test_near_ref.py holds this file to the oracle chain through phrase_ref: ordered
N = 1 is Streams.match."""
import math
from collections import defaultdict

import numpy as np


def where(stream):
    """{term: its positions in the stream, ascending}."""
    out = defaultdict(list)
    for p, t in enumerate(stream):
        out[t].append(p)
    return out


def count_ordered(stream, terms, N, at=None):
    """at: where(stream), if the caller has it (only positions holding the level's
    own term can be reachable, so only those are asked)."""
    L = len(terms)
    if L == 0 or N < 1:
        return 0
    at = where(stream) if at is None else at

    memo = {}

    def reach(j, p):  # (p holds terms[j])
        if j == 0:
            return True
        r = memo.get((j, p))
        if r is None:
            r = memo[j, p] = any(reach(j - 1, q) for q in at.get(terms[j - 1], ()) if p - N <= q < p)
        return r

    return sum(1 for p in at.get(terms[L - 1], ()) if reach(L - 1, p))


def count_unordered(stream, terms, N):
    T = set(terms)
    if not T or N < 1:
        return 0
    stream = list(stream)
    return sum(1 for e in range(len(stream)) if stream[e] in T and T <= set(stream[max(0, e - N + 1):e + 1]))


def count(stream, terms, N, ordered):
    return count_ordered(stream, terms, N) if ordered else count_unordered(stream, terms, N)


def match(st, terms, N, ordered):
    """{docno: freq} of one query over st.records (freq > 0 only)."""
    ats = getattr(st, "_near_where", None)
    if ats is None:
        ats, st._near_hits = [where(s) for _, s in st.records], {}
        st._near_where = ats
    key = (tuple(terms), N, bool(ordered))
    if key not in st._near_hits:  # (the tests ask the same query under several orders and cuts)
        out = defaultdict(int)
        need = set(terms)
        for (d, s), at in zip(st.records, ats):
            if all(t in at for t in need):  # (a record without one of the terms matches neither kind)
                c = count_ordered(s, terms, N, at) if ordered else count_unordered(s, terms, N)
                if c:
                    out[d] += c
        st._near_hits[key] = dict(out)
    return dict(st._near_hits[key])


def run(st, queries, order=0, m=0, idf_mode=0, N=None):
    """The answer of sme_query_near for queries (terms, width, ordered) of term
    strings (None = an unknown term) over the phrase_ref.Streams st: (res_off,
    docno, freq, score) numpy arrays, like Streams.run."""
    N = st.N if N is None else N
    off, dn, fq, sc = [0], [], [], []
    for terms, width, ordered in queries:
        hits = {} if (not terms or any(t is None for t in terms)) else match(st, list(terms), width, ordered)
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
