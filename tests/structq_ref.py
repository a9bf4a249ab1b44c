"""Structured queries (include/sme.h, sme_query_structured) restated by composing
the two restatements already held to the oracle chain: near_ref.py for the operator
leaves and bool_ref.py for everything else.

A query is a list of (leaves, excluded) groups, a leaf (term_ids, kind, width):
kind 0 a term, 1 the ordered window #od:width, 2 the unordered window #uw:width.
Operator leaf i of the batch becomes the virtual term V + i: its posting list and
weights are what near_ref.run gives the leaf as a query of its own under order 0
and m 0 (docno ascending, uncut -- so its df is the leaf's over the whole index).
The rest is bool_ref.Ref over the CSR extended by those lists.  Nothing of the
device's filter, narrowing, descriptors or sort is shared."""
import numpy as np

import bool_ref as B
import near_ref as NR


def flatten(queries, V):
    """(Boolean queries over term ids with the operator leaves as V + i, the
    operator leaves in batch order as (term_ids, width, ordered))."""
    ops, out = [], []
    for groups in queries:
        gs = []
        for leaves, excluded in groups:
            ids = []
            for tids, kind, width in leaves:
                if kind == 0:
                    assert len(tids) == 1
                    ids.append(int(tids[0]))
                else:
                    assert kind in (1, 2)
                    ids.append(V + len(ops))
                    ops.append(([int(t) for t in tids], int(width), kind == 1))
            gs.append((ids, bool(excluded)))
        out.append(gs)
    return out, ops


def run(st, csr, queries, order=0, m=0, idf_mode=0, N=None, term_of=None, first_driver=False):
    """((res_off int64, docno int32, score float64), candidates, matches, leaf
    lists) of sme_query_structured over the streams st (phrase_ref.Streams, or
    anything with .records [(docno, [token, ...])] and .N) and the query-side CSR
    csr = (offsets[V+1], docno, w).  term_of: term id -> the token the streams hold
    for it (default: the id itself); id -1 is unknown.  N: the document count of
    the leaves' idf (default st.N).  leaf lists: near_ref's (off, docno, freq,
    score) of the operator leaves."""
    off, docno, w = csr
    V = len(off) - 1
    term_of = term_of or (lambda t: t)
    bq, ops = flatten(queries, V)
    nq = [([None if t < 0 else term_of(t) for t in tids], width, ordered) for tids, width, ordered in ops]
    lists = NR.run(st, nq, 0, 0, idf_mode, N)
    ext_off = np.concatenate([np.asarray(off, np.int64), int(off[-1]) + lists[0][1:]])
    ext_docno = np.concatenate([np.asarray(docno, np.int32), lists[1]])
    ext_w = np.concatenate([np.asarray(w, np.float64), lists[3]])
    res, cands, total = B.Ref(ext_off, ext_docno, ext_w).run(bq, order, m, first_driver)
    return res, cands, total, lists
