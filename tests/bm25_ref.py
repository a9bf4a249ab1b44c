"""BM25 ranking restated in numpy and math.log (include/sme.h, sme_query_topk_bm25):
document lengths, D, L, the weights and the top k by (-score, docno) over a term CSR
in docno order.  Every operation is one IEEE fp64 operation in the association the
header gives, so the bits are the contract's; idf comes from math.log, the host libm.
Inputs come from Index.csr() (reduce order, re-sorted per term by docno here), never
from the BM25 entries."""
import math

import numpy as np


def idf_value(D, df):
    return math.log(1.0 + ((float(D - df) + 0.5) / (float(df) + 0.5)))


def doc_norm(k1, b, dl, avgdl):
    return k1 * ((1.0 - b) + b * (float(dl) / avgdl))


def weight(idf, tf, k1, norm):
    return idf * ((float(tf) * (k1 + 1.0)) / (float(tf) + norm))


def bound_term(idf, maxtf, k1, b, mindl, avgdl):
    """What a posting of a term adds at most where no tf exceeds maxtf and no document
    is shorter than mindl."""
    return weight(idf, maxtf, k1, doc_norm(k1, b, mindl, avgdl))


def bits(x):
    return int(np.float64(x).view(np.int64)) & 0xFFFFFFFFFFFFFFFF


class Ref:
    def __init__(self, off, dn, tf):
        """off[V+1], dn[P], tf[P]: every term's postings in docno-ascending order."""
        self.off = np.asarray(off, np.int64)
        self.dn = np.asarray(dn, np.int64)
        self.tf = np.asarray(tf, np.int64)
        self.V = len(self.off) - 1
        for t in range(self.V):
            assert np.all(np.diff(self.dn[self.off[t]:self.off[t + 1]]) > 0)
        P = len(self.dn)
        self.dmin = int(self.dn.min()) if P else 0
        self.span = int(self.dn.max()) - self.dmin + 1 if P else 0
        self.dl = np.zeros(self.span, np.int64)
        np.add.at(self.dl, self.dn - self.dmin, self.tf)
        self.D = int(np.count_nonzero(self.dl))
        self.L = int(self.dl.sum())
        self.avgdl = float(self.L) / float(self.D) if self.D else 0.0
        self.df = np.diff(self.off)
        self.idf = np.array([idf_value(self.D, int(d)) for d in self.df], np.float64)
        self._cache, self._order = {}, {}

    @classmethod
    def from_csr(cls, csr):
        """From Index.csr(): (offsets, docno, tf, df) in reduce order (tf desc, docno asc)."""
        off, dn, tf = csr[0], csr[1].copy(), csr[2].copy()
        for t in range(len(off) - 1):
            a, e = int(off[t]), int(off[t + 1])
            o = np.argsort(dn[a:e], kind="stable")
            dn[a:e], tf[a:e] = dn[a:e][o], tf[a:e][o]
        return cls(off, dn, tf)

    def doc_length(self, docno):
        i = docno - self.dmin
        return int(self.dl[i]) if 0 <= i < self.span else 0

    def scores(self, terms, k1, b):
        """(docnos ascending, scores) of the documents holding at least one of the
        terms: the fp64 sum from 0.0 over the slots in listed order."""
        key = (tuple(int(t) for t in terms), k1, b)
        if key in self._cache:
            return self._cache[key]
        acc = np.zeros(self.span, np.float64)
        hit = np.zeros(self.span, bool)
        if self.D:
            norm = k1 * ((1.0 - b) + b * (self.dl.astype(np.float64) / self.avgdl))
            for t in key[0]:
                if t < 0:
                    continue
                a, e = int(self.off[t]), int(self.off[t + 1])
                at = self.dn[a:e] - self.dmin
                tf = self.tf[a:e].astype(np.float64)
                acc[at] = acc[at] + self.idf[t] * ((tf * (k1 + 1.0)) / (tf + norm[at]))
                hit[at] = True
        at = np.nonzero(hit)[0]
        out = (at + self.dmin, acc[at])
        self._cache[key] = out
        return out

    def topk(self, terms, k, k1=1.2, b=0.75):
        """(docno int32[k], score float64[k]): score descending, then docno ascending,
        padded with -1 / 0.0."""
        dn, sc = self.scores(terms, k1, b)
        key = (tuple(int(t) for t in terms), k1, b)
        if key not in self._order:
            self._order[key] = np.lexsort((dn, -sc))
        o = self._order[key][:k]
        od, os = np.full(k, -1, np.int32), np.zeros(k, np.float64)
        od[:len(o)], os[:len(o)] = dn[o], sc[o]
        return od, os

    def run(self, term_ids, q_offsets, k, k1=1.2, b=0.75):
        nq = len(q_offsets) - 1
        od, os = np.zeros((nq, k), np.int32), np.zeros((nq, k), np.float64)
        for q in range(nq):
            od[q], os[q] = self.topk(term_ids[q_offsets[q]:q_offsets[q + 1]], k, k1, b)
        return od, os


def batch(queries):
    """(term_ids int32, q_offsets int64) of a list of term-id lists."""
    off = np.zeros(len(queries) + 1, np.int64)
    off[1:] = np.cumsum([len(q) for q in queries]) if queries else []
    ids = np.array([t for q in queries for t in q], np.int32)
    return ids, off
