"""Scoring given documents restated in numpy (include/sme.h, sme_query_rescore): per
query a list of term slots and a strictly ascending list of docnos -> every listed
document's hits and score, the matches (hits >= min_hits), both orders and the cut.
BM25 goes through bm25_ref.Ref -- its tables and its one-operation-at-a-time
expression --, TF-IDF through Index.weights(), the docno-ordered (off, docno, w): the
fp64 sum from 0.0 over the slots in listed order, one IEEE addition per slot."""
import numpy as np

MODELS = {"tfidf": 0, "bm25": 1, 0: 0, 1: 1}


class Ref:
    def __init__(self, bm, weights):
        """bm: a bm25_ref.Ref of the index; weights: Index.weights()."""
        self.bm = bm
        self.off = np.asarray(weights[0], np.int64)
        self.dn = np.asarray(weights[1], np.int64)
        self.w = np.asarray(weights[2], np.float64)
        assert np.array_equal(self.off, bm.off) and np.array_equal(self.dn, bm.dn)
        self._cache = {}

    def dense(self, terms, model, k1=1.2, b=0.75):
        """(hits int32[span], score float64[span]) of every docno dmin + i of the
        index's docno range."""
        model = MODELS[model]
        key = (tuple(int(t) for t in terms), model) + ((k1, b) if model else ())
        if key in self._cache:
            return self._cache[key]
        bm = self.bm
        acc = np.zeros(bm.span, np.float64)
        hits = np.zeros(bm.span, np.int32)
        norm = None
        if model and bm.D:
            norm = k1 * ((1.0 - b) + b * (bm.dl.astype(np.float64) / bm.avgdl))
        for t in key[0]:
            if t < 0:
                continue
            a, e = int(self.off[t]), int(self.off[t + 1])
            at = self.dn[a:e] - bm.dmin
            if model:
                tf = bm.tf[a:e].astype(np.float64)
                acc[at] = acc[at] + bm.idf[t] * ((tf * (k1 + 1.0)) / (tf + norm[at]))
            else:
                acc[at] = acc[at] + self.w[a:e]
            hits[at] += 1
        self._cache[key] = (hits, acc)
        return hits, acc

    def score(self, terms, docs, model, k1=1.2, b=0.75):
        """(hits int32[len(docs)], score float64[len(docs)]) of the listed docnos; one
        the index has never seen has hits 0 and score 0.0."""
        docs = np.asarray(docs, np.int64)
        hd, sd = self.dense(terms, model, k1, b)
        i = docs - self.bm.dmin
        inside = (i >= 0) & (i < self.bm.span)
        hits, sc = np.zeros(len(docs), np.int32), np.zeros(len(docs), np.float64)
        hits[inside], sc[inside] = hd[i[inside]], sd[i[inside]]
        return hits, sc

    def rank(self, terms, docs, model, order=1, m=0, min_hits=0, k1=1.2, b=0.75):
        """(docno int32, hits int32, score float64) of one query."""
        docs = np.asarray(docs, np.int64)
        assert np.all(np.diff(docs) > 0)
        hits, sc = self.score(terms, docs, model, k1, b)
        keep = np.nonzero(hits >= min_hits)[0]
        if order == 1:
            keep = keep[np.lexsort((docs[keep], -sc[keep]))]
        if m > 0:
            keep = keep[:m]
        return docs[keep].astype(np.int32), hits[keep], sc[keep]

    def run(self, queries, model, order=1, m=0, min_hits=0, k1=1.2, b=0.75):
        """queries: [(terms, docs)] -> (res_off int64[nq+1], docno, hits, score)."""
        parts = [self.rank(t, d, model, order, m, min_hits, k1, b) for t, d in queries]
        off = np.zeros(len(queries) + 1, np.int64)
        if parts:
            off[1:] = np.cumsum([len(p[0]) for p in parts])
        cat = [np.concatenate([p[c] for p in parts]) if parts else np.zeros(0) for c in range(3)]
        return off, cat[0].astype(np.int32), cat[1].astype(np.int32), cat[2].astype(np.float64)


def batch(queries):
    """(term_ids int32, q_offsets int64, docnos int32, d_offsets int64) of [(terms, docs)]."""
    qoff, doff = np.zeros(len(queries) + 1, np.int64), np.zeros(len(queries) + 1, np.int64)
    if queries:
        qoff[1:] = np.cumsum([len(t) for t, _ in queries])
        doff[1:] = np.cumsum([len(d) for _, d in queries])
    ids = np.array([x for t, _ in queries for x in t], np.int32)
    docs = np.concatenate([np.asarray(d, np.int32) for _, d in queries]) if queries else np.zeros(0, np.int32)
    return ids, qoff, docs.astype(np.int32), doff
