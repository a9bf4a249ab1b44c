"""Boolean retrieval restated in plain Python (include/sme.h, sme_query_boolean):
what the device tests hold libsme's results to.  It works over the query-side
CSR as Index.weights() returns it -- offsets, docno-ascending postings, fp64
weights -- with Python sets for membership and a Python-float loop in listed
slot order for the score, so nothing of the device's search or sort is shared.

A query is a list of (term_ids, excluded) groups.  A document matches when every
required group holds it in at least one of its lists and no excluded group does;
a query without a required group, or with a required group without a posting,
matches nothing.  Term id -1 is an empty list."""
import numpy as np

MAX_GROUPS, MAX_SLOTS = 64, 1024


class Ref:
    def __init__(self, off, docno, w):
        self.off = [int(x) for x in off]
        self.docno = [int(x) for x in docno]
        self.w = [float(x) for x in w]
        self._sets, self._maps, self._memo = {}, {}, {}

    def count(self, t):
        return 0 if t < 0 else self.off[t + 1] - self.off[t]

    def docs(self, t):
        """The documents of term t's posting list (a set)."""
        if t not in self._sets:
            self._sets[t] = set() if t < 0 else set(self.docno[self.off[t]:self.off[t + 1]])
        return self._sets[t]

    def weight_of(self, t):
        """docno -> weight of term t's postings."""
        if t not in self._maps:
            a, b = (0, 0) if t < 0 else (self.off[t], self.off[t + 1])
            self._maps[t] = dict(zip(self.docno[a:b], self.w[a:b]))
        return self._maps[t]

    def driver(self, groups, first=False):
        """(index of the driver group, its postings): the required group with the
        fewest postings, ties to the lowest index (first: the first required
        group); None when the query matches nothing by its structure."""
        req = [(sum(self.count(t) for t in ids), g) for g, (ids, ex) in enumerate(groups) if not ex]
        if not req or any(c == 0 for c, _ in req):
            return None
        c, g = req[0] if first else min(req)
        return g, c

    def matches(self, groups):
        """{docno: score} of one query (computed once per distinct query)."""
        key = tuple((tuple(ids), bool(ex)) for ids, ex in groups)
        if key not in self._memo:
            self._memo[key] = self._matches(groups)
        return dict(self._memo[key])

    def _matches(self, groups):
        req =[set().union(*[self.docs(t) for t in ids]) for ids, ex in groups if not ex]
        if not req or any(not s for s in req):
            return {}
        hit = set.intersection(*req)
        for ids, ex in groups:
            if ex:
                for t in ids:
                    hit = hit - self.docs(t)
        out = {}
        for d in hit:
            s = 0.0
            for ids, ex in groups:
                if ex:
                    continue
                for t in ids:
                    wt = self.weight_of(t).get(d)
                    if wt is not None:
                        s = s + wt
            out[d] = s
        return out

    def run(self, queries, order=0, m=0, first_driver=False):
        """((res_off int64, docno int32, score float64), candidates, matches):
        the batch's results ordered and cut, the driver postings and the matches
        before the cut."""
        off, dn, sc = [0], [], []
        cands = total = 0
        for groups in queries:
            drv = self.driver(groups, first_driver)
            if drv is not None:
                cands += drv[1]
            res = self.matches(groups)
            total += len(res)
            rows = sorted(res.items(), key=(lambda r: (-r[1], r[0])) if order == 1 else (lambda r: r[0]))
            if m > 0:
                rows = rows[:m]
            dn.extend(d for d, _ in rows)
            sc.extend(s for _, s in rows)
            off.append(len(dn))
        return (np.array(off, np.int64), np.array(dn, np.int32), np.array(sc, np.float64)), cands, total
