"""Best passages (sme_query_passages) restated in plain Python over phrase_ref.Streams
records, with the idf of feedback_ref.Feedback.idf.

Semantics (include/sme.h has the full text).  A query lists term ids; -1 is dropped, a
repeated id keeps its first place, and the j-th distinct id is slot j.  The records of
a docno are the stream records with that docno in file order, numbered rec = 0, 1, ...
A record of n positions has the window starts 0 .. max(0, n - width); the window at s is
[s, min(s + width, n)).  Of a window: mask = OR of 1 << slot over its positions holding a
query term, cover = popcount(mask), hits = the number of such positions, score = the
float sum from 0.0 of idf(slot's term) over the set bits in ascending slot order.  The
best window of a candidate is the first by (score desc, cover desc, hits desc, rec asc,
start asc); a candidate without a record is (rec -1, start 0, len 0, hits 0, mask 0,
score 0.0).  Candidates with cover >= min_cover are kept, in the given order (order 0)
or by (score desc, docno asc) (order 1), and cut to m (0: no cut).

The windows are slid along a record with one counter per slot; test_passage_ref.py holds
that to a brute force which looks at every window on its own."""
import collections

import numpy as np

Row = collections.namedtuple("Row", "rec start len hits mask score")
NO_RECORD = Row(-1, 0, 0, 0, 0, 0.0)
FIELDS = ("res_off", "docno", "rec", "start", "len", "hits", "mask", "score", "win_off", "win_term", "win_slot")
DTYPES = (np.int64, np.int32, np.int32, np.int32, np.int32, np.int32, np.uint64, np.float64, np.int64, np.int32,
          np.int8)
Result = collections.namedtuple("Result", FIELDS)


def slots_of(listed):
    """The distinct ids in listed order, -1 dropped: slot j = result[j]."""
    out = []
    for t in listed:
        t = int(t)
        if t != -1 and t not in out:
            out.append(t)
    return out


def score_of(mask, idfs):
    s = 0.0
    for j, v in enumerate(idfs):
        if mask >> j & 1:
            s = s + v
    return s


def key(row):
    """Ascending = the order that picks the best window."""
    return (-row.score, -bin(row.mask).count("1"), -row.hits, row.rec, row.start)


def best_of_record(slot_at, rec, idfs, width):
    """slot_at: the record's positions as slots (-1: no query term)."""
    n = len(slot_at)
    cnt = [0] * len(idfs)
    hits = mask = 0
    for p in range(min(width, n)):
        j = slot_at[p]
        if j >= 0:
            cnt[j] += 1
            hits += 1
            mask |= 1 << j
    score = score_of(mask, idfs)
    best = Row(rec, 0, min(width, n), hits, mask, score)
    for s in range(1, n - width + 1):
        j = slot_at[s - 1]
        changed = False
        if j >= 0:
            cnt[j] -= 1
            hits -= 1
            if cnt[j] == 0:
                mask &= ~(1 << j)
                changed = True
        j = slot_at[s + width - 1]
        if j >= 0:
            cnt[j] += 1
            hits += 1
            if cnt[j] == 1:
                mask |= 1 << j
                changed = True
        if changed:
            score = score_of(mask, idfs)
        row = Row(rec, s, width, hits, mask, score)
        if key(row) < key(best):
            best = row
    return best


class Ref:
    """fb: feedback_ref.Feedback (its by_docno streams hold term strings); ids: {term
    string: term id} of the index under test."""

    def __init__(self, fb, ids):
        self.fb = fb
        self.name_of = {i: t for t, i in ids.items()}
        self.streams = {d: [[ids[t] for t in s] for s in recs] for d, recs in fb.by_docno.items()}
        self._best = {}

    def idfs(self, slots, idf_mode):
        return [self.fb.idf(self.name_of[t], idf_mode) for t in slots]

    def best(self, slots, docno, width, idf_mode):
        """The best window of one candidate (slots: slots_of's list, as a tuple)."""
        k = (slots, docno, width, idf_mode)
        if k not in self._best:
            recs = self.streams.get(docno)
            if not recs:
                self._best[k] = NO_RECORD
            else:
                at = {t: j for j, t in enumerate(slots)}
                idfs = self.idfs(slots, idf_mode)
                rows = [best_of_record([at.get(t, -1) for t in s], r, idfs, width) for r, s in enumerate(recs)]
                self._best[k] = min(rows, key=key)
        return self._best[k]

    def run(self, queries, width, min_cover=0, order=0, m=0, with_terms=False, idf_mode=0):
        """The answer of sme_query_passages for queries = [(listed ids, candidates)]:
        (Result of numpy arrays, stats dict without "chunk")."""
        cols = [[] for _ in range(7)]
        off, woff, wterm, wslot = [0], [0], [], []
        cands = with_record = positions = kept = 0
        for listed, docnos in queries:
            slots = tuple(slots_of(listed))
            docnos = [int(d) for d in docnos]
            assert all(a < b for a, b in zip(docnos, docnos[1:]))
            rows = []
            for d in docnos:
                cands += 1
                recs = self.streams.get(d)
                if recs:
                    with_record += 1
                    positions += sum(len(s) for s in recs)
                b = self.best(slots, d, width, idf_mode)
                if bin(b.mask).count("1") >= min_cover:
                    rows.append((d, b))
            kept += len(rows)
            if order == 1:
                rows.sort(key=lambda r: (-r[1].score, r[0]))
            if m > 0:
                rows = rows[:m]
            for d, b in rows:
                for c, v in zip(cols, (d,) + tuple(b)):
                    c.append(v)
                if with_terms:
                    at = {t: j for j, t in enumerate(slots)}
                    win = self.streams[d][b.rec][b.start:b.start + b.len] if b.rec >= 0 else []
                    wterm += win
                    wslot += [at.get(t, -1) for t in win]
                    woff.append(len(wterm))
            off.append(len(cols[0]))
        if not with_terms:
            woff = [0]
        arrays = [off] + cols + [woff, wterm, wslot]
        res = Result(*[np.array(a, dt) for a, dt in zip(arrays, DTYPES)])
        return res, {"candidates": cands, "with_record": with_record, "positions": positions, "kept": kept}


def batch(queries):
    """(term_ids int32, q_offsets int64, docnos int32, d_offsets int64) of [(listed, candidates)]."""
    terms, qoff, docs, doff = [], [0], [], [0]
    for listed, docnos in queries:
        terms.extend(int(t) for t in listed)
        qoff.append(len(terms))
        docs.extend(int(d) for d in docnos)
        doff.append(len(docs))
    return np.array(terms, np.int32), np.array(qoff, np.int64), np.array(docs, np.int32), np.array(doff, np.int64)


def brute(streams, slots, docno, width, idfs):
    """One candidate's best window, every window looked at on its own with a set and a
    counter: the independent statement test_passage_ref.py uses."""
    recs = streams.get(docno)
    if not recs:
        return NO_RECORD
    found = []
    for rec, s in enumerate(recs):
        for start in range(max(0, len(s) - width) + 1):
            win = s[start:start + width]
            held = set(win) & set(slots)
            count = collections.Counter(win)
            hits = sum(count[t] for t in held)
            mask = sum(1 << slots.index(t) for t in held)
            score = 0.0
            for j in sorted(slots.index(t) for t in held):
                score = score + idfs[j]
            found.append(Row(rec, start, len(win), hits, mask, score))
    found.sort(key=lambda r: (-r.score, -len([j for j in range(64) if r.mask >> j & 1]), -r.hits, r.rec, r.start))
    return found[0]
