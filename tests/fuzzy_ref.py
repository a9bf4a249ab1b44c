"""Spelling suggestions restated in Python, independent of csrc/sme_fuzzy.hpp: the
plain dynamic-programming Levenshtein distance over UTF-16 units (one word
against a whole vocabulary at a time, numpy over a padded term matrix), the
ordering rule (distance asc, df desc, term id asc) with the cut, the "distinct
keys / needs scan" rule from its description in include/sme.h, and the word sets
test_fuzzy_host.py and test_gpu_fuzzy.py share.  Term sets: wild_ref.py."""
import random

import numpy as np

import wild_ref as W


def lev(a, b):
    """Levenshtein distance of two unit lists: insert, delete, substitute at cost 1."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


class Vocab:
    """Terms as a padded matrix of units (pad -1, which equals no unit)."""

    def __init__(self, terms):
        us = [W.units(t) for t in terms]
        self.len = np.array([len(u) for u in us], np.int64)
        self.mat = np.full((len(us), max([1] + [len(u) for u in us])), -1, np.int64)
        for i, u in enumerate(us):
            self.mat[i, :len(u)] = u

    def distances(self, word, within=None):
        """The word's distance to every term: the DP row by row, every term at once
        (cur[j] = min(a[j], cur[j-1] + 1) unrolls to a running minimum of a[k] - k).
        within = k: only terms whose length differs from the word's by at most k
        go through the DP; the others report that difference, a lower bound of
        their distance that is itself past k."""
        u = W.units(word)
        out = np.abs(self.len - len(u))
        rows = np.arange(len(out)) if within is None else np.nonzero(out <= within)[0]
        if not len(rows):
            return out
        L = int(self.len[rows].max())
        mat, ar = self.mat[rows][:, :L], np.arange(L + 1, dtype=np.int64)
        prev = np.tile(ar, (len(rows), 1))
        for i, x in enumerate(u, 1):
            a = np.empty_like(prev)
            a[:, 0] = i
            a[:, 1:] = np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (mat != x))
            prev = np.minimum.accumulate(a - ar, axis=1) + ar
        out[rows] = prev[np.arange(len(rows)), self.len[rows]]
        return out


def ranked(dist, df, max_dist):
    """[(term id, distance)] within max_dist, ordered (distance asc, df desc, id asc)."""
    hit = np.nonzero(dist <= max_dist)[0]
    order = sorted(hit.tolist(), key=lambda t: (int(dist[t]), -int(df[t]), t))
    return [(t, int(dist[t])) for t in order]


def suggest(words, vocab, df, max_dist, m, cache=None):
    """(sug_off int64[n+1], term_ids int32, dist uint8), as sme_index_suggest_terms
    returns them (max_dist <= 3: terms more than 4 units longer or shorter than
    the word skip the DP).  cache: {word: distances}, filled as it goes."""
    off, ids, ds = [0], [], []
    for w in words:
        if cache is not None and w in cache:
            dist = cache[w]
        else:
            dist = vocab.distances(w, within=4)
            if cache is not None:
                cache[w] = dist
        r = ranked(dist, df, max_dist)
        if m:
            r = r[:m]
        ids += [t for t, _ in r]
        ds += [d for _, d in r]
        off.append(len(ids))
    return np.array(off, np.int64), np.array(ids, np.int32), np.array(ds, np.uint8)


def distinct_keys(word):
    """The word's windows as a term's (START + units + END), deduplicated."""
    return set(W.term_grams(word))


def needs_scan(word, max_dist):
    """Fewer than 3d + 1 distinct keys: the word takes the whole vocabulary."""
    return len(distinct_keys(word)) < 3 * max_dist + 1


def chosen_lists(word, tab, max_dist):
    """The posting lists of the 3d + 1 distinct keys with the shortest lists."""
    lists = sorted((tab.get(k, []) for k in distinct_keys(word)), key=len)
    return lists[:3 * max_dist + 1]


def df_of(i):
    """Posting count the device tests give term i."""
    return 1 + (7 * i) % 5


def edits_of(t):
    """One substitution, insertion and deletion at the first, middle and last unit."""
    n = len(t)
    out = []
    for p in (0, n // 2, n - 1):
        out += [t[:p] + "q" + t[p + 1:], t[:p] + "q" + t[p:], t[:p] + t[p + 1:]]
    out.append(t + "q")  # insertion after the last unit
    return out


# a word at distance exactly k from its nearest term of small_terms() (the tests
# assert that on the reference): "applesauce" with k units replaced
FAR = {1: "Qpplesauce", 2: "QpplQsauce", 3: "QpplQsauQe", 4: "QpQlQsauQe"}

WORDS = (["apple", "running", "café", W.SUPP, W.AS, "ing", "zz"]
         + edits_of("apple") + edits_of("running") + edits_of("café")
         + ["apply", "appel", W.SUPP, W.SUPP + "smil", W.SUPP + "smiles", "\ud83d", "x" + W.SUPP + "y",
            "a" * 64, "a" * 61, "a" * 59, "", "a", "ab", "abc", "aaaa", "abababab", "a*c", "a?c", "*", "?",
            "strase", "İstanbu", "σοφα",
            "applesauce", "applesauces", "xapplesauce", "snapplesauce"]
         + [FAR[k] for k in sorted(FAR)])
WORDS = list(dict.fromkeys(WORDS))  # each word once, order kept
TOO_LONG = "a" * 65
MALFORMED = b"ab\xffc"

BOUNDARY_WORDS = ["ab", "$ab", "ab$", "\u0000ab", "ab\uffff"]


def random_edit(rng, s, alphabet):
    r = rng.random()
    p = rng.randrange(len(s) + 1)
    if r < 1 / 3 and s:
        p = min(p, len(s) - 1)
        return s[:p] + rng.choice(alphabet) + s[p + 1:]
    if r < 2 / 3 and s:
        p = min(p, len(s) - 1)
        return s[:p] + s[p + 1:]
    return s[:p] + rng.choice(alphabet) + s[p:]


def big_words(terms, seed=11, n_edit=40, n_random=8):
    """n_edit terms of at least 8 units with 1..3 seeded random edits (kept at 7 or
    more units, so they have at least 7 windows), and n_random random strings."""
    rng = random.Random(seed)
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789é"
    long_terms = [t for t in terms if len(W.units(t)) >= 8]
    out = []
    while len(out) < n_edit:
        w = rng.choice(long_terms)
        for _ in range(rng.randint(1, 3)):
            w = random_edit(rng, w, alphabet)
        if len(w) >= 7:
            out.append(w)
    for _ in range(n_random):
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(8, 12))))
    return out
