"""Wildcard expansion restated in Python, independent of csrc/sme_wild.hpp: the
matcher as a regular expression over strings of UTF-16 units, the trigram
extraction rules from their description in include/sme.h, and the pattern and
term sets test_wild_host.py and test_gpu_wild.py share."""
import random
import re

import numpy as np

START_FLAG, END_FLAG = 1 << 48, 1 << 49


def units(s):
    """UTF-16 units of a str (unpaired surrogates kept)."""
    b = s.encode("utf-16-be", "surrogatepass")
    return [(b[i] << 8) | b[i + 1] for i in range(0, len(b), 2)]


def ustr(s):
    """One character per UTF-16 unit."""
    return "".join(chr(u) for u in units(s))


def unit_key(s):
    """String.compareTo order."""
    return s.encode("utf-16-be", "surrogatepass")


def mutf8(s):
    """DataOutput.writeUTF body."""
    out = bytearray()
    for u in units(s):
        if 1 <= u <= 0x7F:
            out.append(u)
        elif u <= 0x7FF:
            out += bytes([0xC0 | (u >> 6), 0x80 | (u & 0x3F)])
        else:
            out += bytes([0xE0 | (u >> 12), 0x80 | ((u >> 6) & 0x3F), 0x80 | (u & 0x3F)])
    return bytes(out)


def to_re(pattern):
    parts = []
    for ch in ustr(pattern):
        parts.append(".*" if ch == "*" else "." if ch == "?" else re.escape(ch))
    return re.compile("".join(parts), re.DOTALL)


def matches(pattern, terms):
    """Indices of the terms the pattern matches, ascending."""
    rx = to_re(pattern)
    return [i for i, t in enumerate(terms) if rx.fullmatch(ustr(t))]


def expand(patterns, terms):
    """(match_off int64[n+1], term_ids int32), as sme_index_expand_wildcards returns them."""
    off, ids = [0], []
    for p in patterns:
        ids += matches(p, terms)
        off.append(len(ids))
    return np.array(off, np.int64), np.array(ids, np.int32)


def _key(a, b, c):
    """Three entries, None = a boundary: 16 bits per unit, flag bits 48 (START first) / 49 (END last)."""
    k = b << 16
    k |= START_FLAG if a is None else a << 32
    k |= END_FLAG if c is None else c
    return k


def _windows(seq):
    return [_key(seq[i], seq[i + 1], seq[i + 2]) for i in range(len(seq) - 2)]


def term_grams(term):
    u = units(term)
    return _windows([None] + u + [None]) if u else []


def pattern_grams(pattern):
    """Windows inside each maximal literal run; START joins the first run when the
    pattern begins with a literal, END the last run when it ends with one."""
    u = units(pattern)
    meta = [x in (0x2A, 0x3F) for x in u]
    out, i = [], 0
    while i < len(u):
        if meta[i]:
            i += 1
            continue
        j = i
        while j < len(u) and not meta[j]:
            j += 1
        seq = ([None] if i == 0 else []) + u[i:j] + ([None] if j == len(u) else [])
        # a boundary is never a window's middle entry
        out += [_key(seq[x], seq[x + 1], seq[x + 2]) for x in range(len(seq) - 2)]
        i = j
    return out


def table(terms):
    """{key: sorted term ids}."""
    t = {}
    for i, term in enumerate(terms):
        for k in set(term_grams(term)):
            t.setdefault(k, []).append(i)
    return t


def candidates(pattern, tab, V):
    """Candidate count of the table path: the shortest list among the pattern's
    trigrams, 0 if one is absent, V without a trigram."""
    g = pattern_grams(pattern)
    if not g:
        return V
    return min(len(tab.get(k, ())) for k in g)


LONG = "long" * 30  # 120 units
AS = "a" * 60
SUPP = "\U0001F600"

SMALL_TERMS_BASE = [
    "a", "b", "c", "x", "é", "ab", "abc", "abcd", "abcde", "abd", "ac", "abbc", "acb", "axxbyyc", "abcbc", "ing",
    "running", "ringo", "king", "cab", "cabd", "café", "cafe", "straße", "strasse", SUPP, SUPP + "smile", "x" + SUPP,
    LONG, AS, "a" * 59 + "b", "aaab", "aaaa", "apple", "apply", "applesauce", "snapple", "zz", "İstanbul", "σοφία",
]


def small_terms():
    """A few hundred terms in String.compareTo order."""
    rng = random.Random(17)
    words = set(SMALL_TERMS_BASE)
    while len(words) < 340:
        words.add("".join(rng.choice("abcing") for _ in range(rng.randint(1, 9))))
    return sorted(words, key=unit_key)


PATTERNS = [
    "apple", "absent", "abc*", "*ing", "*ab*", "a*b*c", "*", "**", "?", "??", "?*", "*?", "a?c", "???*???", "",
    "z" * 130,  # longer than every term
    "a*a*a*a*b", "a*a*a*a*a", "*a*a*a*", "caf?", "stra?e", "*é", SUPP, "?smile", "??smile", SUPP + "*", "*" + SUPP,
    AS, "a" * 59 + "?", "a" * 61, "?" * 60, "?" * 120, LONG[:-1] + "*", "*" + LONG[1:], "long*long", "appl*", "*appl*",
    "a" * 254 + "*",  # 255 units: accepted
    "*" * 255,
]
TOO_LONG = "a" * 255 + "*"        # 256 units
MALFORMED = b"ab\xff*"

BOUNDARY_TERMS = sorted(["ab", "ab$", "$ab", "\u0000ab", "ab￿", "abab", "xab", "abx", "$", "￿", "a$b"],
                        key=unit_key)
BOUNDARY_PATTERNS = ["ab*", "*ab", "ab", "*ab*", "$*", "*$", "?ab", "ab?", "\u0000*", "*￿", "￿"]


def big_terms(n=20000, seed=5):
    """About n distinct generated terms in String.compareTo order."""
    rng = random.Random(seed)
    words = set()
    while len(words) < n:
        words.add("".join(rng.choice("abcdefghijklmnopqrstuvwxyz0123456789é") for _ in range(rng.randint(1, 12))))
    return sorted(words, key=unit_key)
