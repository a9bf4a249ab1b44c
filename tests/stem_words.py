"""Deterministic word lists that reach every rule of the Porter2 stemmer, and a
corpus in which many raw forms share one term, for the four device stemmer paths
(csrc/sme_stem.hpp through vocab_clean, vocab_one in k_vocab, k_vocab_long and
k_tokenize_one).  Pure Python except families(), which asks the CPU oracle which
forms share a stem.

  Meter             pyref_tokenize.EnglishStemmer with its among lookups and steps
                    observed (the restatement itself is not changed): which table
                    entries match, whether steps 2-5 then change the word, and the
                    named conditions of NAMED
  rule_words()      a product of fixed stem and suffix lists plus the exception
                    words: lower-case letters, a few words with digits
  covering_subset() a greedy subset of rule_words() that keeps every event
  length_edges()    one word per applying rule of steps 1b-5 behind a consonant
                    run, at the raw lengths where the device switches path
  family_corpus()   bases x suffixes kept where the oracle stems the form to the
                    base's stem, spelled lower / Capitalised / UPPER, in records
                    that put many forms of one term into one posting

The switches restated here (change both together): vocab_clean takes clean
[a-z0-9] raw tokens of at most CLEAN_MAX bytes, k_vocab every other raw token up
to SHORT_RAW bytes, k_vocab_long the rest; TagTokenizer.addToken drops a token
of 100 bytes or more.
"""
import functools
import re
import struct

import pyref_tokenize as P

CLEAN_MAX = 48    # vocab_clean: len > 48 leaves the LDS fast path
SHORT_RAW = 200   # kShortRaw: longer raw tokens go to k_vocab_long
DROP_LEN = 100    # addToken: tokens of >= 100 bytes are dropped

TABLES = {"A_0": P.A_0, "A_1": P.A_1, "A_2": P.A_2, "A_3": P.A_3, "A_4": P.A_4, "A_5": P.A_5, "A_6": P.A_6,
          "A_7": P.A_7, "A_8": P.A_8, "A_9": P.A_9, "A_10": P.A_10}
_NAME = {id(v): k for k, v in TABLES.items()}
ENTRIES = {k: [P.ustr(e[0]) for e in v] for k, v in TABLES.items()}
STEP_TABLES = ("A_5", "A_6", "A_7", "A_8")  # steps 2, 3, 4, 5

NAMED = (
    "r1_prefix_gener", "r1_prefix_commun", "r1_prefix_arsen", "r1_scan", "p1_eq_limit", "p2_eq_limit",
    "shortv_1b_true", "shortv_1b_false", "shortv_5_true", "shortv_5_false",
    "1b_undouble", "1b_e_after_at", "1b_e_after_bl", "1b_e_after_iz",
    "1a_ie", "1a_i", "1a_s_deleted", "1a_s_kept",
    "2_ogi_after_l", "2_ogi_no_l", "2_li_valid", "2_li_invalid",
    "4_ion_after_s", "4_ion_after_t", "4_ion_after_other", "5_l_after_l", "5_l_not_after_l",
    "exc2_after_1a", "exc1_whole", "exc1_prefix",
    "Y_initial", "Y_after_vowel", "postlude_Y_back", "1c_applied", "1c_declined",
    "len_1", "len_2", "len_3",
)


class Meter(P.EnglishStemmer):
    """The restatement, observed.  events(word) -> (stem, frozenset of events): an
    event is ("among", table, entry), ("step", table, entry, "apply" | "decline")
    and ("why", table, entry, "r1" | "r2" | "cond") for steps 2-5, or one of NAMED."""

    def events(self, word):
        self.ev = set()
        self._last = {}
        self._in = None
        u = P.units(word)
        self._orig = list(u)
        if 1 <= len(u) <= 3:
            self.ev.add("len_%d" % len(u))
        out = P.ustr(self.stem(u))
        return out, frozenset(self.ev)

    # ---- among lookups
    def _hit(self, v, consumed):
        name, entry = _NAME[id(v)], P.ustr(consumed)
        assert entry in ENTRIES[name]
        self.ev.add(("among", name, entry))
        self._last[name] = entry

    def find_among(self, v):
        c0 = self.cursor
        r = super().find_among(v)
        if r != 0:
            self._hit(v, self.cur[c0:self.cursor])
        return r

    def find_among_b(self, v):
        c0 = self.cursor
        r = super().find_among_b(v)
        if r != 0:
            self._hit(v, self.cur[self.cursor:c0])
        return r

    def _observed(self, table, fn):
        """Run one step: (its result, the word before, the entry of `table` it matched or None)."""
        self._last.pop(table, None)
        before = list(self.cur)
        self._in = table
        r = fn()
        self._in = None
        return r, before, self._last.get(table)

    def _outcome(self, table, before, e):
        """apply / decline, and of a decline its reason: the suffix lies before R1
        ("r1"), inside R1 but before R2 where the rule asks for R2 ("r2"), or the
        rule's own condition on the letter before it failed ("cond")."""
        if e is None:
            return
        if self.cur != before:
            self.ev.add(("step", table, e, "apply"))
            return
        self.ev.add(("step", table, e, "decline"))
        pos = len(before) - len(e)
        if self.p1 > pos:
            why = "r1"
        elif self.p2 > pos and (table in ("A_7", "A_8") or (table, e) == ("A_6", "ative")):
            why = "r2"
        else:
            why = "cond"
        self.ev.add(("why", table, e, why))

    # ---- regions, short syllables
    def r_mark_regions(self):
        self._last.pop("A_0", None)
        r = super().r_mark_regions()
        e = self._last.get("A_0")
        if e is not None:
            self.ev.add("r1_prefix_" + e)
        elif self.p1 < self.limit:
            self.ev.add("r1_scan")
        if self.p1 == self.limit:
            self.ev.add("p1_eq_limit")
        if self.p2 == self.limit:
            self.ev.add("p2_eq_limit")
        return r

    def r_shortv(self):
        r = super().r_shortv()
        where = {"A_4": "1b", "A_8": "5"}.get(self._in)
        if where:
            self.ev.add("shortv_%s_%s" % (where, "true" if r else "false"))
        return r

    # ---- prelude / postlude
    def r_prelude(self):
        r = super().r_prelude()
        if self.cur[:1] == [ord("Y")]:
            self.ev.add("Y_initial")
        if ord("Y") in self.cur[1:]:
            self.ev.add("Y_after_vowel")
        return r

    def r_postlude(self):
        before = list(self.cur)
        r = super().r_postlude()
        if self.cur != before:
            self.ev.add("postlude_Y_back")
        return r

    # ---- exceptions
    def r_exception1(self):
        self._last.pop("A_10", None)
        r = super().r_exception1()
        if self._last.get("A_10") is not None:
            self.ev.add("exc1_whole" if r else "exc1_prefix")
        return r

    def r_exception2(self):
        r = super().r_exception2()
        if r and self.cur != self._orig:
            self.ev.add("exc2_after_1a")
        return r

    # ---- steps
    def r_step_1a(self):
        r, before, e = self._observed("A_2", super().r_step_1a)
        if e in ("ies", "ied"):
            self.ev.add("1a_ie" if len(self.cur) == len(before) - 1 else "1a_i")
        if e == "s":
            self.ev.add("1a_s_deleted" if self.cur != before else "1a_s_kept")
        return r

    def r_step_1b(self):
        self._last.pop("A_3", None)
        r, before, e = self._observed("A_4", super().r_step_1b)
        e3 = self._last.get("A_3")
        if e3 in ("at", "bl", "iz"):
            self.ev.add("1b_e_after_" + e3)
        elif e3:
            self.ev.add("1b_undouble")
        return r

    def r_step_1c(self):
        before = list(self.cur)
        r = super().r_step_1c()
        if before[-1:] in ([ord("y")], [ord("Y")]):
            self.ev.add("1c_applied" if self.cur != before else "1c_declined")
        return r

    def r_step_2(self):
        r, before, e = self._observed("A_5", super().r_step_2)
        self._outcome("A_5", before, e)
        if e is not None and self.p1 <= len(before) - len(e):
            prev = before[len(before) - len(e) - 1]
            if e == "ogi":
                self.ev.add("2_ogi_after_l" if prev == ord("l") else "2_ogi_no_l")
            if e == "li":
                self.ev.add("2_li_valid" if self.cur != before else "2_li_invalid")
        return r

    def r_step_3(self):
        r, before, e = self._observed("A_6", super().r_step_3)
        self._outcome("A_6", before, e)
        return r

    def r_step_4(self):
        r, before, e = self._observed("A_7", super().r_step_4)
        self._outcome("A_7", before, e)
        if e == "ion" and self.p2 <= len(before) - 3:
            prev = chr(before[len(before) - 4])
            self.ev.add("4_ion_after_" + (prev if prev in "st" else "other"))
        return r

    def r_step_5(self):
        r, before, e = self._observed("A_8", super().r_step_5)
        self._outcome("A_8", before, e)
        if e == "l" and self.p2 <= len(before) - 1:
            self.ev.add("5_l_after_l" if before[-2:-1] == [ord("l")] else "5_l_not_after_l")
        return r


# ---------------------------------------------------------------------------
# the covering list
# ---------------------------------------------------------------------------
# stems: none and single consonants (every suffix before R1), one syllable (before
# R2), two and more (inside R2); the last letters that step 1b undoubles, that the
# li rule accepts and rejects, s / t / other before ion, l before ogi; the A_0
# prefixes; y first and after a vowel
STEMS = (
    "", "n", "t", "tr", "str", "br",
    "hop", "sit", "run", "bat", "fil", "trip", "bid", "beg", "rub", "hug", "dim", "fit", "stir", "ebb", "add",
    "egg", "err", "stiff", "inn", "fear", "need", "deep", "slow", "box", "quick", "rich", "calm", "pac", "vag",
    "conflat", "relat", "troubl", "disabl", "organiz", "siz",
    "connect", "adjust", "nation", "oper", "organ", "depend", "effect", "direct", "general", "control", "controll",
    "enroll", "parallel", "hope", "care", "use", "achiev", "believ", "replac", "form", "ration", "condit", "sens",
    "act", "decis", "electr", "duplic", "inform", "differ", "adopt", "confus", "opin", "relig", "geol", "pedag",
    "anal", "gener", "commun", "arsen", "generat", "communic", "arsenic",
    "play", "enjoy", "say", "obey", "yield", "young", "yell", "happ", "cr", "cit", "p", "d", "appl",
)

_Y_OF = ("anci", "enci", "ogi", "li", "bli", "abli", "alli", "fulli", "lessli", "ousli", "entli", "aliti", "biliti",
         "iviti", "iciti", "iti")
SUFFIXES = tuple(dict.fromkeys(
    # the table entries themselves
    [e for t in ("A_2", "A_4", "A_5", "A_6", "A_7", "A_8") for e in ENTRIES[t]]
    # their -y spellings (step 1c turns the y into i first), plurals of those
    + [e[:-1] + "y" for e in _Y_OF] + [e + "es" for e in _Y_OF]
    # steps 1a and 1b over the derivational endings; chains through steps 2-4
    + ["es", "y", "ying", "ily", "iness", "ier", "ll", "lly", "ee", "er", "ers", "ering", "ered"]
    + ["ations", "ational", "ationally", "ationalize", "ationalism", "ationalization", "ationed", "ationing",
       "tionally", "tionalize", "tionalism", "tionals", "tioned", "tioning",
       "izations", "izational", "izers", "ized", "izing", "izes", "izingly", "izedly", "izable", "izability",
       "ators", "ated", "ating", "ates", "atingly", "atedly",
       "ative", "atives", "atively", "ativeness", "ativity", "ativism",
       "alisms", "alist", "alistic", "alities", "alize", "alized", "alizing", "alizes", "alization", "alizer",
       "alness", "als",
       "fulnesses", "fulnes", "fuls", "lessness", "lessnesses", "ousnesses", "ivenesses", "ively", "ives", "ivities",
       "ables", "ableness", "ability", "abilities", "ibly", "ibility", "ibilities", "ibles",
       "icates", "icated", "icating", "ication", "ications", "icative", "icator", "icity", "icities", "icals",
       "ically", "icalness", "ics", "icism", "icist", "icize",
       "ances", "ancies", "ences", "encies", "antly", "ants", "ents", "ently", "ements", "ments", "mental",
       "mentally", "ions", "ional", "ionally", "isms", "ists", "ities", "ousli", "ously",
       "nesses", "nessless", "fully", "fulli", "lessly", "logi", "logy", "logies", "logic", "logical", "logist",
       "ology", "ologi", "ologies",
       "eeds", "eeding", "eeded", "edness", "ingness", "ings", "eds"]))

# stems whose last letter step 1b undoubles: the doubled spellings
_DOUBLING = ("ed", "ing", "edly", "ingly", "er", "ers")
EXCEPTION_ENDINGS = ("", "s", "es", "ed", "ing", "ly", "ness", "like", "x")
DIGIT_WORDS = ("7", "42", "7x", "qz", "x9", "abc1ing", "9ational", "ational9", "abc1ed", "a1b2ization", "hop3ing",
               "9ness", "ness9", "connect1ons", "4generously", "gener8", "y2y", "1ying", "sky9", "9sky", "ies9",
               "2ties", "r2d2s", "b52s", "mp3ed", "i18n", "l10nal", "k9li", "x86ly", "3ational", "3ation5")
SHORT_WORDS = ("qz", "xq", "zz", "ab", "ox", "aah", "ski", "sky", "tie", "die", "lie", "ies", "ied", "eed", "ing",
               "bli", "ogi", "yes", "yet", "ply", "dry", "shy", "bye", "gas", "bus", "his", "yay", "say", "ate", "ion")


@functools.lru_cache(maxsize=None)
def rule_words():
    """The covering list: STEMS x SUFFIXES, the doubled spellings, the exception
    words alone and before an ending, short words and words with digits."""
    out = []
    for st in STEMS:
        for sf in SUFFIXES:
            out.append(st + sf)
        if st and st[-1] in "bdfgmnprt":
            for sf in _DOUBLING:
                out.append(st + st[-1] + sf)
        if st.endswith("e"):  # hope -> hoping, hoped
            for sf in ("ing", "ed", "ingly", "edly", "er", "able", "ation"):
                out.append(st[:-1] + sf)
    for t in ("A_9", "A_10"):
        for w in ENTRIES[t]:
            for sf in EXCEPTION_ENDINGS:
                out.append(w + sf)
            out.append("be" + w)
            out.append("be" + w + "s")
    out += SHORT_WORDS
    out += DIGIT_WORDS
    out = [w for w in dict.fromkeys(out) if w]
    assert all(re.fullmatch(r"[a-z0-9]+", w) for w in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def measured():
    """{word: (stem, events)} of rule_words() on the restatement, computed once."""
    m = Meter()
    return {w: m.events(w) for w in rule_words()}


@functools.lru_cache(maxsize=None)
def all_events():
    out = set()
    for _, ev in measured().values():
        out |= ev
    return frozenset(out)


@functools.lru_cache(maxsize=None)
def covering_subset():
    """A subset of rule_words() with every event of the whole list: shortest words
    first, a word kept when it brings an event not yet seen; then, longest first,
    a kept word dropped again when the others still hold all of its events."""
    ms = measured()
    order = sorted(rule_words(), key=lambda w: (len(w), w))
    seen, kept = set(), []
    for w in order:
        ev = ms[w][1]
        if not ev <= seen:
            seen |= ev
            kept.append(w)
    count = {}
    for w in kept:
        for e in ms[w][1]:
            count[e] = count.get(e, 0) + 1
    final = []
    for w in reversed(kept):
        ev = ms[w][1]
        if all(count[e] > 1 for e in ev):
            for e in ev:
                count[e] -= 1
        else:
            final.append(w)
    return tuple(sorted(final))


# ---------------------------------------------------------------------------
# length edges
# ---------------------------------------------------------------------------
# one word per applying rule of steps 1b-5 and the event that shows it applied
EDGE_RULES = (
    ("agreed", ("among", "A_4", "eed")), ("hopping", "1b_undouble"), ("conflated", "1b_e_after_at"),
    ("troubling", "1b_e_after_bl"), ("sizing", "1b_e_after_iz"), ("hoping", "shortv_1b_true"),
    ("connectedly", ("among", "A_4", "edly")), ("connectingly", ("among", "A_4", "ingly")),
    ("happy", "1c_applied"),
    ("conditional", ("step", "A_5", "tional", "apply")), ("valency", ("step", "A_5", "enci", "apply")),
    ("hesitancy", ("step", "A_5", "anci", "apply")), ("comfortably", ("step", "A_5", "abli", "apply")),
    ("differently", ("step", "A_5", "entli", "apply")), ("organizer", ("step", "A_5", "izer", "apply")),
    ("operator", ("step", "A_5", "ator", "apply")), ("formality", ("step", "A_5", "aliti", "apply")),
    ("hopefulness", ("step", "A_5", "fulness", "apply")), ("callously", ("step", "A_5", "ousli", "apply")),
    ("activity", ("step", "A_5", "iviti", "apply")), ("sensibility", ("step", "A_5", "biliti", "apply")),
    ("geology", "2_ogi_after_l"), ("hopefully", ("step", "A_5", "fulli", "apply")),
    ("hopelessly", ("step", "A_5", "lessli", "apply")), ("quickly", "2_li_valid"),
    ("conditionally", ("step", "A_6", "tional", "apply")), ("operationally", ("step", "A_6", "ational", "apply")),
    ("formalize", ("step", "A_6", "alize", "apply")), ("duplicate", ("step", "A_6", "icate", "apply")),
    ("hopeful", ("step", "A_6", "ful", "apply")), ("informative", ("step", "A_6", "ative", "apply")),
    ("adjustment", ("step", "A_7", "ment", "apply")), ("adoption", "4_ion_after_t"),
    ("confusion", "4_ion_after_s"),
    ("achieve", ("step", "A_8", "e", "apply")), ("controll", "5_l_after_l"),
)
EDGE_LENGTHS = (47, 48, 49, 50, 98, 99, 100)
_RUN = "bcdfghjklmnpqrstvwxz"


def pad(word, n):
    """`word` behind a run of consonants, n bytes in all."""
    k = n - len(word)
    assert k > 0
    return (_RUN * (k // len(_RUN) + 1))[:k] + word


def length_edges():
    """Every EDGE_RULES word at raw lengths 47 .. 50 (vocab_clean's 48-byte limit)
    and 98 .. 100 (addToken drops 100)."""
    return tuple(pad(w, n) for w, _ in EDGE_RULES for n in EDGE_LENGTHS)


# ---------------------------------------------------------------------------
# many raw forms per term
# ---------------------------------------------------------------------------
BASES = ("connect", "adjust", "nation", "oper", "organ", "depend", "effect", "direct", "general", "control",
         "form", "act", "inform", "adopt", "differ", "hope", "care", "quick", "fear", "need",
         "play", "enjoy", "yield", "rich", "calm", "box", "slow", "deep", "condit", "system",
         "electr", "relig", "opin", "happi", "achiev", "replac")
FAMILY_FILL = tuple("fq%02d" % i for i in range(40))
LONG_TOKENS = ("nationalization.hopefulness.", "connections.adjustments.", "operators.organizing.depended.",
               "Effective.DIRECTLY.generals.")
N_TF = 10      # families that get the tf 255 / 256 / 257 records
N_SINGLE = 3   # records of one form per family


def spellings(form):
    return (form, form.capitalize(), form.upper())


def is_clean_short(raw):
    """vocab_clean's rule."""
    return len(raw.encode("utf-8")) <= CLEAN_MAX and re.fullmatch(r"[a-z0-9]+", raw) is not None


@functools.lru_cache(maxsize=None)
def families():
    """{base: lower-case forms the oracle stems to the base's stem}, no stopwords."""
    import oracle_lib as O
    out = {}
    for b in BASES:
        root = b[:-1] if b.endswith("e") else b
        want = O.stem(b)
        forms = [b]
        for sf in SUFFIXES:
            for w in (b + sf, root + sf):
                if w not in forms and not O.is_stopword(w) and O.stem(w) == want:
                    forms.append(w)
        out[b] = tuple(forms)
    return out


def _record(docid, words):
    lines = [" ".join(words[i:i + 12]) for i in range(0, len(words), 12)]
    return "<DOC>\n<DOCNO> %s </DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (docid, "\n".join(lines))


@functools.lru_cache(maxsize=None)
def family_records():
    """[(docid, raw words)] in file order.  Four kinds of record: every form of a
    family once (in its three spellings); forms repeated until the term's tf is 255,
    256 and 257; one form alone; two families mixed between filler words so that
    the same phrase of terms stands in different raw forms in different records.
    A few records also hold a dotted raw token over 200 bytes whose parts fall
    into the families."""
    fam = families()
    recs = []

    def add(kind, words):
        recs.append(("FM%s%04d" % (kind, len(recs)), tuple(words)))

    names = list(BASES)
    for b in names:  # A: every form once, the three spellings interleaved
        add("A", [s for f in fam[b] for s in spellings(f)])
    for b in names[:N_TF]:  # T: tf 255, 256, 257 out of all forms in turn
        sp = [s for f in fam[b] for s in spellings(f)]
        for tf in (255, 256, 257):
            add("T", [sp[(7 * i) % len(sp)] for i in range(tf)])
    for bi, b in enumerate(names):  # S: one form alone, a different form and spelling each
        for k in range(N_SINGLE):
            f = fam[b][(bi + 5 * k) % len(fam[b])]
            add("S", [spellings(f)[k % 3]])
    for bi, b in enumerate(names):  # M: two families, forms adjacent between filler words
        c = names[(bi + 1) % len(names)]
        for k in range(2):
            words = []
            for j in range(8):
                fb = fam[b][(3 * j + 11 * k + bi) % len(fam[b])]
                fc = fam[c][(5 * j + 7 * k + bi) % len(fam[c])]
                fill = FAMILY_FILL[(bi + 3 * j + k) % len(FAMILY_FILL)]
                pair = [spellings(fb)[(j + k) % 3], spellings(fc)[(j + 2 * k + 1) % 3]]
                if j % 4 == 3:
                    pair.reverse()
                words += [fill] + pair + [FAMILY_FILL[(bi + j) % len(FAMILY_FILL)]]
            add("M", words)
    for i, t in enumerate(LONG_TOKENS):  # L: raw tokens over 200 bytes, several terms each
        long_tok = t * (SHORT_RAW // len(t) + 2)
        assert len(long_tok) > SHORT_RAW
        for k in range(2):
            add("L", [FAMILY_FILL[i], long_tok, fam[names[i + k]][k], long_tok, FAMILY_FILL[i + 1]])
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def family_corpus():
    """(corpus bytes, sorted mapping docids) of family_records()."""
    recs = family_records()
    return "".join(_record(d, list(w)) for d, w in recs).encode("utf-8"), tuple(sorted(d for d, _ in recs))


def mapping_bytes(ids):
    out = [struct.pack(">i", len(ids))]
    for d in ids:
        b = d.encode("utf-8")
        out.append(struct.pack(">H", len(b)) + b)
    return b"".join(out)


def records_of(words, per=100, prefix="RW"):
    """(corpus bytes, sorted docids): the words in records of `per` words."""
    docs, ids = [], []
    for i in range(0, len(words), per):
        ids.append("%s%05d" % (prefix, i // per))
        docs.append(_record(ids[-1], list(words[i:i + per])))
    return "".join(docs).encode("utf-8"), tuple(sorted(ids))


NON_ASCII_STEMS = ("café", "naïv", "résum", "élect", "façad")
NON_ASCII_ENDINGS = ("", "s", "es", "ed", "ing", "ingly", "edly", "ly", "y", "ies", "ness", "ful", "fulness", "ation",
                     "ational", "ization", "izer", "ize", "ive", "iveness", "ivity", "able", "ably", "ability", "al",
                     "ally", "ality", "alism", "ical", "icate", "ment", "ement", "ent", "ently", "ous", "ously",
                     "ousness", "ion", "er", "ate", "ator", "ative", "ativeness", "ology", "ll", "e")


def non_ascii_words():
    """Words with one letter above every grouping's range (code unit > 121)."""
    return tuple(s + e for s in NON_ASCII_STEMS for e in NON_ASCII_ENDINGS)
