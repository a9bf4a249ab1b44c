"""The stemmer word lists and the many-forms corpus (tests/stem_words.py) checked on
the CPU, before any device run: what the lists cover, measured on the Python
restatement of the stemmer; that the C oracle and the restatement agree on every
word; and that the family corpus really holds terms with many raw forms that
reach the device's stemmer through different paths.  The figures are printed
(pytest -s) and quoted in DESIGN.md section 2."""
import functools

import pytest

import oracle_lib as O
import pyref_tokenize as P
import stem_words as S


# ---- coverage conditions ------------------------------------------------------
def _check_coverage(ev):
    """Every entry of A_0 and A_2 .. A_10 matched; every entry of steps 2-5 both
    applied and declined; every named condition met."""
    for table, entries in S.ENTRIES.items():
        if table == "A_1":
            continue
        missing = [e for e in entries if ("among", table, e) not in ev]
        assert not missing, (table, missing)
    n = 0
    for table in S.STEP_TABLES:
        for e in S.ENTRIES[table]:
            for outcome in ("apply", "decline"):
                assert ("step", table, e, outcome) in ev, (table, e, outcome)
            n += 1
    assert n == 53
    assert not [c for c in S.NAMED if c not in ev]
    # the declines by reason: every entry before R1; every rule that asks for R2 also
    # inside R1 but before R2 (a device that tested R1 there would apply it); the four
    # rules with a condition of their own also on that condition alone
    for table in S.STEP_TABLES:
        for e in S.ENTRIES[table]:
            assert ("why", table, e, "r1") in ev, (table, e)
            if table in ("A_7", "A_8") or (table, e) == ("A_6", "ative"):
                assert ("why", table, e, "r2") in ev, (table, e)
    for table, e in (("A_5", "li"), ("A_5", "ogi"), ("A_7", "ion"), ("A_8", "l")):
        assert ("why", table, e, "cond") in ev, (table, e)


def test_rule_words_cover_every_rule():
    words = S.rule_words()
    ev = S.all_events()
    _check_coverage(ev)
    among = [e for e in ev if e[0] == "among"]
    assert len(among) == sum(len(v) for v in S.ENTRIES.values()) - 3 == 107
    assert len(set(words)) == len(words) and all(w.isascii() and w == w.lower() for w in words)
    assert any(any(ch.isdigit() for ch in w[1:-1]) for w in words) and any(w[-1].isdigit() for w in words)
    print("rule_words: %d words (longest %d), %d of 110 entries matched (A_1 is out of the tokenizer's reach), "
          "%d events" % (len(words), max(map(len, words)), len(among), len(ev)))


def test_covering_subset_keeps_every_event():
    sub = S.covering_subset()
    assert set(sub) <= set(S.rule_words()) and len(set(sub)) == len(sub)
    ms = S.measured()
    ev = set()
    for w in sub:
        ev |= ms[w][1]
    assert ev == S.all_events()
    _check_coverage(ev)
    assert len(sub) <= 500  # one device thread stems these
    print("covering_subset: %d words" % len(sub))


def test_rule_words_are_deterministic():
    """A product of fixed lists: the same list, in the same order, from a fresh run."""
    a = S.rule_words()
    S.rule_words.cache_clear()
    assert S.rule_words() == a


def test_apostrophe_entries_cpu_only():
    """A_1 (' 's 's') is not reachable through processContent: the tokenizer drops
    apostrophes before the stemmer sees the token.  Its three entries are covered
    here with direct stem() calls on the two CPU restatements, and nowhere on the
    device."""
    text = "dog's dogs' 'dog dog's'"
    assert P.process_content(text) == O.process_content(text) == ["dog", "dog", "dog", "dog"]
    m = S.Meter()
    ev = set()
    for w, want in (("dog's", "dog"), ("dogs'", "dog"), ("dog's'", "dog"), ("'dog", "dog"), ("connection's", "connect")):
        got, e = m.events(w)
        assert got == want == O.stem(w), (w, got, O.stem(w))
        ev |= e
    assert {e[2] for e in ev if e[:2] == ("among", "A_1")} == set(S.ENTRIES["A_1"])


# ---- agreement ---------------------------------------------------------------
def test_oracle_agrees_with_restatement_on_rule_words():
    ms = S.measured()
    bad = [(w, ms[w][0], O.stem(w)) for w in S.rule_words() if ms[w][0] != O.stem(w)]
    assert not bad, bad[:10]
    assert all(P.stem(w) == ms[w][0] for w in S.covering_subset())  # the meter does not change the stems


def test_length_edges():
    """Every padded word still applies its rule, has the raw length it claims, sits
    on the side of vocab_clean's limit it claims, and stems alike on both CPU sides."""
    words = S.length_edges()
    assert len(words) == len(S.EDGE_RULES) * len(S.EDGE_LENGTHS) and len(set(words)) == len(words)
    m = S.Meter()
    i = 0
    for word, event in S.EDGE_RULES:
        for n in S.EDGE_LENGTHS:
            w = words[i]
            i += 1
            assert len(w) == n and w.endswith(word)
            assert S.is_clean_short(w) == (n <= S.CLEAN_MAX)
            got, ev = m.events(w)
            assert event in ev, (word, n, event)
            assert got == O.stem(w) and got != w, w
            assert P.process_content(w) == O.process_content(w) == ([] if n >= S.DROP_LEN else [got])
    rules = {e for _, e in S.EDGE_RULES}
    assert len(rules) == len(S.EDGE_RULES)
    for t in S.STEP_TABLES:  # every result code of steps 2-5 has a word
        res = {r for _, _, r in S.TABLES[t]}
        have = {r for s, _, r in S.TABLES[t] for w, e in S.EDGE_RULES
                if e == ("step", t, P.ustr(s), "apply")}
        named = {"A_5": {13, 16}, "A_7": {2}, "A_8": {2}}.get(t, set())  # ogi, li, ion, l: by their named condition
        assert have | named == res, (t, res - have - named)


def test_non_ascii_words_agree():
    for w in S.non_ascii_words():
        assert P.stem(w) == O.stem(w), w
        assert P.process_content(w) == O.process_content(w), w
        assert not S.is_clean_short(w)


# ---- the family corpus ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family_view():
    """(oracle terms {term: postings}, {term: set of raw tokens with that output},
    {raw: outputs}) of family_corpus()."""
    corpus, ids = S.family_corpus()
    ref = O.OracleIndex(corpus, S.mapping_bytes(ids), 1, 1)
    terms = {t[0][0]: t[3] for t in ref.terms() if t[0] != (" ",)}
    outs, forms = {}, {}
    for _, words in S.family_records():
        for raw in words:
            if raw not in outs:
                outs[raw] = O.process_content(raw)
                for t in outs[raw]:
                    forms.setdefault(t, set()).add(raw)
    return terms, forms, outs


def test_family_filler_and_records():
    assert O.process_content(" ".join(S.FAMILY_FILL)) == list(S.FAMILY_FILL)
    recs = S.family_records()
    corpus, ids = S.family_corpus()
    assert 200 <= len(recs) <= 400 and len(corpus) < 500 * 1000
    assert len(ids) == len(recs) and list(ids) == sorted(set(ids))
    assert len(O.split_records(corpus)) == len(recs)


def test_family_records_oracle_vs_restatement():
    corpus, _ = S.family_corpus()
    for off, n in O.split_records(corpus):
        text = corpus[off:off + n]
        assert P.process_content(text) == O.process_content(text), text[:60]


def test_family_conditions():
    terms, forms, outs = _family_view()
    assert all(t in terms for t in forms)
    fams = S.families()
    assert min(len(f) for f in list(fams.values())[:S.N_TF]) >= 40  # lower-case forms per leading base
    big = [t for t, f in forms.items() if len(f) >= 100]
    mid = [t for t, f in forms.items() if len(f) >= 12]
    assert len(big) >= 8 and len(mid) >= 32, (len(big), len(mid))
    for t in mid:  # forms through vocab_clean and through k_vocab's general path
        a = [r for r in forms[t] if S.is_clean_short(r)]
        b = [r for r in forms[t] if not S.is_clean_short(r) and len(r.encode()) <= S.SHORT_RAW]
        assert a and b, t
    long_fed = {t for r, o in outs.items() if len(r.encode()) > S.SHORT_RAW for t in o}
    assert len([t for t in long_fed if t in forms and len(forms[t]) >= 12]) >= 4, sorted(long_fed)
    assert all(len(set(o)) >= 2 for r, o in outs.items() if len(r.encode()) > S.SHORT_RAW)
    # a posting with tf >= 256 made of at least 40 different raw forms; tf 255 / 256 / 257 all present
    docno = {d: i + 1 for i, d in enumerate(S.family_corpus()[1])}
    words_of = {docno[d]: w for d, w in S.family_records()}
    best, tfs = 0, set()
    for t, posts in terms.items():
        for dn, tf in posts:
            if tf >= 255:
                tfs.add(tf)
            if tf >= 256:
                best = max(best, len({r for r in words_of[dn] if t in outs[r]}))
    assert best >= 40 and {255, 256, 257} <= tfs, (best, sorted(tfs))
    sizes = sorted((len(f) for f in forms.values()), reverse=True)
    print("family corpus: %d records, %d bytes, %d terms; raw forms per term: max %d, %d terms >= 100, %d terms >= 12; "
          "%d terms fed by raw tokens over 200 bytes; widest tf >= 256 posting made of %d forms"
          % (len(S.family_records()), len(S.family_corpus()[0]), len(terms), sizes[0], len(big), len(mid),
             len(long_fed), best))


def test_family_phrases_span_forms():
    """The adjacent pair (term of family i, term of family i + 1) stands in the M
    records in at least two different raw spellings."""
    recs = [w for d, w in S.family_records() if d.startswith("FMM")]
    _, _, outs = _family_view()
    pairs = {}
    for words in recs:
        for x, y in zip(words, words[1:]):
            if len(outs[x]) == 1 and len(outs[y]) == 1:
                pairs.setdefault((outs[x][0], outs[y][0]), set()).add((x, y))
    a, b = O.stem(S.BASES[0]), O.stem(S.BASES[1])
    assert len(pairs[(a, b)]) >= 2
    assert sum(1 for v in pairs.values() if len(v) >= 2) >= 20
