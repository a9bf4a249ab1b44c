"""Every Porter2 rule, and terms with many raw forms, on each device stemmer path,
against the CPU oracle.

tests/stem_words.py makes the words; tests/test_stem_words_host.py holds what they
cover (every among entry the tokenizer can reach, both outcomes of every entry of
steps 2-5, the named conditions) and that the oracle and the Python restatement
agree on all of them.  Here the device is asked, once per path:

  (d) k_tokenize_one   Context.process_content over the covering subset and the
                       length edges, whole token lists equal to the oracle's
  (a) vocab_clean      a build over every rule word in lower case (clean raw tokens
                       of at most 48 bytes stem in a lane's LDS slice)
  (b) vocab_one        the same words Capitalised; the length edges of 49 .. 99
                       bytes and words with a letter above every grouping's range
  (c) k_vocab_long     dotted raw tokens over 200 bytes whose parts are the
                       covering subset

and the family corpus (over a hundred raw forms per term, in three spellings, tf
past 255) through builds with and without kept positions, K = 2, both docid_terms
settings, top-k queries and phrase queries.  Every comparison is exact: record
bytes, term strings, postings, fp64 score bits."""
import contextlib
import functools

import numpy as np
import pytest

import common
import oracle_lib as O
import phrase_ref
import stem_words as S

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _built(sme, corpus, mapping, K=1, R=1, idf_mode=0, tiebreak=0, opts=None):
    """A context and its index of `corpus`, both closed on the way out."""
    ctx = sme.Context(K, R, idf_mode, tiebreak=tiebreak)
    ix = None
    try:
        for name, v in (opts or {}).items():
            ctx.set_option(name, v)
        ctx.load_docno_mapping(mapping)
        ix = ctx.build(corpus)
        yield ix
    finally:
        if ix is not None:
            ix.close()
        ctx.close()


def _check(ix, ref, R, K=1):
    """common.check_index; on a mismatch at K = 1 the terms only one side has are
    named first (a wrong stem shows up as one term missing and one extra)."""
    if K == 1:
        want = {t[0][0] for t in ref.terms() if t[0] != (" ",)}
        got = set(ix.terms())
        assert got == want, "device only: %s; oracle only: %s" % (sorted(got - want)[:20], sorted(want - got)[:20])
    common.check_index(ix, ref, R, K)


@functools.lru_cache(maxsize=None)
def _words_corpus(name):
    """(corpus, mapping) of the word lists by stemmer path."""
    if name == "lower":      # path (a); the length edges of 49 bytes and more take (b)
        words = S.rule_words() + S.length_edges()
    elif name == "capital":  # path (b): a Simple token, case folded before the stemmer
        words = tuple(w.capitalize() for w in S.rule_words() + S.length_edges())
    elif name == "general":  # path (b): clean but long, and Complex tokens
        edges = tuple(w for w in S.length_edges() if S.CLEAN_MAX < len(w) < S.DROP_LEN)
        assert len(edges) == 4 * len(S.EDGE_RULES)
        na = S.non_ascii_words()
        words = edges + na + tuple(w.capitalize() for w in na) + tuple(w.upper() for w in na)
    else:                    # path (c): every word of the covering subset inside a raw token over 200 bytes
        sub = S.covering_subset()
        toks = []
        for i in range(0, len(sub), 25):
            t = ".".join(sub[i:i + 25]) + "."
            t += ".".join(sub[:25]) if len(t) <= S.SHORT_RAW else ""
            assert len(t) > S.SHORT_RAW
            toks += [t, t.upper(), "." + t.capitalize()]
        toks += [t * (S.SHORT_RAW // len(t) + 2) for t in S.LONG_TOKENS]
        plain = S.rule_words()[::97]
        words = []
        for r in range(4):  # the long tokens in four records among ordinary words
            for i, t in enumerate(toks):
                words += list(plain[(7 * i + r) % len(plain):][:3]) + [t]
        words = tuple(words)
    corpus, ids = S.records_of(words, 100, "W" + name[0].upper())
    return corpus, S.mapping_bytes(ids)


@functools.lru_cache(maxsize=None)
def _words_ref(name, R):
    corpus, mapping = _words_corpus(name)
    return O.OracleIndex(corpus, mapping, 1, R)


# ---- path (d) ------------------------------------------------------------------
def test_process_content_rules_and_length_edges(sme):
    words = S.covering_subset() + S.length_edges()
    ctx = sme.Context(1, 1)
    try:
        for i in range(0, len(words), 100):
            text = " ".join(words[i:i + 100])
            want = O.process_content(text)
            got = ctx.process_content(text)
            if got != want:
                bad = [(w, ctx.process_content(w), O.process_content(w)) for w in words[i:i + 100]]
                bad = [b for b in bad if b[1] != b[2]]
                assert not bad, "word, device, oracle: %s" % bad[:10]
            assert got == want
    finally:
        ctx.close()


# ---- paths (a), (b), (c) ----------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("name", ["lower", "capital", "general", "long"])
def test_build_rule_words(sme, name, R):
    corpus, mapping = _words_corpus(name)
    assert len(corpus) < 1000 * 1000
    ref = _words_ref(name, R)
    with _built(sme, corpus, mapping, 1, R) as ix:
        _check(ix, ref, R)
        assert ix.ctx.last_build_profile()["vocab_attempts"] == 1


def test_paths_give_the_same_vocabulary(sme):
    """Lower case through vocab_clean and Capitalised through vocab_one: one vocabulary."""
    terms = []
    for name in ("lower", "capital"):
        corpus, mapping = _words_corpus(name)
        with _built(sme, corpus, mapping) as ix:
            terms.append([t for t in ix.terms() if not t.startswith(("wl0", "wc0"))])  # (the docids' own tokens)
    assert terms[0] == terms[1] and len(terms[0]) > 1000


# ---- families ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family():
    corpus, ids = S.family_corpus()
    return corpus, S.mapping_bytes(ids)


@functools.lru_cache(maxsize=None)
def _family_ref(K, R):
    corpus, mapping = _family()
    return O.OracleIndex(corpus, mapping, K, R)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("positions", [0, 1])
def test_family_build(sme, positions, R):
    corpus, mapping = _family()
    with _built(sme, corpus, mapping, 1, R, opts={"positions": positions}) as ix:
        _check(ix, _family_ref(1, R), R)
        # the terms of the leading families hold their tf 255 / 256 / 257 postings
        off, dn, tf, _ = ix.csr()
        for b in S.BASES[:S.N_TF]:
            t = int(ix.lookup([O.stem(b)])[0])
            assert t >= 0 and {255, 256, 257} <= set(tf[off[t]:off[t + 1]].tolist()), b


def test_family_build_k2(sme):
    """Bigrams are made from the records' term streams: every raw form in its place."""
    corpus, mapping = _family()
    with _built(sme, corpus, mapping, 2, 3) as ix:
        _check(ix, _family_ref(2, 3), 3, K=2)


@pytest.mark.parametrize("docid_terms", [0, 1])
def test_family_build_docid_terms(sme, docid_terms):
    corpus, mapping = _family()
    with _built(sme, corpus, mapping, 1, 3, opts={"docid_terms": docid_terms}) as ix:
        _check(ix, _family_ref(1, 3), 3)


def _family_queries():
    """Queries of 1 .. 4 family and filler terms, as term strings."""
    stems = [O.stem(b) for b in S.BASES]
    fill = list(S.FAMILY_FILL)
    qs = []
    for i, s in enumerate(stems):
        qs.append([s])
        qs.append([s, stems[(i + 1) % len(stems)]])
        qs.append([fill[i % len(fill)], s, stems[(i + 7) % len(stems)]])
        qs.append([s, fill[(2 * i) % len(fill)], stems[(i + 1) % len(stems)], fill[(2 * i + 1) % len(fill)]])
    qs += [[f] for f in fill[:6]] + [[stems[0], stems[0]], ["nosuchterm", stems[1]]]
    return qs


@pytest.mark.parametrize("tiebreak", [0, 1])
@pytest.mark.parametrize("idf_mode", [0, 1])
def test_family_queries(sme, idf_mode, tiebreak):
    corpus, mapping = _family()
    ref = _family_ref(1, 1)
    qs = _family_queries()
    with _built(sme, corpus, mapping, 1, 1, idf_mode, tiebreak) as ix:
        words = sorted({t for q in qs for t in q})
        table = dict(zip(words, ix.lookup(words).tolist()))
        assert table["nosuchterm"] == -1 and min(v for w, v in table.items() if w != "nosuchterm") >= 0
        terms = np.array([table[t] for q in qs for t in q], np.int32)
        qoff = np.cumsum([0] + [len(q) for q in qs]).astype(np.int64)
        dn, sc = ix.query_topk(terms, qoff, 10)
        full = 0
        for i, q in enumerate(qs):
            rd, rs = ref.query([t for t in q if table[t] >= 0], 10, idf_mode, tiebreak)
            assert dn[i, :len(rd)].tolist() == rd, (i, q)
            assert np.array_equal(sc[i, :len(rd)].view(np.uint64), np.array(rs, np.float64).view(np.uint64)), (i, q)
            assert (dn[i, len(rd):] == -1).all()
            full += len(rd) == 10
        assert full >= len(S.BASES)


@functools.lru_cache(maxsize=None)
def _family_phrases():
    """(Streams, phrases of term strings): adjacent families in both orders, with a
    filler word before, a term three times running, and phrases that stand nowhere."""
    corpus, mapping = _family()
    st = phrase_ref.Streams(corpus, mapping, _family_ref(1, 1))
    stems = [O.stem(b) for b in S.BASES]
    n = len(stems)
    phrases = []
    for i, s in enumerate(stems):
        nxt = stems[(i + 1) % n]
        phrases += [[s, nxt], [nxt, s], [S.FAMILY_FILL[i % len(S.FAMILY_FILL)], s, nxt]]
        if i % 3 == 0:
            phrases += [[s, nxt, s], [s, stems[(i + 2) % n]], [s, s, s]]
    # from the reference, before the device is asked: enough phrases, half of them in a
    # document, and the matching two-term phrases stand there in differing raw forms
    hits = [st.match(ph) for ph in phrases]
    assert len(phrases) >= 20 and 2 * sum(1 for h in hits if h) >= len(phrases)
    assert any(not h for h in hits)
    spelled = {}
    for _, words in S.family_records():
        for x, y in zip(words, words[1:]):
            spelled.setdefault((tuple(O.process_content(x)), tuple(O.process_content(y))), set()).add((x, y))
    near = {(a, b) for i, a in enumerate(stems) for b in (stems[i - 1], stems[(i + 1) % n])}  # adjacent families
    two = [ph for ph, h in zip(phrases, hits) if h and tuple(ph) in near]
    assert len(two) >= 20 and all(len(spelled.get(((a,), (b,)), ())) >= 2 for a, b in two)
    return st, phrases


def test_family_phrases(sme):
    st, phrases = _family_phrases()
    corpus, mapping = _family()
    for idf_mode in (0, 1):
        with _built(sme, corpus, mapping, 1, 2, idf_mode, opts={"positions": 1}) as ix:
            assert ix.positions()[:2] == (len(st.records), sum(len(s) for _, s in st.records))
            words = sorted({t for ph in phrases for t in ph})
            table = dict(zip(words, ix.lookup(words).tolist()))
            ids = [[table[t] for t in ph] for ph in phrases]
            assert min(min(p) for p in ids) >= 0
            for order, m in ((0, 0), (1, 0), (1, 3)):
                got = ix.query_phrase(ids, order, m)
                want = st.run(phrases, order, m, idf_mode)
                for g, w in zip(got[:3], want[:3]):
                    assert np.array_equal(g, w)
                assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
