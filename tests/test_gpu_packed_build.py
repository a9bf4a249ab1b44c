"""The single-pass aggregation hands the term sort one packed word per pair
(term | tf << key width) and one base value per record.  Builds through it --
the default path, its grid-stride form, the K6b docid split -- must give the
index of the count + emit aggregation (agg_two_pass 1, which keeps separate key
and value words) bit for bit: csr(), weights() and the terms; and the CPU
oracle's index.  The corpora reach what the small parity corpora do not: token-
free records between others, a record for k_agg_big, and a tf at the top of a
tf field that ends exactly at bit 32.  (With a tf above 1023 the reduce order
comes from a radix sort over (merged term id, tf): the split case holds its key
width to the merged ids', which are wider than the term sort's word ranks.)"""
import functools
import importlib
import random

import numpy as np
import pytest

import common
import oracle_lib as O

pytestmark = pytest.mark.gpu
PKG = "simple-mapreduce-search-engine-information-retrieval-_amd"
SME = importlib.import_module(PKG)
SYN = importlib.import_module(PKG + ".synth")


def _trec(did, words):
    return b"<DOC>\n<DOCNO>%s</DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (did.encode(), " ".join(words).encode())


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """(corpus, mapping bytes)"""
    rng = random.Random(41)
    if name == "short":
        # 1,000 records of 1 to 20 tokens; every 9th and a run of 12 have no tokens
        # in their text (empty, or stopwords alone); one has 800 distinct terms
        # (more than the 768 a wave's table takes: k_agg_big).  About 1,100 words
        # (11-bit word ranks) beside 1,000 docid terms (12-bit merged ids), so
        # docid_split 2 splits
        n = 1000
        recs = []
        for i, did in enumerate(SYN.docids(n)):
            if i % 9 == 4 or 200 <= i < 212:
                words = [] if i % 2 else ["the", "of", "and"]
            elif i == 123:
                words = ["big%04d" % j for j in range(800)] + ["big0007"] * 5
            else:
                words = ["w%03d" % min(rng.randrange(300), rng.randrange(300)) for _ in range(rng.randint(1, 20))]
            recs.append(_trec(did, words))
        return b"".join(recs), SYN.mapping_bytes(n)
    if name == "hightf":
        # 32,000 words over 80 records of 400, 9,001 docid terms: about 41,000
        # distinct terms, 16-bit merged ids and 15-bit word ranks; one record of
        # 60,000 copies of one token, whose tf bound takes 16 bits: key and tf end
        # at bit 32 unsplit and at bit 31 split
        n = 9001
        ids = SYN.docids(n)
        recs = []
        for i in range(n):
            if i == 4500:
                words = ["t00017"] * 60000 + ["t00018", "t31999"]
            elif i % 100 == 7 and i // 100 < 80:
                words = ["t%05d" % (400 * (i // 100) + j) for j in range(400)]
            else:
                words = ["t%05d" % rng.randrange(400) for _ in range(rng.randint(1, 4))]
            recs.append(_trec(ids[i], words))
        return b"".join(recs), SYN.mapping_bytes(n)
    raise ValueError(name)


def _build(name, opts, R=1):
    corpus, mb = _corpus(name)
    ctx = SME.Context(1, R)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.load_docno_mapping(mb)
    return ctx.build(corpus)


def _views(ix):
    return ix.csr(), ix.weights(), ix.terms()


@functools.lru_cache(maxsize=None)
def _two_pass(name):
    """the count + emit build's views and the oracle's index, computed once"""
    corpus, mb = _corpus(name)
    ref = O.OracleIndex(corpus, mb, 1, 1)
    ix = _build(name, {"agg_two_pass": 1})
    common.check_index(ix, ref, 1)
    return _views(ix), ref


OPTS = [{}, {"agg_grid": 1}, {"agg_grid": 3}, {"docid_split": 2}, {"docid_split": 2, "sort_digit_bits": 6}]


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: "-".join("%s%d" % kv for kv in o.items()) or "default")
@pytest.mark.parametrize("name", ["short", "hightf"])
def test_packed_build_equals_two_pass(name, opts):
    (csr0, w0, terms0), ref = _two_pass(name)
    ix = _build(name, opts)
    if "docid_split" in opts:
        assert "docid_pairs" in ix.ctx.last_build_profile()  # the split ran
    csr1, w1, terms1 = _views(ix)
    assert terms1 == terms0
    for a, b in zip(csr1, csr0):
        assert np.array_equal(a, b)
    for a, b in zip(w1, w0):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    common.check_index(ix, ref, 1)
    if name == "hightf":
        off, dn, tf, _ = csr1
        assert int(tf.max()) == 60000 and 32768 < ix.V < 65536
