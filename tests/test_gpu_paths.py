"""Build and query paths that small, fresh-context tests never reach, each held
to the CPU oracle bit for bit and each proved to have run by a profile counter:

  * k_query_win's staged window sampling (16 windows and more: a docno span of
    65,536) and its query slices (more than 128 queries, or the win_slice option);
  * the build's grid options (tok_grid, agg_grid, agg_two_pass, raw_load_pct);
  * the capacity-retry loops of the build (raw-vocabulary table, k_vocab's
    long-token and multi-term lists).
"""
import functools
import importlib
import random

import numpy as np
import pytest

import common
import oracle_lib as O
from test_gpu_parity import QUERY_VARIANTS, _check_build

pytestmark = pytest.mark.gpu
PKG = "simple-mapreduce-search-engine-information-retrieval-_amd"
SME = importlib.import_module(PKG)
SYN = importlib.import_module(PKG + ".synth")

# ---------------------------------------------------------------------------
# A sparse-docno index.  k_query_win's window count follows the docno span
# (4096 docnos per window), not the document count: ~4,000 short documents spread
# over a mapping of M docids give 15, 16 or 20 windows and stay cheap for the oracle.
# ---------------------------------------------------------------------------
RARE = "zzqkx"   # in few documents, tf up to 60: outranks every ordinary term
NHOT = 24          # documents at the top of the docno range holding RARE at high tf
# nwin -> docids in the mapping file's range.  15 windows: the largest span of 15
# (docnos 1 .. 15 * 4096); 16: the smallest of 16 staged windows ... 16 * 4096; 20:
# every 7th docid is missing from the mapping, so those documents get negative
# docnos -(insertion point) - 1 (Arrays.binarySearch, T14) and the span is
# [-(6/7 M) - 1, 6/7 M]: M = 47,000 gives 80,570 docnos = 20 windows.
SPAN_M = {15: 15 * 4096, 16: 16 * 4096, 20: 47000}


def _nwin(dmin, dmax):
    """prepare_queries: 1024-document tiles over [dmin, dmax] rounded up to a
    multiple of 4, four tiles per window."""
    return ((((dmax - dmin) >> 10) + 1 + 3) // 4 * 4) >> 2


def _trec(did, words):
    return b"<DOC>\n<DOCNO>%s</DOCNO>\n<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (did.encode(), " ".join(words).encode())


@functools.lru_cache(maxsize=None)
def _sparse_corpus(nwin):
    """(corpus, mapping docids): 40 slices of 100 synthetic documents (V = 600,
    5 - 40 words: equal scores at the k-th place are common) spread evenly over
    docids 0 .. M - 1, the first at docid 0; RARE once or twice in a few documents
    of the first slices (the windows of the first stage); and NHOT documents at
    the very top of the range -- the last window, scored in the last stage --
    with RARE at tf 37 .. 60, which outrank everything the earlier stages kept."""
    M = SPAN_M[nwin]
    nsl, per = 40, 100
    step = (M - NHOT - per) // (nsl - 1)
    parts = []
    for s in range(nsl):
        d0 = s * step
        c = SYN.gen_corpus(per, V=600, seed=29, len_lo=5, len_hi=40, d0=d0)
        if s < 3:  # RARE at low tf in the early windows
            c = c.replace(b"<TEXT>\n", b"<TEXT>\n" + (RARE + " ").encode() * (1 + s % 2), 7)
        parts.append(c)
    rng = random.Random(nwin)
    blob, offs = SYN.make_vocab(600, 29)
    common_words = [blob[offs[i]:offs[i + 1]].decode() for i in range(8)]
    for i in range(NHOT):
        words = [RARE] * (37 + i) + [rng.choice(common_words) for _ in range(rng.randint(2, 9))]
        parts.append(_trec("D%09d" % (M - NHOT + i), words))
    ids = SYN.docids(M)
    if nwin == 20:
        ids = [d for i, d in enumerate(ids) if i % 7 != 3]  # every 7th docid unmapped -> negative docno
    return b"".join(parts), ids


@functools.lru_cache(maxsize=None)
def _sparse_index(nwin, idf_mode, tiebreak):
    """The sparse index on its own context, held to the oracle (_check_build), the
    oracle's index, the query batch and the docnos of the
    RARE documents in the last window."""
    corpus, ids = _sparse_corpus(nwin)
    ix, ref = _check_build(SME, corpus, ids, R=1, idf_mode=idf_mode, tiebreak=tiebreak)
    off, dn, tf, df = ix.csr()
    dmin = int(dn.min())
    assert _nwin(dmin, int(dn.max())) == nwin
    assert (dmin < 0) == (nwin == 20)
    names = [ix.term(i) for i in range(ix.V)]
    terms, qoff = SYN.queries_by_df(df, 300, seed=nwin, qlen_lo=1, qlen_hi=8)
    rare = names.index(RARE)
    terms[::19] = -1           # unknown terms are skipped
    terms[7] = terms[6]        # a repeated term
    for q in range(0, 300, 23):  # RARE in 14 queries, alone (single-term queries) or with others
        terms[qoff[q]] = rare
    # the high-tf RARE documents of the last window (scored in the last stage)
    r0, r1 = off[rare], off[rare + 1]
    hot = {int(d) for d, f in zip(dn[r0:r1], tf[r0:r1]) if f >= 37 and (int(d) - dmin) >> 12 == nwin - 1}
    assert len(hot) >= 20
    return ix, ref, names, terms, qoff, hot


WIN_DEFAULTS = {"query_kernel": 0, "heavy_div": 128, "seed_tiles": 4, "query_order": 1, "cand_cap": 1024,
                "seed_m": 64, "win_sample": 1, "win_stage_min": 0, "win_slice": 0}
# the window kernel's own options: a fifth stage at 20 windows, no stage beyond
# the minimum of three, slices of 1 / 7 / all queries, slices without stages
WIN_VARIANTS = [{"win_stage_min": 1}, {"win_stage_min": 1 << 20}, {"win_slice": 1}, {"win_slice": 7},
                {"win_slice": 1 << 20}, {"win_sample": 0, "win_slice": 7}]


def _query_tie(ix, terms, qoff, k, **opts):
    """(docno, score, tie word) with path options set, the defaults restored
    after; and the profile of that run."""
    try:
        for n, v in opts.items():
            ix.ctx.set_option(n, v)
        out = ix.query_topk(terms, qoff, k, with_tie=True)
        return out, ix.ctx.last_build_profile()
    finally:
        for n in opts:
            ix.ctx.set_option(n, WIN_DEFAULTS[n])


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("idf_mode,tiebreak", [(0, 0), (1, 1)])  # (reference idf, SME_TIE_DOCNO), (true df, SME_TIE_REFERENCE)
@pytest.mark.parametrize("nwin", [15, 16, 20])
def test_staged_windows_vs_oracle(nwin, idf_mode, tiebreak, k):
    """300 queries over 15 (unstaged), 16 and 20 (staged) windows against the
    oracle's rank() -- same docnos, same fp64 bits, -1 padding --, then every
    path variant of test_gpu_parity plus the window kernel's own options, with
    identical docnos, scores and tie words; the profile proves stages, slices,
    overflow and fallback ran."""
    assert (SME.SME_TIE_DOCNO, SME.SME_TIE_REFERENCE) == (0, 1)
    ix, ref, names, terms, qoff, hot = _sparse_index(nwin, idf_mode, tiebreak)
    nq = len(qoff) - 1
    (dn, sc, tie), prof = _query_tie(ix, terms, qoff, k)
    assert prof["query_kernel_name"] == "k_query_win"
    if nwin == 15:
        assert prof["query_stages"] == 1, prof
    else:
        assert prof["query_stages"] >= 4, prof
    assert prof["query_slices"] >= 2, prof
    rare_first = 0
    for q in range(nq):
        tl = [names[t] for t in terms[qoff[q]:qoff[q + 1]] if t >= 0]
        rd, rs = ref.query(tl, k, idf_mode, tiebreak)
        assert dn[q, :len(rd)].tolist() == rd, q
        assert sc[q, :len(rd)].tobytes() == np.array(rs, np.float64).tobytes(), q
        assert (dn[q, len(rd):] == -1).all(), q
        rare_first += RARE in tl and len(rd) > 0 and rd[0] in hot
    # documents of the last window, scored in the last stage, win most of the 15 - 17
    # RARE queries over what the earlier stages kept (12 or more by the oracle)
    assert rare_first >= 10
    for v in QUERY_VARIANTS + WIN_VARIANTS:
        (dn2, sc2, tie2), p2 = _query_tie(ix, terms, qoff, k, **v)
        assert np.array_equal(dn, dn2) and sc.tobytes() == sc2.tobytes() and np.array_equal(tie, tie2), v
        if v == {"win_stage_min": 1} and nwin == 20:
            assert p2["query_stages"] == 5, p2
        if v == {"win_stage_min": 1 << 20} and nwin >= 16:
            assert p2["query_stages"] == 4, p2
        if v.get("win_slice") == 7:
            assert p2["query_slices"] >= 40, p2
        if v.get("win_sample") == 0:
            assert p2["query_stages"] == 1, p2
        if v.get("win_slice") == 1 << 20:
            assert p2["query_slices"] == 1, p2
        if v == {"cand_cap": 4} and nwin >= 16:
            assert p2["query_kernel_name"] == "k_query_win"
            if k == 10:
                assert p2["query_overflow"] > 0, p2
            else:  # a list shorter than k can never finish in the window kernel
                assert p2["query_fallback"] > 0, p2


# ---------------------------------------------------------------------------
# Grid options of the build
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed_corpus():
    """~2,000 records: ordinary synthetic ones, between them the big records of
    test_build_big_records_interleaved (more distinct terms than the LDS table
    holds) and a handful of fuzz documents (markup, acronyms, non-ASCII)."""
    n = 1950
    syn = SYN.gen_corpus(n, V=3000, seed=19, len_lo=10, len_hi=60)
    recs = [r + b"</DOC>\n" for r in syn.split(b"</DOC>\n") if r]
    assert len(recs) == n
    ids = SYN.docids(n)
    rng = random.Random(5)
    docs = []
    for j, at in enumerate((3, 400, 401, 1200, 1949)):
        did = "R%03d" % j
        ids.append(did)
        words = ["b%04d" % rng.randrange(3000) for _ in range(2500)] + ["w%02d" % (j % 7)] * 3
        docs.append((at, _trec(did, words)))
    for j, at in enumerate((0, 77, 640, 641, 1500, 1800, 1948)):
        did = "FZ%04d" % j
        ids.append(did)
        docs.append((at, common.fuzz_doc(rng, did, rng.randint(5, 80)).encode("utf-8")))
    for at, d in sorted(docs, key=lambda x: -x[0]):
        recs.insert(at, d)
    return b"".join(recs), O.write_mapping(sorted(ids))


@functools.lru_cache(maxsize=None)
def _mixed_ref(R):
    corpus, mb = _mixed_corpus()
    return O.OracleIndex(corpus, mb, 1, R)


GRID_OPTS = [{"tok_grid": 1}, {"tok_grid": 7}, {"tok_grid": 64}, {"agg_grid": 1}, {"agg_grid": 3}, {"agg_grid": 64},
             {"agg_two_pass": 1}, {"agg_two_pass": 1, "agg_grid": 3}, {"raw_load_pct": 10}, {"raw_load_pct": 90}]


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("opts", GRID_OPTS, ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
def test_build_grid_options(sme, opts, R):
    """Every grid option of the build gives the oracle's index: tokenizer
    workgroups that own many records each (tok_grid 1 / 7 / 64 over ~2,000
    records), aggregation grids that stride (agg_grid 1 / 3 / 64), the count +
    emit aggregation, and the raw table's load factor -- which acts on the NEXT
    build of the context, so that one builds twice and the second is checked."""
    corpus, mb = _mixed_corpus()
    ctx = sme.Context(1, R)
    for name, v in opts.items():
        ctx.set_option(name, v)
    ctx.load_docno_mapping(mb)
    ix = ctx.build(corpus)
    if "raw_load_pct" in opts:
        ix.close()
        ix = ctx.build(corpus)
    common.check_index(ix, _mixed_ref(R), R)


# ---------------------------------------------------------------------------
# The capacity-retry loops, each on a fresh context (learned caps at their floors)
# ---------------------------------------------------------------------------
def _small_after(sme, ctx, R):
    """An ordinary small corpus on a context whose capacities a retry has grown."""
    n = 200
    c = SYN.gen_corpus(n, V=1500, seed=2, len_lo=20, len_hi=60)
    mb = SYN.mapping_bytes(n)
    ctx.load_docno_mapping(mb)
    ix = ctx.build(c)
    prof = ctx.last_build_profile()
    assert (prof["tok_attempts"], prof["vocab_attempts"], prof["lt_attempts"]) == (1, 1, 1), prof
    common.check_index(ix, O.OracleIndex(c, mb, 1, R), R)


def _dotted_corpus(tokens, nrec):
    """The tokens spread over nrec records, between ordinary words."""
    rng = random.Random(9)
    per = (len(tokens) + nrec - 1) // nrec
    docs, ids = [], []
    for r in range(nrec):
        words = []
        for t in tokens[r * per:(r + 1) * per]:
            words += ["w%02d" % rng.randrange(50), t]
        ids.append("X%04d" % r)
        docs.append(_trec(ids[-1], words + ["tail"]))
    return b"".join(docs), ids


def test_retry_vocab_overflow_list(sme):
    """1,500 distinct dotted tokens of three terms each: 4,500 entries for k_vocab's
    multi-term overflow list (two further terms and a copy of the first, per
    token) against its first capacity of 4,096 -- the kernel runs again."""
    toks = ["q%04d.r%04d.s%04d" % (i, i, i) for i in range(1500)]
    assert O.process_content(toks[1]) == ["q0001", "r0001", "s0001"]
    corpus, ids = _dotted_corpus(toks, 50)
    ix, _ = _check_build(sme, corpus, ids, R=3)
    prof = ix.ctx.last_build_profile()
    assert prof["vocab_attempts"] >= 2, prof
    assert prof["tok_attempts"] == 1 and prof["lt_attempts"] == 1, prof
    _small_after(sme, ix.ctx, 3)


def test_retry_vocab_long_list(sme):
    """4,200 distinct dotted tokens of 210 bytes (30 copies of one term each):
    k_vocab's long-token list (more than 200 bytes, first capacity 4,096)
    overflows in the first pass, which `continue`s before the overflow list is
    read; the second pass runs the long tokens and they push 4,200 x 30 entries
    on the multi-term list (capacity 4,096); the third pass fits both."""
    toks = [("ab%04d." % i) * 30 for i in range(4200)]
    assert len(toks[0]) > 200 and O.process_content(toks[7]) == ["ab0007"] * 30
    corpus, ids = _dotted_corpus(toks, 60)
    ix, _ = _check_build(sme, corpus, ids, R=3)
    prof = ix.ctx.last_build_profile()
    assert prof["vocab_attempts"] >= 3, prof
    _small_after(sme, ix.ctx, 3)


def _many_tokens_corpus(ntok=1100000, per=500):
    """ntok distinct five-letter raw tokens, `per` to a record (6.7 MB)."""
    i = (np.arange(ntok, dtype=np.int64) * 7919 + 12345) % (26 ** 5)  # 7919 is coprime to 26^5: distinct
    b = np.full((ntok, 6), ord(" "), np.uint8)
    for j in range(5):
        b[:, j] = ord("a") + (i // 26 ** j) % 26
    b[per - 1::per, 5] = ord("\n")
    nrec = ntok // per
    rows = b.reshape(nrec, per * 6)
    head = [b"<DOC>\n<DOCNO>D%09d</DOCNO>\n<TEXT>\n" % r for r in range(nrec)]
    return b"".join(h + rows[r].tobytes() + b"</TEXT>\n</DOC>\n" for r, h in enumerate(head)), nrec


def test_retry_raw_table(sme):
    """More than 2^20 distinct raw tokens: the raw-vocabulary table's first size
    (2^20 slots for a small corpus) cannot hold them, a probe run passes its
    limit and the tokenizer runs again on a table four times larger.  Partition
    digests against the oracle at R = 3, N / V / P against the cpu-opt build
    (no Python loop over 1.1 M terms).  The same corpus again on the same
    context starts from the learned size: one pass, the same bytes."""
    corpus, nrec = _many_tokens_corpus()
    mb = SYN.mapping_bytes(nrec)
    ctx = sme.Context(1, 3)
    ctx.load_docno_mapping(mb)
    ix = ctx.build(corpus)
    prof = ctx.last_build_profile()
    assert prof["tok_attempts"] >= 2, prof
    digests = [common.canon_digest(ix.partition_records(p)) for p in range(3)]
    ref = O.OracleIndex(corpus, mb, 1, 3)
    assert ix.N == ref.N == nrec
    assert digests == [common.canon_digest(ref.partition_bytes(p)) for p in range(3)]
    del ref
    opt = O.CpuOptIndex(corpus, mb)
    assert (ix.N, ix.V, ix.P) == (opt.N, opt.V, opt.P)
    del opt
    nvp = (ix.N, ix.V, ix.P)
    ix.close()
    ix = ctx.build(corpus)
    assert ctx.last_build_profile()["tok_attempts"] == 1
    assert (ix.N, ix.V, ix.P) == nvp
    assert [common.canon_digest(ix.partition_records(p)) for p in range(3)] == digests
    ix.close()
    _small_after(sme, ctx, 3)
