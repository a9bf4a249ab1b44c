"""Generated corpora for the index merger's edge tests (tests/test_gpu_ixmerge.py).

Docids are "D%06d" and the mapping holds D000001 .. D{NMAP}, so docno = the number
in the docid (its rank in the mapping): a case places its postings at will.  A
case is a list of inputs, each a list of documents (docid spec, text); the whole
corpus is the inputs laid end to end, in order.  A docid spec is an int (that
docno), None (no DOCNO: docno 0) or a string (a literal docid; one outside the
mapping gets a negative docno, the same one wherever it occurs).  Every case
concentrates on one term, named for the case."""

NMAP = 20000
SHARES = (0, 1, 63, 64, 65, 127, 128, 129)


def mapping_ids():
    return ["D%06d" % i for i in range(1, NMAP + 1)]


def doc_bytes(d, text):
    did = "" if d is None else "<DOCNO> %s </DOCNO>\n" % (d if isinstance(d, str) else "D%06d" % d)
    return ("<DOC>\n%s<TEXT>\n%s\n</TEXT>\n</DOC>\n" % (did, text)).encode()


def corpus_bytes(docs):
    return b"".join(doc_bytes(d, t) for d, t in docs)


def _merge_docs(*lists):
    """Documents given as {docno: [words]} dicts -> one input's document list, by docno."""
    acc = {}
    for m in lists:
        for d, words in m.items():
            acc.setdefault(d, []).extend(words)
    return [(d, " ".join(w)) for d, w in sorted(acc.items())]


def share_case():
    """Two inputs; per (a, b) in SHARES x SHARES three terms held by a documents of A
    and b of B: i<a>x<b> interleaved (A on even docnos, B on odd), l<a>x<b> with all
    of B below all of A, h<a>x<b> with all of B above all of A."""
    A, B = {}, {}
    for a in SHARES:
        for b in SHARES:
            for j in range(a):
                A.setdefault(1000 + 2 * j, []).append("i%dx%d" % (a, b))
                A.setdefault(5000 + j, []).append("l%dx%d" % (a, b))
                A.setdefault(7000 + j, []).append("h%dx%d" % (a, b))
            for j in range(b):
                B.setdefault(1001 + 2 * j, []).append("i%dx%d" % (a, b))
                B.setdefault(3000 + j, []).append("l%dx%d" % (a, b))
                B.setdefault(9000 + j, []).append("h%dx%d" % (a, b))
    return [_merge_docs(A), _merge_docs(B)]


def tile_edge_case(T):
    """Merged lists of three tiles + 1 postings: `edge`'s first share is exactly one
    tile (it ends at a tile edge), `inside`'s ends inside the second tile; `mixed`
    interleaves the same counts."""
    L = 3 * T + 1
    A, B = {}, {}
    for j in range(T):
        A.setdefault(1 + j, []).append("edge")
    for j in range(L - T):
        B.setdefault(1 + T + j, []).append("edge")
    na = T + T // 2 + 3
    for j in range(na):
        A.setdefault(1 + j, []).append("inside")
    for j in range(L - na):
        B.setdefault(1 + na + j, []).append("inside")
    for j in range(na):
        A.setdefault(2 * L + 2 * j, []).append("mixed")
    for j in range(L - na):
        B.setdefault(2 * L + 1 + 2 * j, []).append("mixed")
    return [_merge_docs(A), _merge_docs(B)]


def three_input_case():
    """A term only in the first input, only in the last, in all three."""
    ins = []
    for a in range(3):
        docs = {}
        for j in range(5):
            d = 10 + 3 * j + a
            docs[d] = ["everywhere", "filler%d" % a]
            if a == 0:
                docs[d].append("onlyfirst")
            if a == 2:
                docs[d].append("onlylast")
        ins.append(_merge_docs(docs))
    return ins


def duplicate_case():
    """The same docid in two and in three inputs, docno 0 (no DOCNO) and docids
    outside the mapping in several (MISSING7 sorts after every mapped docid, AMISSING
    before: two different negative docnos)."""
    ins = []
    for a in range(3):
        docs = [(40, "intwo twice" if a < 2 else "other"), (41, "inthree inthree" + " inthree" * a),
                (None, "nodocno zero%d" % a), (None, "nodocno again"), ("MISSING7", "unmapped neg"),
                ("AMISSING" if a else "MISSING7", "unmapped other"), (50 + a, "plain intwo")]
        ins.append(docs)
    return ins


def large_tf_case():
    """One word 600 times in a document of two inputs: the summed tf 1200 leaves
    kTfSortMaxTf = 1023 while no input does."""
    big = " ".join(["sixhundred"] * 600)
    return [[(7, big), (8, "small sixhundred")], [(7, big + " tail"), (9, "sixhundred sixhundred")]]


def stream_len_case():
    """Records of 0, 1, 63, 64, 65 stream positions next to each other in docno order,
    alternating between the inputs; with and without a DOCNO."""
    ins = [[], []]
    d = 100
    for rep in range(2):
        for k in (0, 1, 63, 64, 65):
            text = " ".join("w%d" % (i % 7) for i in range(k))
            ins[(d + rep) % 2].append((d, text))
            d += 1
    ins[0].append((None, ""))
    ins[1].append((None, "w1 w2"))
    ins[0].append((None, " ".join("w3" for _ in range(64))))
    return ins


def empty_input_cases():
    """An input with no records first, in the middle and last."""
    a = [(5, "alpha beta"), (9, "beta gamma")]
    b = [(6, "beta delta"), (9, "gamma gamma")]
    return [[[], a, b], [a, [], b], [a, b, []]]


def tiny_inputs_case(n=64):
    """n inputs of one or two small documents: every term's lists are single postings."""
    ins = []
    for a in range(n):
        docs = [(200 + (a * 37) % 101, "common t%d" % (a % 5))]
        if a % 3 == 0:
            docs.append((200 + (a * 37) % 101 + 101, "common rare%d" % a))
        ins.append(docs)
    return ins


def four_pieces_case():
    """Four inputs for the merge of two merges against the merge of the four."""
    ins = []
    for a in range(4):
        docs = {}
        for j in range(40):
            d = 300 + 4 * j + (a * 7) % 4 if a % 2 else 300 + 2 * j + a
            docs.setdefault(d, []).extend(["quad", "p%d" % a, "m%d" % (j % 3)])
        ins.append(_merge_docs(docs) + [(None, "quad nodoc%d" % a)])
    return ins
