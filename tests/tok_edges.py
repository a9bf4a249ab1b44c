"""Deterministic corpora that put markup, entities, UTF-8 and record bounds on the
chunk, wave, lane and stage edges of the byte-parallel tokenizer (k_tok_fast in
csrc/sme_build.hip), and on the constants of its neighbours k_scan_lt and k_docno.
Pure Python: no GPU, no libsme, no oracle.

The constants below RESTATE the kernel's.  If the kernel's change, everything here
still passes -- the placement assertions are about this file's own arithmetic --
but the cases no longer sit on the kernel's edges: change both together.

Layout.  With the build option tok_grid = 1 one workgroup owns every fast record
and walks them as one stream of CHUNK-byte chunks; chunk k begins at text position
((rs0 + mis) & ~15) - mis + k * CHUNK, rs0 the start of the first fast record and
mis the corpus pointer modulo 16.  Every corpus starts with an 8 KiB fast record
at byte 0, so the origin is -mis.  After it comes one record per case: a case is
(construct, edge kind, cut j) and byte j of the construct sits exactly on an edge
of that kind (bytes [0, j) before it).  Records are packed in position order --
the next chunk-end case when a chunk end is near, else a wave-edge case, else a
lane-edge case -- so a record is as long as the way to its edge, not a whole chunk.
Every placement is asserted after the corpus is built (Corpus.check), and every
record's declared path (fast / slow) is checked against a restatement of the
kernel's lt_simple and its 48-byte rule.

The docid spells the case: family letter, construct index, edge kind (C chunk
end, W wave edge, L lane edge, S stage end, N not placed), variant (A markers
abut the construct, S a space between) and the cut, e.g. G004CAJ00007.
"""
import re
import struct

CHUNK = 16384          # kChunk = kTokNT * kTokBytes: text bytes per workgroup step
LANE = 64              # kTokBytes: bytes per lane
WAVE = 4096            # 64 lanes * kTokBytes: bytes per wave (the block scans' wave totals)
STAGE = 16384 + 1024   # kStageV * 16: the LDS stage, chunk + SME_TOKLA * 16 bytes of lookahead
REC_WIN = 384          # kRecWin: records overlapping one chunk
MIN_FAST = 48          # kMinFastRec (SME_MINFASTREC): shorter records take k_tok_slow
DOC_WIN = 96           # kDocWin: k_docno's staged window
LT_BUF = 2048          # kLtBuf: '<' positions k_scan_lt buffers per step
TOK_CAP = 2560         # kTokCap (SME_TOKCAP): chunk tokens per round
TOK_MISS = 256         # kTokMiss (SME_TOKMISS): deferred raw-vocabulary inserts per round

MINFILL = 200          # filler bytes either side of a case
HEAD = b"<DOC>\n<DOCNO> %s </DOCNO>\n<TEXT>\n"
TAIL = b"\n</TEXT>\n</DOC>"

# three vocabularies of words that stem to themselves and are no stopwords (the
# host test checks that with the oracle): filler (>= 5 bytes, so a record stays
# far below the token stream's len / 2 slots), words hidden inside spans, and the
# per-case markers bef##### / aft#####
FILL = [b"w" + bytes([97 + i // 26, 97 + i % 26]) + b"%02d" % (i % 100) for i in range(300)]
HIDDEN = [b"hq%03d" % i for i in range(400)]


def bef(n):
    return b"bef%05d" % n


def aft(n):
    return b"aft%05d" % n


# ---------------------------------------------------------------------------
# the kernel's record classification, restated
# ---------------------------------------------------------------------------
_BEGIN_STOP = re.compile(rb"[ <>\x80-\xff]")


def lt_span_end(t, p):
    """lt_span_end: inclusive end of the markup at '<' p, len(t) if unterminated."""
    n = len(t)
    if p + 1 >= n:
        return n
    c = t[p + 1:p + 2]
    if c == b"!" and t[p + 2:p + 4] == b"--":
        i = t.find(b"-->", p + 1)
        return i + 2 if i >= 0 else n
    if c == b"?":
        i = t.find(b"?>", p + 1)
        return i + 1 if i >= 0 else n
    i = t.find(b">", p + (2 if c == b"/" else 1))
    return i if i >= 0 else n


def lt_simple(t, p):
    """lt_simple: does the byte-parallel path reproduce the markup at '<' p?"""
    n = len(t)
    if p + 1 >= n:
        return False
    c = t[p + 1:p + 2]
    if c in (b"/", b"!", b"?"):
        q = lt_span_end(t, p)
        return q < n and t.find(b"<", p + 1, q + 1) < 0
    m = _BEGIN_STOP.search(t, p + 1)
    if m is None or m.group() != b">":
        return False
    return t[p + 1:m.start()].lower() not in (b"script", b"style")


def record_is_fast(t, rs, re_):
    if re_ - rs < MIN_FAST:
        return False
    p = t.find(b"<", rs, re_)
    while p >= 0:
        if not lt_simple(t, p):
            return False
        p = t.find(b"<", p + 1, re_)
    return True


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
def is_edge(kind, x, mis):
    """Is text position x an edge of this kind for the chunk origin -mis?"""
    q = x + mis
    if kind == "C":
        return q > 0 and q % CHUNK == 0
    if kind == "W":
        return q % WAVE == 0 and q % CHUNK != 0
    if kind == "L":
        return q % LANE == 0 and q % WAVE != 0
    if kind == "S":  # c + STAGE of a chunk c >= 0
        return q >= STAGE and (q - (STAGE - CHUNK)) % CHUNK == 0
    raise ValueError(kind)


_STEP = {"C": CHUNK, "W": WAVE, "L": LANE, "S": CHUNK}


def next_edge(kind, p, mis):
    """The first edge of this kind at or after text position p."""
    off = STAGE - CHUNK if kind == "S" else 0
    step = _STEP[kind]
    x = -((-(p + mis - off)) // step) * step + off - mis
    while not is_edge(kind, x, mis):
        x += step
    return x


def cuts(n, extra=()):
    """Every cut of a construct of up to 12 bytes; of a longer one the first and
    last four and `extra` (the cuts through its terminator)."""
    if n <= 12:
        return list(range(n + 1))
    return sorted(set([0, 1, 2, 3] + list(range(n - 3, n + 1)) + [j for j in extra if 0 <= j <= n]))


class Spec:
    """One case before placement: the construct, its edge kind, cut and variant;
    sep = (construct separates a marker abutting it before, after); hidden = words
    that must not reach the vocabulary; fast = the record's declared path;
    ends = the construct ends with the record's </DOC> (no tail follows)."""

    def __init__(self, ci, cons, kind, j, variant="S", sep=(True, True), hidden=(), fast=True, ends=False,
                 aft_hidden=False):
        self.ci, self.cons, self.kind, self.j, self.variant = ci, cons, kind, j, variant
        self.sep, self.hidden, self.fast, self.ends, self.aft_hidden = sep, list(hidden), fast, ends, aft_hidden


class Corpus:
    def __init__(self, fam, mis):
        self.fam, self.mis = fam, mis
        self.buf = bytearray()
        self.recs = []      # dicts: docid, rs, re, fast, expect (words with one posting here), hidden
        self.anchors = []   # (text position, kind, construct start or None)
        self.placed = []    # (construct start, construct bytes)
        self.constructs = {}  # construct index -> bytes, of the cases place_all placed
        self._word = 0
        self._serial = 0
        self.lead()

    # --- bytes
    def fill(self, n):
        """Exactly n bytes of filler words, a space before and after each."""
        out = bytearray(b" " if n else b"")
        while len(out) + 6 <= n:
            out += FILL[self._word % len(FILL)] + b" "
            self._word += 1
        return bytes(out) + b" " * (n - len(out))

    def serial(self):
        self._serial += 1
        return self._serial

    def emit(self, seq, kind=None, dry=False):
        """Append a sequence of bytes and markers: ("R", docid, fields) / ("E",)
        record start / end, ("F", n) n filler bytes, ("X",) the one flexible fill,
        ("K", cons) a construct starts here, ("A", j) the byte j after this point
        goes on the next edge of `kind`.  dry: only the extra fill that would take."""
        pos, anchor = len(self.buf), None
        for it in seq:
            if isinstance(it, (bytes, bytearray)):
                pos += len(it)
            elif it[0] == "F":
                pos += it[1]
            elif it[0] == "X":
                pos += MINFILL
            elif it[0] == "A":
                anchor = pos + it[1]
        extra = 0
        if kind is not None:
            extra = next_edge(kind, anchor, self.mis) - anchor
        if dry:
            return extra
        cur, kpos = None, None
        for it in seq:
            if isinstance(it, (bytes, bytearray)):
                self.buf += it
            elif it[0] == "F":
                self.buf += self.fill(it[1])
            elif it[0] == "X":
                self.buf += self.fill(MINFILL + extra)
            elif it[0] == "R":
                cur = dict(docid=it[1], rs=len(self.buf), fast=True, expect=[], hidden=[])
                cur.update(it[2])
            elif it[0] == "E":
                cur["re"] = len(self.buf)
                self.recs.append(cur)
            elif it[0] == "K":
                kpos = len(self.buf)
                self.placed.append((kpos, bytes(it[1])))
            elif it[0] == "A":
                self.anchors.append((len(self.buf) + it[1], kind, kpos))
        return extra

    def lead(self):
        """The first record: fast, at byte 0, exactly 8 KiB; it fixes the chunk origin."""
        h = HEAD % (b"%s0LEAD" % self.fam.encode())
        self.emit([("R", "%s0LEAD" % self.fam, {}), h, ("F", 8192 - len(h) - len(TAIL)), TAIL, ("E",), b"\n"])
        assert len(self.buf) == 8193 and self.recs[0]["re"] == 8192

    def plain(self, docid, nbytes=MINFILL, **fields):
        """An ordinary fast record with nbytes of filler."""
        self.emit([("R", docid, fields), HEAD % docid.encode(), ("F", nbytes), TAIL, ("E",), b"\n"])

    # --- standard cases
    def case_seq(self, s):
        n = self.serial() if not hasattr(s, "n") else s.n
        s.n = n
        docid = "%s%03d%s%sJ%05d" % (self.fam, s.ci, s.kind, s.variant, s.j)
        gap = b"" if s.variant == "A" else b" "
        expect = []
        if s.variant == "S" or s.sep[0]:
            expect.append(bef(n))
        if not s.aft_hidden and not s.ends and (s.variant == "S" or s.sep[1]):
            expect.append(aft(n))
        hidden = list(s.hidden) + ([aft(n)] if s.aft_hidden else [])
        seq = [("R", docid, dict(fast=s.fast, expect=expect, hidden=hidden, kind=s.kind, cut=s.j)),
               HEAD % docid.encode(), ("X",), bef(n) + gap, ("K", s.cons), s.cons[:s.j], ("A", 0), s.cons[s.j:]]
        if s.ends:
            seq += [("E",), b"\n"]
        else:
            seq += [gap + aft(n), ("F", MINFILL), TAIL, ("E",), b"\n"]
        return seq

    def place_all(self, specs):
        """Pack the cases in position order: the rarest edge kind whose next edge
        is near, else a lane-edge case, else whatever needs the least filler."""
        left = {k: [s for s in specs if s.kind == k] for k in "SCWL"}
        for s in specs:
            self.constructs.setdefault(s.ci, s.cons)
        for k in left:
            left[k].reverse()
        while any(left.values()):
            best = None
            for k in "SCWL":
                if left[k] and self.emit(self.case_seq(left[k][-1]), k, dry=True) <= 600:
                    best = k
                    break
            if best is None:
                best = "L" if left["L"] else min((k for k in "SCW" if left[k]),
                                                 key=lambda k: self.emit(self.case_seq(left[k][-1]), k, dry=True))
            s = left[best].pop()
            self.emit(self.case_seq(s), best)

    # --- results
    def bytes(self):
        return bytes(self.buf)

    def docids(self):
        return sorted(r["docid"] for r in self.recs)

    def mapping(self):
        out = [struct.pack(">i", len(self.recs))]
        for d in self.docids():
            b = d.encode("utf-8")
            out.append(struct.pack(">H", len(b)) + b)
        return b"".join(out)

    def docno(self, docid):
        return self.docids().index(docid) + 1

    def n_fast(self):
        return sum(1 for r in self.recs if r["fast"])

    def n_slow(self):
        return sum(1 for r in self.recs if not r["fast"])

    def check(self):
        """The generator's self-checks: every construct is where it was put, byte j
        of it on an edge of its kind (a stage-end construct beginning inside the
        chunk whose stage ends there), the first record fast at byte 0, docids
        unique, records disjoint and ascending, and every record's declared path
        equal to the restated lt_simple / 48-byte rule."""
        t = bytes(self.buf)
        for a, cons in self.placed:
            assert t[a:a + len(cons)] == cons, (self.fam, a)
        for x, kind, k0 in self.anchors:
            if kind is None:
                continue
            assert is_edge(kind, x, self.mis), (self.fam, kind, x)
            if kind == "S":
                assert x - STAGE <= k0 < x - (STAGE - CHUNK), (self.fam, x, k0)
        ids = [r["docid"] for r in self.recs]
        assert len(set(ids)) == len(ids)
        assert self.recs[0]["rs"] == 0 and self.recs[0]["fast"]
        last = 0
        for r in self.recs:
            assert last <= r["rs"] < r["re"] and t[r["rs"]:r["rs"] + 5] == b"<DOC>" and t[r["re"] - 6:r["re"]] == b"</DOC>"
            last = r["re"]
            assert record_is_fast(t, r["rs"], r["re"]) == r["fast"], (r["docid"], r["fast"])
        return True


# ---------------------------------------------------------------------------
# construct makers
# ---------------------------------------------------------------------------
def token(n, salt=0):
    """A token of n lower-case letters, the same for one (n, salt)."""
    x = (n * 2654435761 + salt * 40503 + 12345) & 0xFFFFFFFF
    out = bytearray()
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(97 + (x >> 16) % 26)
    return bytes(out)


_DECOY = [b" ", b" -- ", b" -> ", b" > ", b" - "]


def hidden_body(n, h0=0):
    """n bytes of hidden words between decoys of the comment / PI terminators
    (no '<', no "-->", no "?>"); returns (bytes, words)."""
    out, words, i = bytearray(), [], 0
    while len(out) + 5 + 4 <= n:
        w = HIDDEN[(h0 + i) % len(HIDDEN)]
        out += w + _DECOY[i % len(_DECOY)]
        words.append(w)
        i += 1
    if not words and n >= 2:
        out += b"zq"
        words.append(b"zq")
    return bytes(out) + b" " * (n - len(out)), sorted(set(words))


def comment(n, h0=0):
    body, words = hidden_body(n - 7, h0)
    return b"<!--" + body + b"-->", words


def pi(n, h0=0):
    body, words = hidden_body(n - 6, h0)
    return b"<?pi" + body + b"?>", words


def _specs(items, kinds="CWL", variants="AS"):
    """items: (construct, options) in construct-index order -> every (kind, variant, cut)."""
    out = []
    for ci, (cons, opt) in enumerate(items):
        opt = dict(opt)
        extra = opt.pop("extra", ())
        ks = opt.pop("kinds", kinds)
        vs = opt.pop("variants", variants)
        for k in ks:
            for v in vs:
                for j in cuts(len(cons), extra):
                    if k == "S" and not STAGE - CHUNK < j <= STAGE:
                        continue  # a stage-end construct begins before its chunk's end
                    out.append(Spec(ci, cons, k, j, v, **opt))
    return out


# ---------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------
SHORT_LENS = [1, 2, 15, 16, 17, 24, 25, 32, 33]
LONG_LENS = [63, 64, 65, 100, 101, 199, 200, 201, 256, 1100]


def _twins(c, lens):
    """Every token of 17 bytes or more once more inside one wave of a chunk (it
    must merge with its straddling copies), and two near-twins that differ only
    at byte 17 or only in the last byte (they must not)."""
    for i, n in enumerate(x for x in lens if x >= 17):
        t = token(n)
        a = t[:16] + bytes([97 + (t[16] - 96) % 26]) + t[17:]
        b = t[:-1] + bytes([97 + (t[-1] - 96) % 26])
        assert a != t and b != t and len(a) == len(b) == n
        body = b" " + t + b" " + a + b" " + b + b" " + t + b" "
        docid = "%sTW%05d" % (c.fam, n)
        kind = "W" if len(body) <= WAVE else "C" if len(body) <= CHUNK else None
        c.emit([("R", docid, dict(kind="N")), HEAD % docid.encode(), ("X",), ("K", body), ("A", 0), body,
                ("F", MINFILL), TAIL, ("E",), b"\n"], kind)


def family_tokens_short(mis):
    """Tokens of 1 .. 33 bytes and the acronym / apostrophe / number shapes, a
    space either side, cut at every byte across chunk, wave and lane edges: a
    token ends on the last byte before the edge (cut = len), starts on the
    first after it (cut 0), a single split byte sits on the edge (cut len of a
    token followed by its space)."""
    c = Corpus("T", mis)
    items = [(token(n), {}) for n in SHORT_LENS] + [(w, {}) for w in (b"U.S.A.", b"a.b.c.d.e", b"don't", b"3.14")]
    c.place_all(_specs(items, variants="S"))
    _twins(c, SHORT_LENS)
    return c


def family_tokens_long(mis):
    """Tokens of 63 .. 1100 bytes (tok_sig_long, the emask of the next lane, the
    100-byte drop) and one of 17000 that starts in one chunk and ends two on;
    the 1100-byte token also with its last bytes across the stage end."""
    c = Corpus("U", mis)
    items = [(token(n), {"kinds": "CWLS" if n > 1024 else "CWL"}) for n in LONG_LENS]
    items.append((token(17000), {"kinds": "C"}))
    c.place_all(_specs(items, variants="S"))
    _twins(c, LONG_LENS + [17000])
    return c


def family_utf8(mis):
    """2-, 3- and 4-byte characters inside a token, the no-break / em / ideographic
    spaces between words (none is a split byte), a lone continuation byte, a
    truncated lead byte and 0xFF, each cut at every byte."""
    c = Corpus("Y", mis)
    ns = {"sep": (False, False)}
    items = [(b"ab" + ch.encode("utf-8") + b"cd", ns) for ch in ("é", "€", "\U0001F600")]
    items += [(ch.encode("utf-8"), ns) for ch in (" ", " ", "　")]
    items += [(b"\x80", ns), (b"\xe2", ns), (b"\xe2\x82", ns), (b"\xff", ns)]
    c.place_all(_specs(items))
    return c


def family_tags(mis):
    """Simple tags with words abutting them and a space away."""
    c = Corpus("G", mis)
    items = [(t, {}) for t in (b"<b>", b"</b>", b"<br/>", b"<HEADLINE>", b"</HEADLINE>", b"<!DOCTYPE html>")]
    c.place_all(_specs(items))
    return c


def family_comments(mis):
    """Comments of 9 .. 1030 bytes, hidden words and terminator decoys inside, and
    the Galago quirks <!--> and <!--->; the 1030-byte one also with --> across
    the stage end."""
    c = Corpus("M", mis)
    items = []
    for i, n in enumerate((9, 70, 200, 1030)):
        cons, words = comment(n, 20 * i)
        items.append((cons, {"hidden": words, "kinds": "CWLS" if n > 1024 else "CWL"}))
    items += [(b"<!-->", {}), (b"<!--->", {})]
    c.place_all(_specs(items))
    return c


def family_pis(mis):
    """Processing instructions of 8 and 1100 bytes (the long one also with ?> across
    the stage end) and <?>."""
    c = Corpus("P", mis)
    items = []
    for i, n in enumerate((8, 1100)):
        cons, words = pi(n, 100 + 20 * i)
        items.append((cons, {"hidden": words, "kinds": "CWLS" if n > 1024 else "CWL"}))
    items.append((b"<?>", {}))
    c.place_all(_specs(items))
    return c


def family_comments_long(mis):
    """Comments of 4200, 20000 and 40000 bytes: the last two hold one and two whole
    chunks, so the span carried from chunk to chunk (mask_carry) crosses several
    edges before its --> is cut by one; the 4200-byte one also across the stage end."""
    c = Corpus("N", mis)
    items = []
    for i, (n, kinds) in enumerate(((4200, "CWLS"), (20000, "C"), (40000, "C"))):
        cons, words = comment(n, 37 * i)
        items.append((cons, {"hidden": words, "kinds": kinds}))
    c.place_all(_specs(items))
    return c


def family_entities(mis):
    """Entities: terminated, numeric, upper-case (no entity), empty, unterminated."""
    c = Corpus("A", mis)
    items = [(e, {}) for e in (b"&amp;", b"&#169;", b"&AMP;", b"&;")]
    items.append((b"&nosemi word", {"sep": (True, False)}))
    c.place_all(_specs(items))
    return c


def family_entities_long(mis):
    """An entity of 1100 bytes ending in ';' and the same ending in a space, the
    decisive byte also across the stage end."""
    c = Corpus("B", mis)
    items = [(b"&" + b"q" * 1100 + b";", {"kinds": "CWLS"}), (b"&" + b"q" * 1100 + b" ", {"kinds": "CWLS"})]
    c.place_all(_specs(items))
    return c


def family_entities_end(mis):
    """'&' and '&amp' as the record's last bytes before </DOC>, and &amp; inside a
    comment."""
    c = Corpus("E", mis)
    items = [(b"&</DOC>", {"ends": True, "kinds": "CL"})]
    items.append((b"&amp</DOC>", {"ends": True, "kinds": "CL"}))
    items.append((b"<!-- hq390 &amp; hq391 -->", {"hidden": [b"hq390", b"hq391"], "extra": range(10, 18)}))
    c.place_all(_specs(items))
    return c


BOUNDARY = b"</DOC>\n<DOC>\n<DOCNO>"
JUNK = b" jq001 <b> &amp; jq002 "


def family_records(mis):
    """Record bounds on the edges: </DOC>\\n<DOC>\\n<DOCNO> cut at every byte (a
    record ends at c - 1, c, c + 1 and the next starts there), junk between
    records across the edge, and a slow record under 48 bytes across the edge
    between fast ones."""
    c = Corpus("R", mis)
    for kind in "CL":
        for j in range(len(BOUNDARY) + 1):
            n, m = c.serial(), c.serial()
            a, b = "R900%sAJ%05d" % (kind, j), "R900%sBJ%05d" % (kind, j)
            c.emit([("R", a, dict(expect=[bef(n)], kind=kind, cut=j)), HEAD % a.encode(), ("X",), bef(n) + b"\n</TEXT>\n",
                    ("K", BOUNDARY), ("A", j), b"</DOC>", ("E",), b"\n", ("R", b, dict(expect=[aft(m)], kind=kind, cut=j)),
                    b"<DOC>\n<DOCNO>", b" %s </DOCNO>\n<TEXT>\n" % b.encode(), aft(m), ("F", MINFILL), TAIL, ("E",),
                    b"\n"], kind)
        for j in range(len(JUNK) + 1):
            a = "R901%sAJ%05d" % (kind, j)
            c.emit([("R", a, dict(hidden=[b"jq001", b"jq002"], kind=kind, cut=j)), HEAD % a.encode(), ("X",), TAIL,
                    ("E",), ("K", JUNK), ("A", j), JUNK], kind)
        for j in cuts(40, (19, 20)):  # a record under 48 bytes, between two fast ones
            n = c.serial()
            a, z = "R902%sAJ%05d" % (kind, j), "Z%s%02d" % (kind, j)
            tiny = b"<DOC><DOCNO>%s</DOCNO> %s </DOC>" % (z.encode(), bef(n))
            assert len(tiny) == 40 < MIN_FAST
            c.emit([("R", a, dict(kind=kind, cut=j)), HEAD % a.encode(), ("X",), TAIL, ("E",), b"\n",
                    ("R", z, dict(fast=False, expect=[bef(n)], kind=kind, cut=j)), ("K", tiny), ("A", j), tiny, ("E",),
                    b"\n"], kind)
    return c


def family_records_slow(mis):
    """Slow records (unterminated comment, attribute tags, script) across the edge
    between fast ones, a slow record over a whole chunk and one over more than
    two, and a fast record of 50 KiB."""
    c = Corpus("S", mis)
    slow = [(b"<!-- hq380 never closed ", {"hidden": [b"hq380"], "aft_hidden": True, "fast": False}),
            (b"<a href=\"x\">", {"fast": False}),
            (b"<script> hq381 </script>", {"hidden": [b"hq381"], "fast": False}),
            (b"<img src='y' />", {"fast": False})]
    c.place_all(_specs(slow, kinds="CL"))
    for docid, nbytes in (("S950WHOLE", CHUNK + 600), ("S951TWOCHUNKS", 2 * CHUNK + 600)):
        n = c.serial()
        c.plain("S94%sPRE" % docid[3])
        c.emit([("R", docid, dict(fast=False, expect=[bef(n), aft(n)], kind="C")), HEAD % docid.encode(), ("X",),
                bef(n) + b" ", ("K", b"<a href=\"x\">"), ("A", 300), b"<a href=\"x\">", ("F", nbytes), aft(n), TAIL, ("E",),
                b"\n"], "C")
        r = c.recs[-1]
        assert r["rs"] < c.anchors[-1][0] and c.anchors[-1][0] + nbytes - 600 < r["re"]  # whole chunks inside
        c.plain("S94%sPOST" % docid[3])
    n = c.serial()
    c.emit([("R", "S960FAST50K", dict(expect=[bef(n), aft(n)], kind="N")), HEAD % b"S960FAST50K", bef(n), ("F", 50 * 1024),
            aft(n), TAIL, ("E",), b"\n"])
    return c


def _b36(i, w):
    s = ""
    for _ in range(w):
        s = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"[i % 36] + s
        i //= 36
    return s


def family_window(mis):
    """The record window and the token rounds: 800 records of exactly 48 bytes back
    to back (about 341 to a chunk, under REC_WIN), 800 alternating 48 and 47
    (every other one slow), 800 of 48 bytes 64 apart; a three-chunk record of
    single letters (8192 tokens a chunk: four rounds, the densest the token
    stream's (rs >> 1) + i addressing allows); and a three-chunk record of
    distinct 4-byte tokens (more than TOK_CAP tokens and more than TOK_MISS new
    raw tokens in every round)."""
    c = Corpus("D", mis)
    k = 0
    for run, (lens, gap) in enumerate((((48,), b""), ((48, 47), b""), ((48,), b" " * 16))):
        for i in range(800):
            ln = lens[i % len(lens)]
            docid = "Q" + _b36(k, 3)
            w1, w2 = b"v%06d" % k, b"x%07d" % k
            body = b" " + w1 + b" " + w2 + b" " * (ln - 47)
            rec = b"<DOC><DOCNO>" + docid.encode() + b"</DOCNO>" + body + b"</DOC>"
            assert len(rec) == ln
            c.emit([("R", docid, dict(fast=ln >= MIN_FAST, expect=[w1, w2], kind="N")), rec, ("E",), gap])
            k += 1
        c.buf += b"\n"
    assert 800 * 48 > 2 * CHUNK and CHUNK // 48 + 2 <= REC_WIN
    letters = b"".join(bytes([97 + i % 26, 32]) for i in range(3 * CHUNK // 2))
    c.emit([("R", "D970LETTERS", dict(kind="N")), HEAD % b"D970LETTERS", letters, TAIL, ("E",), b"\n"])
    assert CHUNK // 2 > 3 * TOK_CAP
    four = bytearray()
    for i in range(3 * CHUNK // 5):
        four += bytes([97 + i % 26, 97 + i // 26 % 26, 97 + i // 676 % 26, 122]) + b" "
    assert CHUNK // 5 > TOK_CAP + TOK_MISS
    c.emit([("R", "D971DISTINCT", dict(kind="N")), HEAD % b"D971DISTINCT", bytes(four), TAIL, ("E",), b"\n"])
    c.plain("D972AFTER")
    return c


FAMILIES = {
    "tokens_short": family_tokens_short, "tokens_long": family_tokens_long, "utf8": family_utf8,
    "tags": family_tags, "comments": family_comments, "pis": family_pis, "comments_long": family_comments_long,
    "entities": family_entities, "entities_long": family_entities_long, "entities_end": family_entities_end,
    "records": family_records, "records_slow": family_records_slow, "window": family_window,
}
MIS = (0, 1, 8, 15)

_cache = {}


def corpus(family, mis):
    """The family's corpus for one misalignment, built once."""
    key = (family, mis)
    if key not in _cache:
        _cache[key] = FAMILIES[family](mis)
    return _cache[key]


# ---------------------------------------------------------------------------
# the neighbours
# ---------------------------------------------------------------------------
def dense_lt():
    """k_scan_lt's overflow path: more than LT_BUF '<' in one 16 KiB step.  A fast
    record of <b> x 6000 between words; a slow one of <a x> x 4000 with fast
    records before, between and after; a 20 KiB run of '<' inside a record (every
    one complex: slow) and once more as junk between records."""
    c = Corpus("L", 0)
    n = c.serial()
    assert 6000 * 3 > CHUNK and CHUNK // 3 > LT_BUF
    c.emit([("R", "L100BOLD", dict(expect=[bef(n), aft(n)], kind="N")), HEAD % b"L100BOLD", ("F", MINFILL), bef(n) + b" ",
            b"<b>" * 6000, b" " + aft(n), ("F", MINFILL), TAIL, ("E",), b"\n"])
    c.plain("L101BETWEEN")
    n = c.serial()
    c.emit([("R", "L102ATTR", dict(fast=False, expect=[bef(n), aft(n)], kind="N")), HEAD % b"L102ATTR", ("F", MINFILL),
            bef(n) + b" ", b"<a x>" * 4000, b" " + aft(n), ("F", MINFILL), TAIL, ("E",), b"\n"])
    c.plain("L103BETWEEN")
    n = c.serial()
    c.emit([("R", "L104RUN", dict(fast=False, expect=[bef(n)], kind="N")), HEAD % b"L104RUN", ("F", MINFILL), bef(n) + b" ",
            b"<" * 20480, b" ", ("F", MINFILL), TAIL, ("E",), b"\n"])
    c.plain("L105BETWEEN")
    c.buf += b"<" * 20480 + b" \n"
    c.plain("L106AFTER")
    return c


def docid_window():
    """k_docno's 96-byte window, whose start depends on (rs + mis) & 15: records
    <DOC> + w bytes of spaces and newlines + <DOCNO> id </DOCNO> for w over
    38 .. 100 (55 .. 100 alone leaves start offsets 14 and 15 without a docid
    inside the window), each at every record start offset rs & 15, so </DOCNO> ends on
    every side of window byte 96 and <DOCNO> itself straddles it (w 84 .. 91 and
    around); the same with a 2-byte character in the docid around byte 96."""
    c = Corpus("K", 0)
    k = 0
    for uni in (False, True):
        for w in (range(70, 90) if uni else range(38, 101)):
            for al in range(16):
                c.buf += b" " * ((al - len(c.buf)) % 16)
                docid = ("Ké%04d" if uni else "KA%04d") % k
                n = c.serial()
                ws = (b" \n" * w)[:w]
                c.emit([("R", docid, dict(expect=[bef(n)], kind="N", w=w, al=al)), b"<DOC>" + ws + b"<DOCNO> ",
                        docid.encode("utf-8"), b" </DOCNO>\n", bef(n), ("F", 30), b"</DOC>", ("E",), b"\n"])
                assert c.recs[-1]["rs"] % 16 == al
                k += 1
    return c
