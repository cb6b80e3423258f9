"""TEST INFRASTRUCTURE: a bit-level reader of raw DEFLATE (RFC 1951) that returns one record per
block -- where it starts and ends, its header fields as written, its codes, the histogram of its
tokens and their bit count.  Plain Python; never used by the product path.

``read_block`` decodes a block's tokens, or -- given the block's token histograms -- skips them:
the end then follows from the code lengths (a level-1 segment costs a header parse, not 32768
symbol decodes); the end-of-block code is still read at the place that arithmetic gives.
``blocks`` walks a whole stream, ``segments`` a libdmx stream: per input segment one block (two
stored blocks above 65535 bytes), then, unless BFINAL, the padding and the empty stored block
``00 00 FF FF`` that byte-aligns the next segment."""
PERM = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class FormatError(ValueError):
    pass


class Block:
    """start, end: bit positions; btype 0 / 1 / 2.  Dynamic: hlit (257..), hdist (1..), hclen
    (4..), prelens[19], clsyms [(code-length symbol, repeat)], litlens[hlit], distlens[hdist]
    (fixed blocks carry the fixed lengths).  lit_hist[286] (end-of-block included), dist_hist[30],
    token_bits (extra bits and end-of-block included), header_bits; stored: length."""

    def __init__(self):
        self.start = self.end = self.bfinal = self.btype = 0
        self.hlit = self.hdist = self.hclen = None
        self.prelens = self.clsyms = None
        self.litlens = self.distlens = None
        self.lit_hist, self.dist_hist = [0] * 286, [0] * 30
        self.token_bits = self.header_bits = 0
        self.length = None
        self.data_start = None  # stored: byte offset of the data

    @property
    def bits(self):
        return self.end - self.start


def kraft(lens):
    """Kraft sum of a code as a fraction of 2^15 (complete: 32768)."""
    return sum(1 << (15 - l) for l in lens if l)


def _table(lens):
    """(lookup by the next maxlen bits, LSB first) -> (symbol, length); None where no code."""
    mx = max(lens) if lens else 0
    if mx == 0:
        return None, 0
    bl = [0] * (mx + 2)
    for l in lens:
        if l:
            bl[l] += 1
    if sum(bl[l] << (mx - l) for l in range(1, mx + 1)) > (1 << mx):
        raise FormatError("over-subscribed code")
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    tab = [None] * (1 << mx)
    for s, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        rev = int(format(c, "0%db" % l)[::-1], 2)
        for hi in range(1 << (mx - l)):
            tab[rev | (hi << l)] = (s, l)
    return tab, mx


class _Bits:
    def __init__(self, data, pos=0):
        self.b = bytes(data)
        self.n = 8 * len(self.b)
        self.p = pos

    def peek(self, n):
        i = self.p >> 3
        return (int.from_bytes(self.b[i:i + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        if self.p + n > self.n:
            raise FormatError("stream ends inside a block")
        x = self.peek(n)
        self.p += n
        return x

    def sym(self, tab, mx):
        e = tab[self.peek(mx)] if tab else None
        if e is None:
            raise FormatError("no such code")
        self.p += e[1]
        if self.p > self.n:
            raise FormatError("stream ends inside a block")
        return e[0]


def read_block(data, pos=0, out=None, hist=None):
    """The block at bit `pos`.  out: a bytearray the decoded bytes are appended to (matches copy
    from it).  hist = (lit_hist without end-of-block or with it, dist_hist): the tokens are not
    decoded; their bits follow from the lengths, and `out` is left alone."""
    br = _Bits(data, pos)
    b = Block()
    b.start = pos
    b.bfinal = br.get(1)
    b.btype = br.get(2)
    if b.btype == 3:
        raise FormatError("BTYPE 3")
    if b.btype == 0:
        br.p = (br.p + 7) & ~7
        ln, nln = br.get(16), br.get(16)
        if ln != (~nln & 0xFFFF):
            raise FormatError("LEN / NLEN")
        if br.p + 8 * ln > br.n:
            raise FormatError("stored block runs past the stream")
        b.length, b.data_start = ln, br.p >> 3
        b.header_bits = br.p - pos
        if out is not None and hist is None:
            out += br.b[b.data_start:b.data_start + ln]
        b.end = br.p + 8 * ln
        return b
    if b.btype == 1:
        b.litlens, b.distlens = list(FIXED_LIT), list(FIXED_DIST)
    else:
        b.hlit, b.hdist, b.hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
        b.prelens = [0] * 19
        for i in range(b.hclen):
            b.prelens[PERM[i]] = br.get(3)
        ptab, pmx = _table(b.prelens)
        lens, b.clsyms = [], []
        while len(lens) < b.hlit + b.hdist:
            x = br.sym(ptab, pmx)
            if x < 16:
                rep, v = 1, x
            elif x == 16:
                if not lens:
                    raise FormatError("16 with nothing to repeat")
                rep, v = 3 + br.get(2), lens[-1]
            elif x == 17:
                rep, v = 3 + br.get(3), 0
            else:
                rep, v = 11 + br.get(7), 0
            b.clsyms.append((x, rep))
            lens += [v] * rep
        if len(lens) != b.hlit + b.hdist:
            raise FormatError("a repeat runs past HLIT + HDIST")
        b.litlens, b.distlens = lens[:b.hlit], lens[b.hlit:]
    b.header_bits = br.p - pos
    ltab, lmx = _table(b.litlens)
    ll = b.litlens + [0] * (288 - len(b.litlens))
    if not ll[256]:
        raise FormatError("no end-of-block code")
    if hist is not None:
        lh, dh = list(hist[0]) + [0] * (286 - len(hist[0])), list(hist[1]) + [0] * (30 - len(hist[1]))
        lh[256] = 1
        dl = b.distlens + [0] * (30 - len(b.distlens))
        if any(lh[s] and not ll[s] for s in range(286)) or any(dh[s] and not dl[s] for s in range(30)):
            raise FormatError("a symbol of the histogram has no code")
        b.lit_hist, b.dist_hist = lh, dh
        b.token_bits = (sum(lh[s] * (ll[s] + (LEN_EXTRA[s - 257] if s > 256 else 0)) for s in range(286)) +
                        sum(dh[s] * (dl[s] + DIST_EXTRA[s]) for s in range(30)))
        br.p += b.token_bits - ll[256]
        if br.sym(ltab, lmx) != 256:
            raise FormatError("no end-of-block where the histogram puts it")
        b.end = br.p
        return b
    dtab, dmx = _table(b.distlens)
    t0 = br.p
    lh, dh = b.lit_hist, b.dist_hist
    while True:
        x = br.sym(ltab, lmx)
        if x >= 286:
            raise FormatError("lit/len symbol 286 / 287")
        lh[x] += 1
        if x < 256:
            if out is not None:
                out.append(x)
        elif x == 256:
            break
        else:
            L = LEN_BASE[x - 257] + br.get(LEN_EXTRA[x - 257])
            d = br.sym(dtab, dmx)
            if d >= 30:
                raise FormatError("distance symbol 30 / 31")
            dh[d] += 1
            dist = DIST_BASE[d] + br.get(DIST_EXTRA[d])
            if out is not None:
                if dist > len(out):
                    raise FormatError("distance beyond the output")
                if dist >= L:
                    out += out[len(out) - dist:len(out) - dist + L]
                else:
                    for _ in range(L):
                        out.append(out[-dist])
    b.token_bits = br.p - t0
    b.end = br.p
    return b


def blocks(data, out=None):
    """Every block of the stream up to and including the BFINAL one."""
    pos, res = 0, []
    while True:
        b = read_block(data, pos, out)
        res.append(b)
        pos = b.end
        if b.bfinal:
            return res


def fixed_bits(b):
    """The block's tokens under the fixed code, with the 3 header bits."""
    return 3 + (sum(b.lit_hist[s] * (FIXED_LIT[s] + (LEN_EXTRA[s - 257] if s > 256 else 0)) for s in range(286)) +
                sum(b.dist_hist[s] * (5 + DIST_EXTRA[s]) for s in range(30)))


class Segment:
    """blocks: the segment's own blocks (one; two when stored above 65535 bytes); start, end:
    byte offsets in the stream (end: behind the empty stored block unless final); final."""

    def __init__(self, blocks, start, end, final):
        self.blocks, self.start, self.end, self.final = blocks, start, end, final

    @property
    def block(self):
        return self.blocks[0]


def segments(data, sizes, hists=None, out=None):
    """A libdmx stream of len(sizes) segments with these input sizes.  hists[i] (optional): the
    token histograms of segment i, see read_block."""
    res, pos = [], 0
    for i, nb in enumerate(sizes):
        if pos & 7:
            raise FormatError("a segment starts inside a byte")
        h = hists[i] if hists is not None else None
        b = read_block(data, pos, out, h)
        bl = [b]
        if b.btype == 0 and b.length != nb:  # the stored form of more than 65535 bytes: two blocks
            if b.bfinal or nb <= 65535 or b.length != 32768:
                raise FormatError("stored block of %d bytes in a segment of %d" % (b.length, nb))
            b2 = read_block(data, b.end, out, h)
            if b2.btype != 0 or b2.length != nb - 32768:
                raise FormatError("second stored block")
            bl.append(b2)
        last = bl[-1]
        end = last.end
        if not last.bfinal:
            e = read_block(data, end)
            if e.btype != 0 or e.bfinal or e.length != 0:
                raise FormatError("no empty stored block behind a segment that is not final")
            if e.end - end > 3 + 7 + 32:
                raise FormatError("padding")
            end = e.end
        elif i + 1 != len(sizes):
            raise FormatError("BFINAL before the last segment")
        end = (end + 7) & ~7
        res.append(Segment(bl, bl[0].start >> 3, end >> 3, bool(last.bfinal)))
        pos = end
    if pos != 8 * len(data):
        raise FormatError("%d bytes behind the last segment" % (len(data) - pos // 8))
    return res
