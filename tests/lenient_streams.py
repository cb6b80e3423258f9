"""Seeded generator of small adversarial DEFLATE streams (TEST INFRASTRUCTURE ONLY).

Every stream the GPU suite decodes otherwise comes from a well-behaved encoder.  The reference
inflate is far more lenient than RFC 1951 (oracle/inflate_oracle.c restates its rules), and
libdmx restates those rules in several separately written decoders.  The families below aim at
the rules no encoder exercises:

  prefix      complete codes up to 15 bits (random leaf splitting); HLIT up to 288, HDIST up to
              32; codes for length symbols 286/287 and distance symbols 30/31, used in the
              payload; matches (258, 1), distance == bytes so far, == bytes so far + 1, 32768
  incomplete  the same with 20 % of the lengths zeroed and a single-code or empty distance code;
              a marked subset ("bad") steps onto an unassigned prefix (-> DATA)
  oversub     1-4 extra codes in the lit/len code, the distance code or the precode; the payload
              is chosen with the lookup model, collision winners first
  overshoot   the lit/len (or distance) sequence ends in a 17/18 run past its count (dropped) or
              in a 16 run past it with a non-zero length (symbols above 285 / 29 get codes)
  sixteen     a 16 right after a 17/18, a 16 as the first distance symbol, a 16 as the very
              first symbol
  longheader  precodes of 15-19 symbols of 5-7 bits, (almost) no repeats: code-length sections
              beyond 1938 bits; variants put the lit/dist switch just before / after that bit
  fixedodd    fixed-code blocks with 286/287, 30/31, far and overlapping copies; stored blocks
              with LEN 0, 1, LEN == all the input left, LEN one more than that, a wrong NLEN; a
              non-final BTYPE 3
  truncated   the cases of incomplete, oversub and longheader, each cut at 3 seeded byte
              positions inside the interesting block (case i: base family i % 3, base case i // 9);
              the first cut of a bad case falls inside its unassigned pattern, where "no code"
              and "out of input" compete

lane_case() is no family: `prefix`-style blocks inside the table limits of libdmx's lane decoder,
the filler of the many-segments stream.  fixed_run() is a long run of fixedodd Huffman blocks.

A repeat can overshoot its count by at most 5 entries (a 16 that starts at index 287 writes
up to 292), so in the reference's two-sequence reading no stream reaches index 300: the
"index >= 300 -> DATA" rule of the oracle is unreachable there and no family claims it.

Every case starts with 0..3 empty fixed blocks (the interesting block at bit 0, 10, 20, 30), is
at most 4 KiB long and decodes to at most 32 KiB.  Randomness is drawn only through
random.Random(seed).getrandbits, so the bytes do not depend on the Python version.

Code assignment follows the reference (FlatHuffmanTree::construct as oracle/inflate_oracle.c
restates it): canonical over (length, value), a code that overflows its length keeps the low k
bits as its key.  `Lookup` is the model of the reference's lookup: the first length whose key
hits, the last insert wins, and the precode also requires code == bits.
"""
import functools
import hashlib
import random

from golden.quirk_streams import (BitWriter, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, PERM,
                                  huffman_lengths, rle_ops)

FAMILIES = ["prefix", "incomplete", "oversub", "overshoot", "sixteen", "longheader", "fixedodd", "truncated"]
TRUNC_BASES = ["incomplete", "oversub", "longheader"]
N_CASES = 1024          # cases per family the manifest covers (the batch routes take them all)
LONG_BITS = 1938        # 2048 - 110: beyond this the header reader refills its window
MAX_STREAM = 4096
MAX_OUT = 32768


class Rng:
    def __init__(self, seed):
        self.g = random.Random(seed).getrandbits

    def below(self, n):
        return self.g(32) % n

    def between(self, a, b):
        return a + self.below(b - a + 1)

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def chance(self, pct):
        return self.below(100) < pct

    def shuffle(self, lst):
        for i in range(len(lst) - 1, 0, -1):
            j = self.below(i + 1)
            lst[i], lst[j] = lst[j], lst[i]


class Lookup:
    """The reference's dictionary of (length, key) -> symbol for one code."""

    def __init__(self, lengths, exact=False):
        self.exact = exact
        self.tab = {}
        self.code = [None] * len(lengths)   # symbol -> (key, length)
        self.collided = set()               # symbols that overwrote an earlier insert
        bl = [0] * 17
        for L in lengths:
            if L:
                bl[L] += 1
        nxt, c = [0] * 16, 0
        for b in range(1, 16):
            c = (c + bl[b - 1]) << 1
            nxt[b] = c
        for k in range(1, 16):
            for v, L in enumerate(lengths):
                if L != k:
                    continue
                c = nxt[k]
                nxt[k] += 1
                key = c & ((1 << k) - 1)
                if (k, key) in self.tab:
                    self.collided.add(v)
                self.tab[(k, key)] = (v, c)
                self.code[v] = (key, k)

    def decode(self, bits, n):
        """bits: n bits in reading order (first bit read = most significant) -> (symbol, length)
        of the first length that hits, or None."""
        for k in range(1, min(n, 15) + 1):
            x = bits >> (n - k)
            e = self.tab.get((k, x))
            if e and (not self.exact or e[1] == x):
                return e[0], k
        return None

    def usable(self):
        """The symbols whose own key decodes as themselves."""
        return [v for v, ck in enumerate(self.code) if ck and self.decode(ck[0], ck[1]) == (v, ck[1])]

    def unassigned(self, bits, r):
        """True when r real bits followed by zeros hit at no length (a window zero-padded past
        the stream end finds "no code" there)."""
        return self.decode(bits << (15 - r), 15) is None


class Case:
    def __init__(self):
        self.stream = b""
        self.family = ""
        self.far_by = 0         # how far a copy reached before the first byte of the case's output
        self.bad = False        # the payload steps onto an unassigned prefix on purpose
        self.hdr_bits = 0       # bits of the code-length section of the interesting block
        self.block = (0, 0)     # byte range of the interesting block
        self.codes = []         # (bit position, length, Lookup, key) of every Huffman code in it
        self.max_sym = 0        # highest lit/len index that got a code
        self.bad_at = None      # index in codes of the unassigned pattern of a bad case
        self.unassigned = False  # truncated: the last real bits lie on an unassigned prefix
        self.note = ""


# ---- code construction -------------------------------------------------------------------
def split_lengths(R, m, maxd=15):
    """Depths of the m leaves of a random full binary tree, none deeper than maxd."""
    if m == 1:
        return [1]
    leaves = [1, 1]
    c = [0, 1]  # the leaves that can still split, in index order
    while len(leaves) < m:
        i = max(c, key=leaves.__getitem__) if R.chance(35) else R.pick(c)
        leaves[i] += 1
        leaves.append(leaves[i])
        if leaves[i] < maxd:
            c.append(len(leaves) - 1)
        else:
            c.remove(i)
    return leaves


def make_lens(R, n, m, forced=(), maxd=15):
    """n code lengths, m of them non-zero and forming a complete code of at most maxd bits;
    `forced` get one."""
    syms = sorted(set(s for s in forced if s < n))
    rest = [s for s in range(n) if s not in syms]
    R.shuffle(rest)
    syms = (syms + rest)[:max(m, len(syms))]
    depths = split_lengths(R, len(syms), maxd)
    R.shuffle(depths)
    L = [0] * n
    for s, d in zip(syms, depths):
        L[s] = d
    return L


def apply_ops(ops, count):
    """The lengths the reference builds from one code-length sequence of `count` entries
    (overshoot kept, 16 repeats the last literal length, initially 0), capped at 300."""
    lens, last = [], 0
    for s, v, _ in ops:
        assert len(lens) < count
        if s < 16:
            lens.append(s)
            last = s
        elif s == 16:
            lens += [last] * (3 + v)
        elif s == 17:
            lens += [0] * (3 + v)
        else:
            lens += [0] * (11 + v)
    assert len(lens) >= count
    return lens[:300]


def default_precode(ops):
    pf = [0] * 19
    for s, _, _ in ops:
        pf[s] += 1
    if sum(1 for x in pf if x) < 2:
        pf[0 if pf[0] == 0 else 1] += 1
    return huffman_lengths(pf, 7)


class Writer:
    """One case being written: the bit writer, the output size so far and the records."""

    def __init__(self, R, case):
        self.R = R
        self.bw = BitWriter()
        self.case = case
        self.outn = 0

    def pos(self):
        return 8 * len(self.bw.out) + self.bw.n

    def code(self, lk, sym):
        key, k = lk.code[sym]
        self.case.codes.append((self.pos(), k, lk, key))
        self.bw.put_code(key, k)

    def header(self, hlit, hdist, ops, plen):
        bw = self.bw
        pre = Lookup(plen, exact=True)
        hclen = 19
        while hclen > 4 and plen[PERM[hclen - 1]] == 0:
            hclen -= 1
        bw.put(hlit - 257, 5)
        bw.put(hdist - 1, 5)
        bw.put(hclen - 4, 4)
        for i in range(hclen):
            bw.put(plen[PERM[i]], 3)
        p0 = self.pos()
        for s, v, nb in ops:
            self.code(pre, s)
            if nb:
                bw.put(v, nb)
        self.case.hdr_bits = self.pos() - p0

    def literal(self, lit, s):
        self.code(lit, s)
        self.outn += 1

    def match(self, lit, dist, ls, extra, ds, dextra):
        self.code(lit, ls)
        L = 0
        if ls <= 285:
            L = LEN_BASE[ls - 257] + extra
            if LEN_EXTRA[ls - 257]:
                self.bw.put(extra, LEN_EXTRA[ls - 257])
        self.code(dist, ds)
        d = 0
        if ds < 30:
            d = DIST_BASE[ds] + dextra
            if DIST_EXTRA[ds]:
                self.bw.put(dextra, DIST_EXTRA[ds])
        if L and d:
            if d > self.outn:
                self.case.far_by = max(self.case.far_by, d - self.outn)
            else:
                self.outn += L

    def payload(self, lit, dist, ntok, special=False, prefer=(), bad=False):
        """Tokens on usable codes only, then the end of block.  special: the edge matches of the
        `prefix` family; prefer: symbols to use early; bad: stop on an unassigned prefix."""
        R = self.R
        lu, du = lit.usable(), dist.usable()
        lits = [s for s in lu if s < 256]
        lens = [s for s in lu if s > 256]
        odd = [s for s in lens if s > 285] + [s for s in prefer if s in lens]
        dodd = [s for s in du if s >= 30] + [s for s in prefer if s in du]
        for s in prefer:
            if s in lits:
                self.literal(lit, s)
        bad_at = R.below(ntok + 1) if bad else -1
        far_ok = R.chance(12)  # few cases copy from far before their own output
        targets = []
        for t in range(ntok):
            if len(self.bw.out) > MAX_STREAM - 600 or self.outn > MAX_OUT - 260:
                break
            if t == bad_at and self.bad_code(lit, dist, lens, du):
                return False
            if lens and du and (R.chance(30) or not lits):
                ls = R.pick(odd) if odd and R.chance(30) else R.pick(lens)
                ex = R.below(1 << LEN_EXTRA[ls - 257]) if ls <= 285 else 0
                near = [s for s in du if s < 30 and DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1 <= self.outn]
                if not near and lits and not far_ok:
                    self.literal(lit, R.pick(lits))
                    continue
                ds = R.pick(dodd) if dodd and R.chance(25) else R.pick(near) if near and not (far_ok and R.chance(20)) else R.pick(du)
                dx = R.below(1 << DIST_EXTRA[ds]) if ds < 30 else 0
                if special and R.chance(50):
                    if not targets:
                        targets = [(285, 1), (0, self.outn), (0, self.outn + 1), (0, 32768 if far_ok else 0)]
                    wl, wd = targets.pop(0)
                    wd = wd or (self.outn if R.chance(50) else self.outn + 1)
                    if 1 <= wd <= 32768:
                        k = max(i for i in range(30) if DIST_BASE[i] <= wd)
                        if k in du:
                            ds, dx = k, wd - DIST_BASE[k]
                            if wl in lens:
                                ls, ex = wl, 0
                self.match(lit, dist, ls, ex, ds, dx)
            elif lits:
                self.literal(lit, R.pick(lits))
            else:
                break
        if bad and self.bad_code(lit, dist, lens, du):
            return False
        if 256 in lu:
            self.code(lit, 256)
        else:
            self.case.note += " no-eob"
        return True

    def bad_code(self, lit, dist, lens, du):
        """15 bits no lit/len code matches, or a length symbol and then 16 bits no distance code
        matches; then two zero bytes, so the error is DATA and not an over-read."""
        R = self.R
        if lens and R.chance(50):
            ls = R.pick(lens)
            for _ in range(64):
                p = R.below(1 << 15) | (0x7000 if R.chance(30) else 0)
                if dist.decode(p, 15) is None:
                    self.code(lit, ls)
                    if ls <= 285 and LEN_EXTRA[ls - 257]:
                        self.bw.put(0, LEN_EXTRA[ls - 257])
                    self.case.bad_at = len(self.case.codes)
                    self.case.codes.append((self.pos(), 15, dist, p))
                    self.bw.put_code(p, 15)
                    self.bw.put(R.below(2), 1)
                    self.bw.put(0, 16)
                    self.case.note += " bad-dist"
                    return True
        for _ in range(64):
            p = R.below(1 << 15) | (0x7000 if R.chance(30) else 0)
            if lit.decode(p, 15) is None:
                self.case.bad_at = len(self.case.codes)
                self.case.codes.append((self.pos(), 15, lit, p))
                self.bw.put_code(p, 15)
                self.bw.put(0, 16)
                self.case.note += " bad-lit"
                return True
        return False


# ---- the families --------------------------------------------------------------------------
def _hlit_hdist(R):
    return (R.pick([257, 258, 285, 286, 287, 288, R.between(257, 288)]),
            R.pick([1, 2, 29, 30, 31, 32, R.between(1, 32)]))


def _plain_codes(R, hlit, hdist, maxl=15, maxd=15):
    forced = [256, R.below(256), 257] + [s for s in (285, 286, 287) if s < hlit]
    m = R.pick([R.between(len(forced), 24), R.between(len(forced), hlit), hlit])
    LL = make_lens(R, hlit, m, forced, maxl)
    if hdist == 1:
        DL = [1]
    else:
        dforced = [0] + [s for s in (29, 30, 31) if s < hdist]
        DL = make_lens(R, hdist, R.between(max(2, len(dforced)), hdist), dforced, maxd)
    return LL, DL


def _dyn(W, hlit, hdist, lops, dops, plen=None, ntok=None, **kw):
    """Write header and payload of one dynamic block from its two code-length sequences; the
    codes are the ones the reference really builds from them."""
    R = W.R
    LLa, DLa = apply_ops(lops, hlit), apply_ops(dops, hdist)
    lit, dist = Lookup(LLa), Lookup(DLa)
    W.case.max_sym = max([s for s, L in enumerate(LLa) if L] or [0])
    W.header(hlit, hdist, lops + dops, plen or default_precode(lops + dops))
    return W.payload(lit, dist, R.between(1, 160) if ntok is None else ntok, **kw)


def fam_prefix(W):
    R = W.R
    hlit, hdist = _hlit_hdist(R)
    LL, DL = _plain_codes(R, hlit, hdist)
    _dyn(W, hlit, hdist, rle_ops(LL), rle_ops(DL), special=True)


def fam_incomplete(W, i):
    R = W.R
    hlit, hdist = _hlit_hdist(R)
    LL, DL = _plain_codes(R, hlit, hdist)
    for s in range(hlit):
        if LL[s] and R.chance(20) and (s != 256 or R.chance(10)):
            LL[s] = 0
    if not any(LL):
        LL[256] = 1
    DL = [0] * hdist
    if R.chance(60):
        DL[R.below(hdist)] = R.between(1, 15)
    W.case.bad = i % 3 == 2
    _dyn(W, hlit, hdist, rle_ops(LL), rle_ops(DL), bad=W.case.bad)


def fam_oversub(W, i):
    R = W.R
    hlit, hdist = _hlit_hdist(R)
    hlit, hdist = max(hlit, 262), max(hdist, 6)
    LL, DL = _plain_codes(R, hlit, hdist)
    where = i % 3
    extra = R.between(1, 4)
    plen = None
    if where < 2:
        T = LL if where == 0 else DL
        used = sorted(set(x for x in T if x))
        free = [s for s, x in enumerate(T) if not x]
        R.shuffle(free)
        for s in free[:extra]:
            T[s] = R.pick(used) if R.chance(50) else used[-1]
    lops, dops = rle_ops(LL), rle_ops(DL)
    if where == 2:
        # extra precode symbols: keep the draw whose needed symbols all still decode exactly
        need = set(s for s, _, _ in lops + dops)
        base = default_precode(lops + dops)
        # (the first draws take any length; the later ones 7 bits, which disturbs fewest)
        for attempt in range(48):
            plen = list(base)
            free = [s for s in range(19) if not plen[s]]
            R.shuffle(free)
            for s in free[:max(1, extra - attempt // 12)]:
                plen[s] = R.pick([x for x in plen if x] + [7]) if attempt < 8 else 7
            if need <= set(Lookup(plen, exact=True).usable()):
                break
        W.case.note += " precode"
    lk = Lookup(apply_ops(lops, hlit)) if where == 0 else Lookup(apply_ops(dops, hdist))
    _dyn(W, hlit, hdist, lops, dops, plen, prefer=sorted(lk.collided) if where < 2 else ())
    if where < 2 and lk.collided & set(lk.usable()):
        W.case.note += " collision"


def fam_overshoot(W, i):
    R = W.R
    hlit, hdist = _hlit_hdist(R)
    LL, DL = _plain_codes(R, hlit, max(hdist, 2))
    hdist = len(DL)
    kind = i % 4

    def tail(T, count, nonzero):
        """T[:count] re-encoded so that its last run overshoots `count`."""
        if nonzero:  # ... v, then a 16 that starts t entries before the end and repeats more
            t = R.between(1, min(5, count - 1))
            head = T[:count - t]
            if not head[-1]:
                head[-1] = R.pick([x for x in T if x])
            return rle_ops(head) + [(16, R.between(max(t + 1, 3), 6) - 3, 2)]
        t = R.between(1, min(10, count - 1))
        head = T[:count - t]
        if R.chance(50) or t > 8:
            return rle_ops(head) + [(18, R.between(max(t + 1, 11), 138) - 11, 7)]
        return rle_ops(head) + [(17, R.between(max(t + 1, 3), 10) - 3, 3)]

    lops, dops = rle_ops(LL), rle_ops(DL)
    if kind in (0, 1):
        lops = tail(LL, hlit, kind == 1)
    else:
        dops = tail(DL, hdist, kind == 3)
    prefer = [s for s in range(hlit, 300)] if kind == 1 else [s for s in range(hdist, 40)] if kind == 3 else []
    _dyn(W, hlit, hdist, lops, dops, prefer=prefer)


def fam_sixteen(W, i):
    R = W.R
    hlit, hdist = _hlit_hdist(R)
    LL, DL = _plain_codes(R, hlit, max(hdist, 4))
    hdist = len(DL)
    kind = i % 3
    lops, dops = rle_ops(LL), rle_ops(DL)
    r = R.between(3, 6)
    if kind == 0:    # ... literal v, 17/18 of n zeros, 16 of r: r more entries of v
        n = R.pick([3, R.between(3, 10), R.between(11, 40)])
        p = R.between(1, hlit - n - r)
        zeros = [(17, n - 3, 3)] if n <= 10 else [(18, n - 11, 7)]
        lops = rle_ops(LL[:p]) + zeros + [(16, r - 3, 2)] + rle_ops(LL[p + n + r:])
    elif kind == 1:  # 16 as the first distance symbol: r zeros
        dops = [(16, r - 3, 2)] + rle_ops(DL[r:]) if hdist > r else [(16, r - 3, 2)]
    else:            # 16 as the very first symbol: r zeros
        lops = [(16, r - 3, 2)] + rle_ops(LL[r:])
    _dyn(W, hlit, hdist, lops, dops)


def fam_longheader(W, i):
    R = W.R
    variant = i % 4  # 0: switch just after bit LONG_BITS, 1: just before, 2: runs (16s), 3: free
    hlit = R.between(280, 288) if variant != 3 else R.between(257, 288)
    hdist = R.between(28, 32) if variant != 3 else R.between(2, 32)
    if variant < 2:
        # the bit of the lit/dist switch, counted from the 32-bit word the HLIT field starts
        # in, with 19 precode lengths and 7 bits per code length
        at = (W.pos() & 31) + 14 + 3 * 19
        want = LONG_BITS + (R.between(4, 56) if variant == 0 else -R.between(4, 56))
        hlit = max(257, min(288, (want - at) // 7))
    LL = make_lens(R, hlit, hlit - R.below(4), [256])
    DL = make_lens(R, hdist, hdist - R.below(2), [0])
    if variant == 2:  # gather equal lengths into a few runs, so some 16s appear (one near the refill)
        for at in (R.between(1, 200), R.between(255, 272), R.between(1, hlit - 8)):
            v = LL[at]
            same = [j for j in range(hlit) if LL[j] == v and not at <= j < at + 6]
            for k in range(1, 6):
                if same and LL[at + k] != v:
                    j = same.pop()
                    LL[j], LL[at + k] = LL[at + k], LL[j]
        lops = rle_ops(LL)
    else:
        lops = [(v, 0, 0) for v in LL]
    dops = [(v, 0, 0) for v in DL]
    order = list(range(19))
    R.shuffle(order)
    keep = set(order[:R.between(15, 19)]) | set(s for s, _, _ in lops + dops)
    if variant < 2:
        keep = set(range(19))
    plen = [0] * 19
    for s in keep:
        plen[s] = 7 if variant < 2 else R.between(5, 7)
    _dyn(W, hlit, hdist, lops, dops, plen, ntok=R.between(1, 60))


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_LIT, FIXED_DIST = Lookup(_FIXED_LL), Lookup([5] * 32)


def fixed_block(W, ntok, final):
    W.bw.put(1 if final else 0, 1)
    W.bw.put(1, 2)
    W.payload(FIXED_LIT, FIXED_DIST, ntok)


def fam_fixedodd(W, final):
    R = W.R
    bw = W.bw
    nb = R.between(1, 4)
    for b in range(nb):
        last = b == nb - 1
        fin = 1 if last and final else 0
        kind = R.pick(["fixed", "fixed", "fixed", "len0", "len1", "nlen", "btype3", "rest", "toolong"])
        if kind in ("rest", "toolong") and not (last and final):
            kind = "fixed"
        if kind == "btype3" and last:
            kind = "fixed"
        if kind == "fixed":
            fixed_block(W, R.between(0, 120), fin)
            continue
        if kind == "btype3":
            bw.put(0, 1)
            bw.put(3, 2)
            continue
        bw.put(fin, 1)
        bw.put(0, 2)
        bw.align()
        n = {"len0": 0, "len1": 1}.get(kind, R.between(2, 300))
        stated = n + 1 if kind == "toolong" else n
        bw.put(stated, 16)
        bw.put(R.below(65536) if kind == "nlen" else stated ^ 0xFFFF, 16)
        for _ in range(n):
            bw.put(R.below(256), 8)
        W.outn += n
        W.case.note += " " + kind


def make_case(family, i, final=True, keep_codes=False):
    """Case i of a family (not `truncated`): one stream; final=False leaves the interesting
    block (for fixedodd: the last block) non-final and ends the stream byte-aligned with an
    empty stored block (00 00 FF FF), for a caller that appends more.  keep_codes: keep the
    record of every Huffman code and its Lookup (what a truncation needs; some 100 KB a case, so
    the cached cases do without)."""
    R = Rng((FAMILIES.index(family) << 24) | i)
    c = Case()
    c.family = family
    W = Writer(R, c)
    bw = W.bw
    for _ in range(R.below(4)):  # empty fixed blocks: 0 01 0000000
        bw.put(0, 1)
        bw.put(1, 2)
        bw.put(0, 7)
    b0 = W.pos() // 8
    if family == "fixedodd":
        fam_fixedodd(W, final)
    else:
        bw.put(1 if final else 0, 1)
        bw.put(2, 2)
        if family == "prefix":
            fam_prefix(W)
        elif family == "incomplete":
            fam_incomplete(W, i)
        elif family == "oversub":
            fam_oversub(W, i)
        elif family == "overshoot":
            fam_overshoot(W, i)
        elif family == "sixteen":
            fam_sixteen(W, i)
        elif family == "longheader":
            fam_longheader(W, i)
        else:
            raise ValueError(family)
    if final:
        bw.align()
    else:
        bw.empty_stored()
    c.stream = bw.bytes()
    c.block = (b0, len(c.stream))
    assert len(c.stream) <= MAX_STREAM
    if not keep_codes:
        c.codes, c.bad_at = (), None
    return c


@functools.lru_cache(maxsize=4)
def _truncation_base(fam, idx):
    return make_case(fam, idx, keep_codes=True)


def lane_case(i, final=False):
    """A `prefix`-style case inside the table limits of libdmx's lane decoder (one block, at bit
    0; HLIT <= 286, 2 <= HDIST <= 30; complete lit/len codes of at most 9 bits, distance codes of at most 6;
    plain RFC run-length coding): a segment the lanes decode themselves, where the families'
    cases are segments they must decline."""
    R = Rng((len(FAMILIES) << 24) | i)
    c = Case()
    c.family = "lane"
    W = Writer(R, c)
    W.bw.put(1 if final else 0, 1)
    W.bw.put(2, 2)
    hlit = R.pick([257, 258, 285, 286, R.between(257, 286)])
    hdist = R.pick([2, 29, 30, R.between(2, 30)])
    LL, DL = _plain_codes(R, hlit, hdist, 9, 6)
    _dyn(W, hlit, hdist, rle_ops(LL), rle_ops(DL), ntok=R.between(1, 40), special=True)
    if final:
        W.bw.align()
    else:
        W.bw.empty_stored()
    c.stream = W.bw.bytes()
    c.block = (0, len(c.stream))
    c.codes = ()
    return c


def truncated_case(i):
    """Case i of `truncated`: base family i % 3, base case i // 9, cut (i // 3) % 3."""
    fam = TRUNC_BASES[i % 3]
    base = _truncation_base(fam, i // 9)
    R = Rng((FAMILIES.index("truncated") << 24) | i)
    b0, b1 = base.block
    cut = R.between(min(b0 + 1, b1 - 1), max(b1 - 1, b0 + 1)) if b1 - b0 > 1 else b0
    if base.bad_at is not None and (i // 3) % 3 == 0:
        # the first cut of a bad case falls inside its unassigned pattern; of the byte positions
        # there, the model picks one whose real bits stay unassigned when zeros follow
        pos, k, lk, key = base.codes[base.bad_at]
        inside = [b for b in range(pos // 8 + 1, (pos + k - 1) // 8 + 1) if pos < 8 * b < pos + k]
        good = [b for b in inside if lk.unassigned(key >> (k - (8 * b - pos)), 8 * b - pos)]
        if good or inside:
            cut = R.pick(good or inside)
    c = Case()
    c.family = "truncated"
    c.note = "%s[%d] cut at %d of %d" % (fam, i // 9, cut, b1)
    c.stream = base.stream[:cut]
    c.far_by, c.hdr_bits, c.block = base.far_by, base.hdr_bits, (b0, cut)
    end = 8 * cut
    for pos, k, lk, key in base.codes:
        if pos < end < pos + k:
            r = end - pos
            c.unassigned = lk.unassigned(key >> (k - r), r)
    return c


@functools.lru_cache(maxsize=None)
def cases(family, n=N_CASES, final=True):
    """The first n cases of a family (shared between tests: do not modify)."""
    if family == "truncated":
        return tuple(truncated_case(i) for i in range(n))
    return tuple(make_case(family, i, final) for i in range(n))


def expected(oracle, stream, rfc=False):
    """(bytes, None) or (None, oracle error code: -1 over-read, -2 data) for one stream."""
    from oracle_bind import CheckerError
    try:
        return oracle.inflate(stream, rfc=rfc), None
    except CheckerError as e:
        return None, e.code


@functools.lru_cache(maxsize=None)
def _expected_all(family, n, rfc):
    from oracle_bind import Oracle
    o = Oracle()
    return tuple(expected(o, c.stream, rfc) for c in cases(family, n))


def expected_all(family, n=N_CASES, rfc=False):
    """expected() of the first n cases of a family, computed once per process."""
    return _expected_all(family, n, rfc)


def streams_digest(family, n=N_CASES):
    h = hashlib.sha256()
    for c in cases(family, n):
        h.update(c.stream)
    return h.hexdigest()


def records_digest(outputs):
    """Digest over the (length, SHA-256) records of the outputs of a family's decodable cases, in
    case order (None entries -- cases that do not decode -- are skipped)."""
    h = hashlib.sha256()
    for out in outputs:
        if out is not None:
            h.update(("%d %s\n" % (len(out), hashlib.sha256(out).hexdigest())).encode())
    return h.hexdigest()


def fixed_run(seed, nbytes, lo=2000, hi=4000, before_start=False):
    """Consecutive fixedodd Huffman blocks (no stored block, none byte-aligned) of lo..hi tokens
    each and at least nbytes in all, the last one final: literals, length symbols up to 287 and
    distance symbols up to 31, overlapping copies and copies from up to 32768 back; with
    before_start also copies that reach before the first byte of the output (they copy nothing)."""
    c = Case()
    W = Writer(Rng(seed), c)
    R = W.R
    while len(W.bw.out) < nbytes:
        W.bw.put(0, 1)
        W.bw.put(1, 2)
        for _ in range(R.between(lo, hi)):
            if not R.chance(25):
                W.literal(FIXED_LIT, R.below(256))
                continue
            ls = R.between(257, 287)
            ds = R.between(0, 31)
            if ds < 30 and not before_start:  # a distance symbol that stays inside the output
                near = [k for k in range(30) if DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1 <= W.outn]
                if not near:
                    W.literal(FIXED_LIT, R.below(256))
                    continue
                ds = R.pick(near)
            W.match(FIXED_LIT, FIXED_DIST, ls, R.below(1 << LEN_EXTRA[ls - 257]) if ls <= 285 else 0,
                    ds, R.below(1 << DIST_EXTRA[ds]) if ds < 30 else 0)
        W.code(FIXED_LIT, 256)
    W.bw.put(1, 1)
    W.bw.put(1, 2)
    W.code(FIXED_LIT, 256)
    W.bw.align()
    assert before_start or not c.far_by
    return W.bw.bytes()
