"""TEST INFRASTRUCTURE: a sequential model of the deflate's entropy stage (deflate_kernels.hip:
em_build_codes, wave_build_lengths64, the run-length header and the block-type compare of
em_segment), in plain Python integers.  Never used by the product path.

tests/test_huff_fit.py pins it to tests/cpp/huff_fit_test.cpp --lengths / --plan, which run the
functions the kernels compile (csrc/huff_fit.h); tests/test_gpu_deflate_entropy.py then asks the
kernels for exactly this model's lengths, header, block type and size."""
from collections import namedtuple

LIT, DIST, PRE = ("lit", 286, 9), ("dist", 30, 6), ("pre", 19, 7)
PERM = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]  # symbols 257..285
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]          # symbols 0..29
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def raw_len(f, F):
    """round(log2(F / f)) for 0 < f <= F: the largest L with (f 2^L)^2 <= 2 F^2 (never a tie:
    the square root of 2 is irrational)."""
    L = 0
    while ((f << (L + 1)) ** 2) <= 2 * F * F:
        L += 1
    return L


def init_len(f, F, maxbits):
    return max(1, min(maxbits, raw_len(f, F))) if f else 0


def fit_classes(cnt, maxbits):
    """Kraft repair, then slack fill, on the class sizes cnt[1..maxbits] (in place).
    Returns (symbols lengthened by the repair, slack-fill passes)."""
    U = 1 << maxbits
    K = sum(cnt[L] << (maxbits - L) for L in range(1, maxbits + 1))
    moved = 0
    while K > U:
        for L in range(maxbits - 1, 0, -1):
            if K > U and cnt[L]:
                gain = 1 << (maxbits - L - 1)
                k = min(-(-(K - U) // gain), cnt[L])
                cnt[L] -= k
                cnt[L + 1] += k
                K -= k * gain
                moved += k
    R, passes = U - K, 0
    while R and passes < 64:
        changed = False
        for L in range(2, maxbits + 1):
            w = 1 << (maxbits - L)
            if cnt[L] and w <= R:
                k = min(cnt[L], R // w)
                cnt[L] -= k
                cnt[L - 1] += k
                R -= k * w
                changed = True
        if not changed:
            break
        passes += 1
    return moved, passes


Build = namedtuple("Build", "lens moved passes clamped")


def build(freq, alpha):
    """Code lengths of freq under alphabet (name, nsym, maxbits), with what the fit did."""
    name, nsym, maxbits = alpha
    freq = list(freq) + [0] * (nsym - len(freq))
    lens = [0] * nsym
    used = [s for s in range(nsym) if freq[s]]
    if len(used) <= 1:  # two codes of length 1
        u = used[-1] + 1 if used else 0
        lens[u - 1 if u else 0] = 1
        lens[1 if u <= 1 else 0] = 1
        return Build(lens, 0, 0, 0)
    F = sum(freq)
    cnt = [0] * 17
    keys = []
    for s in used:
        L0 = init_len(freq[s], F, maxbits)
        cnt[L0] += 1
        if name == "pre":  # the precode's 64-key sort: frequency descending, then symbol
            keys.append((-freq[s], s))
        else:              # (initial length, less frequent half of the class behind, symbol)
            keys.append((2 * L0 + (1 if (freq[s] << L0) <= F else 0), s))
    clamped = sum(1 for s in used if raw_len(freq[s], F) > maxbits)  # held at the limit
    moved, passes = fit_classes(cnt, maxbits)
    keys.sort()
    r = 0
    for L in range(1, maxbits + 1):
        for _ in range(cnt[L]):
            lens[keys[r][1]] = L
            r += 1
    return Build(lens, moved, passes, clamped)


def lengths(freq, alpha):
    return build(freq, alpha).lens


def canonical(lens):
    """RFC 1951 3.2.2: {symbol: (length, code)}, codes MSB first."""
    bl = [0] * 17
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (l, nxt[l])
            nxt[l] += 1
    return out


def plan_run(v, r):
    """Code-length symbols of a run of r lengths v, as (symbol, repeat) in writing order."""
    out = []
    if v == 0:
        while r >= 138:
            out.append((18, 138))
            r -= 138
        if r >= 11:
            out.append((18, r))
        elif r >= 3:
            out.append((17, r))
        else:
            out += [(0, 1)] * r
        return out
    out.append((v, 1))
    r -= 1
    while r >= 6:
        out.append((16, 6))
        r -= 6
    if r >= 3:
        out.append((16, r))
    else:
        out += [(v, 1)] * r
    return out


Header = namedtuple("Header", "hlit hdist hclen prelens syms bits")


def header(litlens, distlens):
    """The dynamic header of the two code-length sequences: runs never span HLIT/HDIST."""
    hlit = max(257, max(s + 1 for s in range(286) if litlens[s]))
    hdist = max(1, max(s + 1 for s in range(30) if distlens[s]))
    syms = []
    for seq in (litlens[:hlit], distlens[:hdist]):
        i = 0
        while i < len(seq):
            j = i
            while j < len(seq) and seq[j] == seq[i]:
                j += 1
            syms += plan_run(seq[i], j - i)
            i = j
    prefreq = [0] * 19
    for s, _ in syms:
        prefreq[s] += 1
    prelens = lengths(prefreq, PRE)
    hclen = max(4, max(i + 1 for i in range(19) if prelens[PERM[i]]))
    extra = {16: 2, 17: 3, 18: 7}
    bits = 14 + 3 * hclen + sum(prelens[s] + extra.get(s, 0) for s, _ in syms)
    return Header(hlit, hdist, hclen, prelens, syms, bits)


Block = namedtuple("Block", "btype nbytes bits litlens distlens hdr dyn_bits fix_bits stored_bytes lit distb")


def block(lit_hist, dist_hist, nb, final):
    """What em_segment emits for a segment of nb input bytes whose tokens have these histograms
    (lit_hist without the end-of-block, which is added here).  btype 0 / 1 / 2; nbytes: the
    segment's bytes in the stream (the block, and unless final the padding and the empty stored
    block); bits: the block's own bits (None when stored)."""
    lit = list(lit_hist) + [0] * (286 - len(lit_hist))
    lit[256] += 1
    dist = list(dist_hist) + [0] * (30 - len(dist_hist))
    lb, db = build(lit, LIT), build(dist, DIST)
    ll, dl = lb.lens, db.lens
    hdr = header(ll, dl)
    lx = lambda s: LEN_EXTRA[s - 257] if s > 256 else 0
    dyn_tok = sum(lit[s] * (ll[s] + lx(s)) for s in range(286)) + sum(dist[s] * (dl[s] + DIST_EXTRA[s]) for s in range(30))
    fix_tok = sum(lit[s] * (FIXED_LIT[s] + lx(s)) for s in range(286)) + sum(dist[s] * (5 + DIST_EXTRA[s]) for s in range(30))
    dyn_bits, fix_bits = 3 + hdr.bits + dyn_tok, 3 + fix_tok
    use_dyn = dyn_bits <= fix_bits
    bits = dyn_bits if use_dyn else fix_bits
    hbytes = (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4
    nsto = 2 if nb > 65535 else 1
    stored_bytes = 5 * nsto + nb + (0 if final else 5)
    if hbytes < stored_bytes:
        return Block(2 if use_dyn else 1, hbytes, bits, ll, dl, hdr, dyn_bits, fix_bits, stored_bytes, lb, db)
    return Block(0, stored_bytes, None, ll, dl, hdr, dyn_bits, fix_bits, stored_bytes, lb, db)


def byte_hist(data):
    h = [0] * 286
    for b, n in enumerate(_count(data)):
        h[b] = n
    return h


def _count(data):
    import numpy as np
    return np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=256).tolist()
