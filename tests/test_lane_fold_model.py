"""Model of the lane decoder's run fold (inflate_lanes.hip, step()): a step whose
symbol is an accepted match (L, d) of c bits takes n copies of it at once when the low c bits of
the 64-bit window stand n times in it, n <= FOLD_MAX, n c <= STEP_BITS, outpos + n L <= CAP and
the merged word's 16-bit length holds.  For random complete codes (<= 9 / <= 6 bits) and bit
strings with runs, folded stepping must give the token words, the output size, the flag and the
final bit position of one-symbol stepping -- also for copies that lie past the end-of-block
(the bits behind it are random here) and with the bounds set low enough to bite.
"""
import pytest

import lenient_streams as LS
from golden.quirk_streams import BitWriter, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, canonical

FOLD_MAX, STEP_BITS = 4, 42


def table(lengths, B):
    T = [None] * (1 << B)
    for sym, (code, l) in canonical(lengths).items():
        r = int(format(code, "0%db" % l)[::-1], 2)
        for hi in range(1 << (B - l)):
            T[r | (hi << l)] = (sym, l)
    return T


def decode(LT, DT, bits, bp, cap, lenmax, fold):
    """Token words [("lit", bytes) | ("match", L, d)], outpos, flag, final bp."""
    words, pend, outpos, flag = [], None, 0, None
    while flag is None:
        win = (bits >> bp) & ((1 << 64) - 1)
        sym, cl = LT[win & 511]
        if sym == 256:
            bp += cl
            break
        if sym < 256:
            bp += cl
            if outpos >= cap:
                flag = "cap"
            elif pend and pend[0] == "lit" and len(pend[1]) < 3:
                pend = ("lit", pend[1] + [sym])
                outpos += 1
            else:
                words.append(pend)
                pend = ("lit", [sym])
                outpos += 1
            continue
        k = sym - 257
        L = LEN_BASE[k] + ((win >> cl) & ((1 << LEN_EXTRA[k]) - 1))
        n1 = cl + LEN_EXTRA[k]
        ds, dcl = DT[(win >> n1) & 63]
        d = DIST_BASE[ds] + ((win >> (n1 + dcl)) & ((1 << DIST_EXTRA[ds]) - 1))
        c = n1 + dcl + DIST_EXTRA[ds]
        if d > outpos:
            flag = "far"
        elif outpos + L > cap:
            flag = "cap"
        if flag:
            bp += c
            break
        cont = bool(pend) and pend[0] == "match" and pend[2] == d and pend[1] + L <= lenmax
        n = 1
        if fold:
            P = win & ((1 << c) - 1)
            base = pend[1] if cont else 0
            for k in range(2, FOLD_MAX + 1):
                if not (k * c <= min(64, STEP_BITS) and (win >> ((k - 1) * c)) & ((1 << c) - 1) == P
                        and outpos + k * L <= cap and base + k * L <= lenmax):
                    break
                n = k
        bp += n * c
        outpos += n * L
        if cont:
            pend = ("match", pend[1] + n * L, d)
        else:
            words.append(pend)
            pend = ("match", n * L, d)
    return [w for w in words + [pend] if w], outpos, flag, bp


def random_stream(R):
    """Codes, and a block of literals and runs of equal matches, random bits behind its end."""
    hlit, hdist = 286, 30
    LL = LS.make_lens(R, hlit, R.between(8, 60), [256, 285, 257 + R.below(28)], 9)
    DL = LS.make_lens(R, hdist, R.between(2, 12), [R.below(4), R.below(30)], 6)
    lc, dc = canonical(LL), canonical(DL)
    lits = [s for s in lc if s < 256]
    lens = [s for s in lc if s > 256]
    bw = BitWriter()
    bw.put(R.below(1 << 7), R.below(8))  # any bit phase
    start = 8 * len(bw.out) + bw.n
    outn = 0
    for _ in range(R.between(1, 40)):
        near = [k for k in sorted(dc) if DIST_BASE[k] + (1 << DIST_EXTRA[k]) - 1 <= outn]
        if lits and (R.chance(40) or not near):
            for _ in range(R.between(1, 5)):
                bw.put_code(*lc[R.pick(lits)])
                outn += 1
            continue
        ls, ds = R.pick(lens), R.pick(near) if near and not R.chance(5) else R.pick(sorted(dc))
        ex, dx = R.below(1 << LEN_EXTRA[ls - 257]), R.below(1 << DIST_EXTRA[ds])
        for i in range(R.pick([1, 1, 2, 3, 4, 5, 7, 8, 9, 13, 40])):
            outn += LEN_BASE[ls - 257] + ex
            bw.put_code(*lc[ls])
            bw.put(ex, LEN_EXTRA[ls - 257])
            bw.put_code(*dc[ds])
            # (now and then the last bit sent differs: the run is broken inside a copy)
            bw.put(dx ^ (1 << (DIST_EXTRA[ds] - 1)) if DIST_EXTRA[ds] and R.chance(4) else dx, DIST_EXTRA[ds])
    if R.chance(70):
        bw.put_code(*lc[256])
    for _ in range(40):
        bw.put(R.below(1 << 16), 16)
    bw.align()
    return table(LL, 9), table(DL, 6), int.from_bytes(bw.bytes(), "little"), start


@pytest.mark.parametrize("cap,lenmax", [(32768, 0xFFFF), (3000, 0xFFFF), (5000, 1400), (700, 600)])
def test_folded_steps_equal_single_steps(cap, lenmax):
    folded = 0
    for seed in range(300):
        LT, DT, bits, start = random_stream(LS.Rng(0x5EED0000 | seed))
        one = decode(LT, DT, bits, start, cap, lenmax, False)
        many = decode(LT, DT, bits, start, cap, lenmax, True)
        assert many == one, seed
        folded += any(w[0] == "match" and w[1] > 258 for w in one[0])
    assert folded > 50  # the streams do hold runs
