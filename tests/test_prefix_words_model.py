"""CPU model of the two groupings of a run segment's tokens into words (32 KiB level-2 front
kernel, DESIGN 4.1, "Prefix words in closed form").

The old grouping, by bitmap word: thread t owns the 32 token-start bits of tokmap[t], splits them
into matches (a candidate) and literals, and makes one word per match and one per group of up to
three adjacent literals, a group ending at a match and at the bitmap word's end.  The new one takes
the literal prefix [D, fm) out of that: fm (run_fm in the kernel) is the first match bit at or
above D, at most nb; the prefix is W0 = ceil(P / 3) words, word k the positions D + 3k .. D + 3k +
min(3, P - 3k) - 1, and thread t words only the bits of its bitmap word at or above fm, its words
starting at W0 + (its exclusive scan).  Both are modelled with the kernel's bit operations and read
back position by position:

* the token sequence of the new words is the old one's (the emission codes every word on its own,
  so the stream depends on nothing else);
* the words tile [0, total) without gap or overlap;
* the new total is at most 17408, the token buffer's bound, and at most the old total -- except
  that a literal AT fm (a match bit whose match turned out shorter than 3, a fingerprint collision)
  which the old grouping put into one word with the prefix's last literals now starts a word of its
  own: one word more at the most, and only then.
"""
import random

import pytest

NT = 1024
M32 = 0xFFFFFFFF
CAP = 17408


def popc(x):
    return bin(x).count("1")


def thread_words(m, nz, base):
    """The kernel's per-thread words of the token bits m (nz: positions with a candidate):
    [(kind, first position, count)] in order."""
    mt, lt = m & nz, m & ~nz & M32
    chain = lt & (lt << 1) & (lt << 2) & (lt << 3) & M32
    ws = lt & ~(lt << 1) & M32
    for _ in range(10):
        ws |= (ws << 3) & chain & M32
    out = []
    every = mt | ws
    assert popc(every) == popc(mt) + popc(ws)
    while every:
        b = (every & -every).bit_length() - 1
        every &= every - 1
        if (mt >> b) & 1:
            out.append(("M", base + b, 1))
        else:
            x = lt >> b
            out.append(("L", base + b, 1 + ((x >> 1) & 1) + ((x >> 1) & (x >> 2) & 1)))
    return out


def place(per_thread, first):
    """Words laid out at first + exclusive scan of the threads' counts: {offset: word}."""
    at, off = {}, first
    for words in per_thread:
        for w in words:
            assert off not in at
            at[off] = w
            off += 1
    return at, off


def old_words(tokmap, nzmap):
    at, total = place([thread_words(tokmap[t], nzmap[t], 32 * t) for t in range(NT)], 0)
    return at, total


def new_words(tokmap, nzmap, D, fm):
    P = fm - D
    W0 = (P + 2) // 3
    at = {}
    for k in range(W0):  # (thread k mod NT in the kernel)
        at[k] = ("L", D + 3 * k, min(3, P - 3 * k))
    per_thread = []
    for t in range(NT):
        fr = fm - 32 * t
        m = 0 if fr >= 32 else tokmap[t] & ((M32 << fr) & M32 if fr > 0 else M32)
        per_thread.append(thread_words(m, nzmap[t], 32 * t))
    rest, total = place(per_thread, W0)
    assert not set(rest) & set(at)
    at.update(rest)
    return at, total


def sequence(at, total):
    """The tokens the words hold, in word order; the words tile [0, total)."""
    assert sorted(at) == list(range(total))
    seq = []
    for k in range(total):
        kind, p, c = at[k]
        seq += [(kind, p + i) for i in range(c)]
    return seq


def segment(rng, D, P, nb, at_fm, style):
    """Token and candidate bitmaps of a run segment: literals on [D, D + P), then tokens up to nb.
    at_fm: the token at fm is a match ('M') or a literal ('L', a collision).  style: what follows
    -- 'run' (maximal matches to the end), 'mixed' (literals and short matches, then the run),
    'dense' (literal, match of three, ...: the most words per position)."""
    tok, nz = [0] * NT, [0] * NT
    fm = min(D + P, nb)

    def put(p, match):
        tok[p >> 5] |= 1 << (p & 31)
        if match:
            nz[p >> 5] |= 1 << (p & 31)

    for p in range(D, fm):
        put(p, False)
    p = fm
    first = True
    mixed_end = fm + (nb - fm) // 2
    while p < nb:
        if first:
            match = at_fm == "M"
        elif style == "dense":
            match = ((p - fm) % 4) == (0 if at_fm == "M" else 1)
        elif style == "mixed" and p < mixed_end:
            match = rng.random() < 0.5
        else:
            match = True
        first = False
        if match and nb - p >= 3:
            put(p, True)
            p += 3 if style == "dense" else min(rng.choice((3, 4, 17, 258)) if p < mixed_end and style == "mixed" else 258, nb - p)
        else:
            put(p, False)
            p += 1
    # (positions inside a match keep stale candidates in the kernel: set some)
    for t in range(NT):
        nz[t] |= rng.getrandbits(32) & ~tok[t] & M32
    # the prefix positions have no candidate: their match bit is clear
    for q in range(D, fm):
        nz[q >> 5] &= ~(1 << (q & 31)) & M32
    return tok, nz, fm


PREFIXES = (0, 1, 2, 3, 4, 5, 31, 32, 33, 95, 96, 97, 251, 1023, 1024, 1025, 3000, 3001, 3002, 9999, 20000)


def cases():
    rng = random.Random(2011)
    for di, D in enumerate((0, 1, 33, 4096)):
        for pi, P in enumerate(PREFIXES):
            for at_fm in ("M", "L"):
                # (over the four D, each style meets every P with either token at fm)
                style = ("run", "mixed", "dense")[(di + pi) % 3]
                nb = D + rng.choice((32768 - D, 32767 - D, 32765 - D, P + 4099, P + 2051))
                nb = min(nb, 32768)
                if D + P + 3 > nb:
                    continue
                yield D, P, nb, at_fm, style, segment(rng, D, P, nb, at_fm, style)


def test_new_words_hold_the_old_token_sequence():
    n = 0
    seen_p, seen_mod = set(), set()
    for D, P, nb, at_fm, style, (tok, nz, fm) in cases():
        assert fm == D + P
        old_at, old_total = old_words(tok, nz)
        new_at, new_total = new_words(tok, nz, D, fm)
        want, got = sequence(old_at, old_total), sequence(new_at, new_total)
        assert got == want, (D, P, nb, at_fm, style)
        assert [p for _, p in got] == sorted(p for _, p in got)
        assert len(got) == sum(popc(x) for x in tok)
        assert new_total <= CAP, (D, P, nb, at_fm, style, new_total)
        if at_fm == "M":
            assert new_total <= old_total, (D, P, nb, style, new_total, old_total)
        else:  # (see the module's text)
            assert new_total <= old_total + 1, (D, P, nb, style, new_total, old_total)
        seen_p.add(P)
        seen_mod.add(P % 3)
        n += 1
    assert {0, 1, 2, 3, 4} <= seen_p and seen_mod == {0, 1, 2} and n >= 150


def test_collision_at_fm_is_the_only_extra_word():
    """One literal of the prefix left in fm's bitmap word, a literal at fm, then a match: the old
    grouping has one word for both literals, the new one two."""
    rng = random.Random(5)
    tok, nz, fm = segment(rng, 0, 34, 32768, "L", "run")
    _, old_total = old_words(tok, nz)
    _, new_total = new_words(tok, nz, 0, fm)
    assert new_total == old_total + 1
    # with a match at fm the prefix is never dearer: ceil(P / 3) <= the sum over the bitmap words
    tok, nz, fm = segment(rng, 0, 34, 32768, "M", "run")
    assert new_words(tok, nz, 0, fm)[1] == old_words(tok, nz)[1]


@pytest.mark.parametrize("D", (0, 33))
def test_no_match_bit_at_all(D):
    """run_fm = nb: every position a literal, every word a prefix word, the threads hold none."""
    nb = 32765
    tok, nz = [0] * NT, [0] * NT
    for p in range(D, nb):
        tok[p >> 5] |= 1 << (p & 31)
    new_at, new_total = new_words(tok, nz, D, nb)
    assert new_total == (nb - D + 2) // 3 <= old_words(tok, nz)[1]
    assert sequence(new_at, new_total) == [("L", p) for p in range(D, nb)]


def test_capacity_of_the_densest_tail():
    """Literal, match of three, ... from fm on (two words per four positions) behind every prefix
    length mod 3 and mod 32: at most 17408 words."""
    rng = random.Random(7)
    worst = 0
    for P in list(range(0, 70)) + [251, 1024, 3001]:
        for at_fm in ("M", "L"):
            tok, nz, fm = segment(rng, 0, P, 32768, at_fm, "dense")
            worst = max(worst, new_words(tok, nz, 0, fm)[1])
    assert worst <= CAP
