"""CPU model of the literal prefix of a run segment's parse (32 KiB level-2 front kernel,
DESIGN 4.1, "Literal prefix").

The kernel's rule, as deflate_kernels.hip states it: fm is the first position >= D whose match
bit is set, at most nb.  The token bits of [D, fm) are set by bitmap word before the walk; a
parse chunk [lo, hi) with hi <= fm walks nothing and records hi - 1 as its last token; the chunk
that holds fm starts its walk at fm with fm - 1 as its last token so far; every other chunk walks
from lo.  This is checked against the position-by-position walk (a position without a match bit
is a literal; one with a bit is a match of its length clipped at the chunk end, or a literal when
its length is below 3, a fingerprint collision) on random bitmaps: same token bitmap, same last
token of every chunk.
"""
import random

CHUNK = 258


def walk(bits, length, lo, hi, p, lastp, tok):
    """The walk of chunk [lo, hi) from p on: token starts into tok, returns the last one."""
    while p < hi:
        tok.add(p)
        lastp = p
        L = min(length[p], hi - p) if bits[p] else 1
        p += L if L >= 3 else 1
    return lastp


def parse_plain(bits, length, D, nb):
    tok, last = set(), []
    for lo in range(D, nb, CHUNK):
        last.append(walk(bits, length, lo, min(lo + CHUNK, nb), lo, lo, tok))
    return tok, last


def parse_prefixed(bits, length, D, nb):
    fm = next((q for q in range(D, nb) if bits[q]), nb)
    tok, last = set(), []
    # by bitmap word, as the kernel does it
    for w in range(D // 32, (nb + 31) // 32):
        a, b = max(D, 32 * w), min(fm, 32 * w + 32)
        tok.update(range(a, b))
    for lo in range(D, nb, CHUNK):
        hi = min(lo + CHUNK, nb)
        if hi <= fm:
            last.append(hi - 1)
        elif fm > lo:
            last.append(walk(bits, length, lo, hi, fm, fm - 1, tok))
        else:
            last.append(walk(bits, length, lo, hi, lo, lo, tok))
    return tok, last


def cases():
    rng = random.Random(1906)
    firsts = (0, 1, 3, 31, 32, 33, 257, 258, 259, 515, 516, 2047, 2048, 5000)
    for D in (0, 1, 257, 4096):
        for first in firsts:
            for trial in range(3):
                nb = D + rng.choice((6000, 5999, 258 * 20, 258 * 20 + 1, first + 1, first + 4, first + 300))
                if nb <= D:
                    continue
                density = rng.choice((0.02, 0.3, 1.0))
                bits = [False] * nb
                for q in range(D + first, nb):
                    bits[q] = rng.random() < density
                if D + first < nb and trial != 2:
                    bits[D + first] = True
                for q in range(D):  # the dictionary's bits are not the parse's
                    bits[q] = rng.random() < 0.5
                length = [rng.choice((1, 2, 3, 4, 17, 258)) for _ in range(nb)]
                yield bits, length, D, nb


def test_prefixed_walk_is_the_plain_walk():
    n = skipped_chunks = 0
    for bits, length, D, nb in cases():
        want, got = parse_plain(bits, length, D, nb), parse_prefixed(bits, length, D, nb)
        assert got == want, (D, nb)
        fm = next((q for q in range(D, nb) if bits[q]), nb)
        skipped_chunks += (fm - D) // CHUNK
        n += 1
    assert n >= 150 and skipped_chunks >= 100


def test_no_bit_at_all():
    """fm = nb: every chunk is literals."""
    nb = 258 * 3 + 7
    tok, last = parse_prefixed([False] * nb, [1] * nb, 0, nb)
    assert tok == set(range(nb)) and last == [257, 515, 773, nb - 1]
