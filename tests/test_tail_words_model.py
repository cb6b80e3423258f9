"""CPU model of the two token-word writers of the 32 KiB level-2 front kernel (DESIGN 4.1,
"Run-segment token writer").

Both are written here once, as deflate_kernels.hip states them.  A token word is a match
(1 << 31 | L - 3 << 16 | d - 1) or a literal run (count << 24 | up to three bytes, first lowest);
a literal word is closed by a match, when it holds three bytes, and at the end of its writer's
share of the tokens:

* by range: thread t of 1024 owns tokens [t K, (t + 1) K) in position order, K = ceil(tokens / 1024);
* by word (segments with a terminal run): thread t owns the tokens that start in
  [32 t, 32 t + 32), the set bits of its token-start bitmap word.

k_deflate_emit codes every word on its own (one symbol per literal, two per match), so a stream
depends only on the symbol sequence the words decode to.  Checked on seeded random valid token
sequences over 32768 positions: both groupings decode to the same sequence, and the by-word
grouping stays inside the token buffer: <= 17 words per bitmap word, <= 17408 =
deflate_tok_stride(32768) - 224 per segment.
"""
import random

import pytest

SEG = 32768
NT = 1024
CAP_WORD = 17
CAP_SEG = 17408


def words_of(tokens):
    """The words one writer makes of its share of the tokens ((p, L, d): d = 0 is the literal L)."""
    out, lit, nl = [], 0, 0
    for _, L, d in tokens:
        if d:
            if nl:
                out.append(lit | nl << 24)
            lit = nl = 0
            out.append(1 << 31 | (L - 3) << 16 | (d - 1))
        else:
            lit |= L << (8 * nl)
            nl += 1
            if nl == 3:
                out.append(lit | 3 << 24)
                lit = nl = 0
    if nl:
        out.append(lit | nl << 24)
    return out


def by_range(tokens):
    K = (len(tokens) + NT - 1) // NT
    return [words_of(tokens[t * K:(t + 1) * K]) for t in range(NT)]


def by_word(tokens):
    own = [[] for _ in range(SEG // 32)]
    for tok in tokens:
        own[tok[0] // 32].append(tok)
    return [words_of(o) for o in own]


def decode(per_thread):
    syms = []
    for words in per_thread:
        for w in words:
            if w >> 31:
                syms.append(("M", ((w >> 16) & 0xFF) + 3, (w & 0x7FFF) + 1))
            else:
                syms.extend(("L", (w >> (8 * i)) & 0xFF) for i in range((w >> 24) & 3))
    return syms


def symbols(tokens):
    return [("M", L, d) if d else ("L", L) for _, L, d in tokens]


def parse(nb, rng, p_match, max_len, start=()):
    """A valid token sequence over [0, nb): `start` fixes the first tokens as lengths (1 = a
    literal), the rest are matches of 3..max_len with probability p_match, literals otherwise."""
    toks, p, forced = [], 0, list(start)
    while p < nb:
        L = forced.pop(0) if forced else (rng.randint(3, max_len) if rng.random() < p_match else 1)
        L = min(L, nb - p)
        if L < 3:
            toks.extend((p + i, rng.randrange(256), 0) for i in range(L))
        else:
            toks.append((p, L, rng.randint(1, 32768)))
        p += L
    return toks


def build_cases():
    rng = random.Random(20311)
    cases = {}
    for p_match, max_len in ((0.0, 3), (0.02, 258), (0.3, 258), (0.5, 3), (0.5, 8), (0.9, 4), (0.9, 258), (1.0, 3), (1.0, 258)):
        for nb in (SEG, SEG - 3, 258 * 40 + 2):
            cases[f"mix_p{p_match}_L{max_len}_n{nb}"] = parse(nb, rng, p_match, max_len)
    # a match on bit 31 and on bit 0 of a bitmap word, after 1..4 literals and before them
    for bit in (31, 0):
        for k in (1, 2, 3, 4):
            head = [1] * (32 * 7 + bit - k - 5) + [5] + [1] * k + [rng.randint(3, 40)] + [1] * k
            cases[f"match_bit{bit}_lit{k}"] = parse(SEG, rng, 0.3, 258, start=head)
    # literal runs of 1..7 across a word edge: a of them before the edge at 320, the rest after it
    for n in range(1, 8):
        for a in range(0, n + 1):
            # (nine matches of 33 end at 297; two more end at 320 - a, the second of length 4)
            cases[f"litrun{n}_before{a}"] = parse(SEG, rng, 0.2, 100, start=[33] * 9 + [19 - a, 4] + [1] * n + [9])
    return cases


CASES = build_cases()


def worst_case(phase):
    """`L MMM` repeated from position `phase`: phase 2 puts every match on bits 3, 7, ... 31."""
    rng = random.Random(phase)
    return parse(SEG, rng, 0.0, 3, start=[1] * phase + [1, 3] * ((SEG - phase) // 4))


@pytest.mark.parametrize("name", sorted(CASES))
def test_groupings_decode_alike(name):
    toks = CASES[name]
    assert decode(by_word(toks)) == symbols(toks)
    assert decode(by_range(toks)) == symbols(toks)


@pytest.mark.parametrize("name", sorted(CASES))
def test_by_word_capacity(name):
    per = by_word(CASES[name])
    assert max(len(w) for w in per) <= CAP_WORD
    assert sum(len(w) for w in per) <= CAP_SEG


def test_litrun_cases_cross_the_edge():
    """The constructed literal runs lie where they are meant to: a literals before 320."""
    for n in range(1, 8):
        for a in range(0, n + 1):
            toks = {p: d for p, _, d in CASES[f"litrun{n}_before{a}"]}
            run = range(320 - a, 320 - a + n)
            assert all(toks.get(p) == 0 for p in run), (n, a)
            assert toks.get(320 - a - 4, 0) != 0 and toks.get(320 - a + n, 0) != 0, (n, a)


@pytest.mark.parametrize("phase", (0, 1, 2, 3))
def test_worst_case(phase):
    toks = worst_case(phase)
    if phase == 2:
        assert all(p % 32 == 31 for p, _, d in toks if d and p % 32 > 27)
    per = by_word(toks)
    assert decode(per) == symbols(toks) == decode(by_range(toks))
    full = [len(w) for w in per[1:-1]]
    assert 16 <= min(full) and max(full) <= CAP_WORD
    assert sum(len(w) for w in per) <= CAP_SEG
