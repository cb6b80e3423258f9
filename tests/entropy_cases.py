"""Inputs of the deflate entropy-stage tests (tests/test_gpu_deflate_entropy.py on the GPU,
tests/test_huff_fit.py for the reach conditions on the model alone).  TEST INFRASTRUCTURE.

Level 1 is Huffman-only, so a segment's lit/len histogram is its byte histogram plus one
end-of-block: every level-1 input here is a seeded shuffle of an exact multiset of bytes, whose
histogram is known without the GPU.  Everything is seeded and built from numpy / random only."""
import random

import numpy as np

SEGS = (16384, 32768, 65536)


# ---- level-1 families: name -> 256 weights (0: the value does not occur) -----------------------
def _uniform(m):
    return [1.0] * m + [0.0] * (256 - m)


def _near_uniform(m):
    """m values at two weights a factor 4 apart, both a little above a half-power of two
    (shares 2^-6.45 and 2^-8.45), so that every initial length rounds down and the code starts
    well over-full: the repair moves dozens of symbols from 8 to 9 bits and more from 6 to 7.
    (An exactly uniform alphabet does not get there: the model counts 5 moves at 130 values and
    at most 1 at 200 or 255, whose initial lengths of 8 bits leave slack instead.)"""
    hi, lo = 2.0 ** -6.45, 2.0 ** -8.45
    a = round((1.0 - m * lo) / (hi - lo))
    return [hi] * a + [lo] * (m - a) + [0.0] * (256 - m)


def _geometric(q):
    return [q ** i for i in range(256)]


def _fibonacci(n):
    w, a, b = [], 1, 1
    for _ in range(n):
        w.append(float(a))
        a, b = b, a + b
    return w + [0.0] * (256 - n)


def _dominant(share):
    return [share * 255.0 / (1.0 - share)] + [1.0] * 255  # value 0 takes `share`; the floor of 1 does the rest


def _used(values, weight=None):
    w = [0.0] * 256
    for i, v in enumerate(values):
        w[v] = weight(i) if weight else 1.0
    return w


# zero runs of the lit/len code-length sequence between used byte values (the end-of-block symbol
# 256 is always used): {0, 1} leaves 2..255, a run of 254 that ends at symbol 255
ZERO_RUNS = {
    "zero runs 1 2 3 10 11": ([0, 2, 5, 9, 20, 32], (1, 2, 3, 10, 11)),
    "zero run 138": ([0, 139], (138,)),
    "zero run 139": ([0, 140], (139,)),
    "zero run 140": ([0, 141], (140,)),
    "zero run 141": ([0, 142], (141,)),
    "zero run 148": ([0, 149], (148,)),
    "zero run 149": ([0, 150], (149,)),
    "zero run 254": ([0, 1], (254,)),
}
# runs of equal non-zero lengths: blocks of (size, length) -- consecutive used values of weight
# 2^-length, one unused value between two blocks.  With the end-of-block symbol (9 bits) each
# member's initial lengths are a complete code already, so the fit leaves every block whole.
EQUAL_RUNS = {
    "equal runs 2 3 4 6 7": ([(2, 2), (3, 4), (4, 5), (6, 6), (7, 7), (2, 6), (3, 9)], (2, 3, 4, 6, 7)),
    "equal runs 8 9 10 13": ([(8, 4), (9, 6), (10, 6), (13, 7), (3, 5), (3, 9)], (8, 9, 10, 13)),
}


def _blocks(blocks):
    assert sum(k << (9 - L) for k, L in blocks) == 511
    w, v = [0.0] * 256, 0
    for k, L in blocks:
        for _ in range(k):
            w[v] = 2.0 ** -L
            v += 1
        v += 1
    return w


def families():
    f = {}
    for m in (1, 2, 3, 5, 17, 64, 128, 130, 200, 255, 256):
        f[f"uniform {m}"] = _uniform(m)
    for m in (130, 200, 255):
        f[f"near-uniform {m}"] = _near_uniform(m)
    for q in (0.5, 0.7, 0.9, 0.97, 0.99):
        f[f"geometric {q}"] = _geometric(q)
    f["fibonacci 22"] = _fibonacci(22)
    f["one value at 90 %"] = _dominant(0.90)
    f["one value at 99 %"] = _dominant(0.99)
    f["16 frequent + 240 rare"] = [400.0] * 16 + [1.0] * 240
    f["zipf"] = [1.0 / (i + 1) for i in range(256)]
    for name, (vals, _) in ZERO_RUNS.items():
        f[name] = _used(vals)
    for name, (blocks, _) in EQUAL_RUNS.items():
        f[name] = _blocks(blocks)
    return f


FAMILIES = families()


def counts(weights, n):
    """Exactly n bytes shared out by the weights: every used value at least once, the rounding's
    rest to (or from) the most frequent value."""
    tot = sum(weights)
    c = [max(1, int(w / tot * n)) if w > 0 else 0 for w in weights]
    order = sorted(range(256), key=lambda i: (-weights[i], i))
    over = sum(c) - n
    if over <= 0:
        c[order[0]] -= over
    for i in order:  # (a short tail: the frequent values give way first, down to one each,
        take = min(over, c[i] - 1) if over > 0 else 0
        c[i] -= take
        over -= take
    for i in reversed(order):  # then the rarest values drop out)
        if over > 0 and c[i]:
            c[i] -= 1
            over -= 1
    assert sum(c) == n and min(c) >= 0
    return c


def shuffled(cnt, seed):
    a = np.repeat(np.arange(256, dtype=np.uint8), cnt)
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def level1_streams(seg):
    """[(names, sizes, data)]: streams of three full segments and a tail of 1..5000 bytes, each
    segment from another family member."""
    names = list(FAMILIES)
    rng = random.Random(seg)
    out = []
    for i in range(0, len(names), 3):  # (every member fills a whole segment once; the tail is the next one)
        grp = (names[i:i + 4] + names[:4])[:4]
        sizes = [seg, seg, seg, rng.randint(1, 5000)]
        parts = [shuffled(counts(FAMILIES[nm], n), 7919 * seg + 31 * i + k) for k, (nm, n) in enumerate(zip(grp, sizes))]
        out.append((grp, sizes, b"".join(parts)))
    return out


# ---- the small-buffer sweep ---------------------------------------------------------------------
SWEEP_ALPHABETS = ("two values", "16 values geometric", "text")


def sweep_buffers(text):
    """1800 buffers: lengths 1..600 of three alphabets (text: bytes of the text corpus).  The 16
    values lie above 143, where the fixed code takes 9 bits: only there can the stored form win
    (5 + n bytes against n + 2 under the fixed code's 8 bits), so this is the alphabet that walks
    stored -> fixed -> dynamic; two values and text walk fixed -> dynamic."""
    rng = np.random.default_rng(600)
    p16 = np.array([0.9 ** i for i in range(16)])
    p16 /= p16.sum()
    out = []
    for n in range(1, 601):
        out.append(("two values", rng.choice(np.array([0x41, 0x7A], dtype=np.uint8), n).tobytes()))
    for n in range(1, 601):
        out.append(("16 values geometric", rng.choice(np.arange(0xC0, 0xD0, dtype=np.uint8), n, p=p16).tobytes()))
    for n in range(1, 601):
        out.append(("text", bytes(text[n:2 * n])))
    return out


# ---- levels 2 and 3: the distance alphabet --------------------------------------------------------
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577, 32769]


def _fresh(n, seed):
    """n random bytes in which no four consecutive bytes occur twice."""
    for k in range(64):
        a = np.random.default_rng(1000 * seed + k).integers(0, 256, n, dtype=np.uint8)
        w = a[:-3].astype(np.uint32) | a[1:-2].astype(np.uint32) << 8 | a[2:-1].astype(np.uint32) << 16 | a[3:].astype(np.uint32) << 24
        if len(np.unique(w)) == len(w):
            return a.tobytes()
    raise AssertionError("no seed without a repeated four bytes")


def copies(symbols, n=32768, seed=1):
    """16 fresh random bytes alternating with 16 bytes copied from a distance whose symbol is
    drawn from `symbols` ({symbol: weight}); every symbol is used at least once where the
    position allows it.  A source starts inside fresh bytes no copy has read before, so the
    copy's first four bytes occur once before it: at the chosen distance.  (Distances of 17..32,
    symbols 8 and 9, would start in copied bytes and are left out.)"""
    rng = random.Random(seed)
    fresh = _fresh(n, seed)
    data = bytearray(fresh)
    slots = list(range(n // 32))  # copy k fills [32 k + 16, 32 k + 32)
    total = sum(symbols.values())
    want = []
    for s, w in sorted(symbols.items(), reverse=True):
        want += [s] * max(1, round(w / total * len(slots) * 0.9))
    rng.shuffle(slots)
    taken, plan = set(), {}
    for s in want:  # far symbols first: they fit the fewest slots
        lo, hi = DIST_BASE[s], DIST_BASE[s + 1] - 1
        for k in slots:
            if k in plan:
                continue
            p = 32 * k + 16
            if p - lo < 0:
                continue
            d = rng.randint(lo, min(hi, p))
            j, off = divmod(p - d, 32)
            if d > 16 and (off > 12 or j in taken):
                continue
            taken.add(j)
            plan[k] = d
            break
    for k in sorted(plan):
        p, d = 32 * k + 16, plan[k]
        for i in range(16):
            data[p + i] = data[p + i - d]
    return bytes(data)


def single_copy_period(n, period, seed):
    """Fresh bytes, each stretch of `period` followed by its own copy: every match lies at
    distance `period`, and nothing else repeats."""
    fresh = _fresh(n, seed)
    out = bytearray()
    i = 0
    while len(out) < n:
        out += fresh[i:i + period] * 2
        i += period
    return bytes(out[:n])


def level23_inputs(text, mixed):
    """name -> one 32 KiB segment."""
    geo = {s: 0.7 ** s for s in range(30)}
    return {
        "zeros": bytes(32768),
        "period 1": b"\x55" * 32768,
        "period 251": single_copy_period(32768, 251, 2),
        # (a copy at distance 30000 leaves 2768 bytes to match, of which the match finder's hash
        # table keeps too few candidates for the block to beat the stored form at level 3)
        "period 25000": (lambda f: f + f[:7768])(_fresh(25000, 3)),
        "30 distance symbols": copies(geo, seed=4),
        "2 distance symbols": copies({10: 1.0, 22: 1.0}, seed=5),
        "text": bytes(text[:32768]),
        "mixed": bytes(mixed[:32768]),
    }
