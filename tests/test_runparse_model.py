"""CPU model of the run-aware parse of the 32 KiB level-2 front kernel.

The kernel's two statements are written here once, as deflate_kernels.hip states them:

* run_e (the backward extension): the words of [run_lo - 2048, run_lo), not below run_d, are
  compared with the words run_d before them; run_e is the end of the last mismatching byte,
  and without a mismatch the first word compared, max(run_lo - 2048, run_d rounded up to 4).
* known_len(q, d): q >= run_e, d a multiple of run_d (a float32-reciprocal quotient verified by
  one multiply) and q - d + run_d >= run_e.  Then the parse takes min(258, hi - q) as the match
  length without reading a byte.

Both are checked against brute force on seeded periodic inputs with one or two flipped bytes
near run_e, run_lo and the parse-chunk edges: [run_e, nb) really repeats at run_d, and wherever
known_len holds the byte-by-byte match length is maxl.
"""
import random

import numpy as np

RP = 2048     # positions per match round
CHUNK = 258   # bytes per parse chunk
SEG = 32768


def run_e_of(data, run_lo, run_d):
    e = max(run_lo - RP, (run_d + 3) & ~3)
    for bq in range(run_lo - RP, run_lo, 4):
        if bq >= run_d:
            for b in range(4):
                if data[bq + b] != data[bq + b - run_d]:
                    e = max(e, bq + b + 1)
    return e


def known_len(q, d, run_e, run_d, ulp=0):
    """ulp: the reciprocal moved that many float32 steps (the kernel's v_rcp_f32 is accurate to
    one, not exactly rounded)."""
    rcp = np.float32(1.0) / np.float32(run_d)
    for _ in range(abs(ulp)):
        rcp = np.nextafter(rcp, np.float32(np.inf if ulp > 0 else 0.0), dtype=np.float32)
    m = int(np.float32(d) * rcp + np.float32(0.5))
    return q >= run_e and m * run_d == d and q - d + run_d >= run_e


def matchlen(data, p, q, maxl):
    n = 0
    while n < maxl and data[p + n] == data[q + n]:
        n += 1
    return n


def build_cases():
    """(data, nb, run_lo, run_d): run_lo a round start, data[q] == data[q - run_d] on [run_lo, nb)
    (what the kernel's forward test has proven when it calls the run terminal)."""
    rng = random.Random(20260)
    cases = []
    for P in (1, 2, 3, 4, 6, 12, 97, 251, 502, 1004, 2008):
        for pre in (0, 2048, 4096):
            for trial in range(6):
                nb = rng.choice((SEG, SEG - 3, 258 * 40 + rng.randrange(1, 6), pre + 2 * RP + rng.randrange(1, 600)))
                pat = rng.randbytes(P)
                data = bytearray(rng.randbytes(pre) + (pat * (nb // P + 2))[:nb - pre])
                run_lo = pre + RP
                run_d = P * rng.choice([k for k in (1, 1, 2, 3, 8) if P * k <= run_lo])
                # one or two flips before run_lo - run_d (so the forward test still passes): near the
                # floor of the backward compare, near run_lo and near chunk edges
                spots = [pre + rng.randrange(0, 8), pre + P + rng.randrange(0, 8), run_lo - run_d - 1 - rng.randrange(0, 6),
                         CHUNK * rng.randrange(1, 8) + pre // CHUNK * CHUNK + rng.randrange(-2, 3),
                         rng.randrange(pre, run_lo)]
                for f in rng.sample(spots, rng.choice((0, 1, 1, 2))):
                    if pre <= f < run_lo - run_d:
                        data[f] ^= 0xFF
                data = bytes(data)
                if all(data[q] == data[q - run_d] for q in range(run_lo, nb)):
                    cases.append((data, nb, run_lo, run_d))
    return cases


def test_known_lengths_match_brute_force():
    rng = random.Random(7)
    holds = fails = 0
    cases = build_cases()
    assert len(cases) >= 100
    for data, nb, run_lo, run_d in cases:
        run_e = run_e_of(data, run_lo, run_d)
        assert run_e <= run_lo
        assert all(data[q] == data[q - run_d] for q in range(run_e, nb)), (nb, run_lo, run_d, run_e)
        starts = {run_e - 1, run_e, run_e + 1, run_lo - 1, run_lo, nb - 1, nb - 4}
        starts |= {CHUNK * j + k for j in range(0, 12) for k in (0, 1, 257)}
        starts |= {rng.randrange(1, nb) for _ in range(12)}
        for q in sorted(x for x in starts if 1 <= x < nb):
            hi = min(q // CHUNK * CHUNK + CHUNK, nb)
            maxl = min(258, hi - q)
            ds = {run_d, 2 * run_d, 3 * run_d, 8 * run_d, q - run_e + run_d, q - run_e + run_d + 1,
                  (q - run_e) // run_d * run_d, (q - run_e) // run_d * run_d + run_d, 1, 2, 3, 4,
                  run_d + 1, run_d - 1, q // run_d * run_d, q}
            for d in sorted(x for x in ds if 1 <= x <= q):
                if known_len(q, d, run_e, run_d):
                    holds += 1
                    assert matchlen(data, q, q - d, maxl) == maxl, (nb, run_lo, run_d, run_e, q, d)
                else:
                    fails += 1
    assert holds >= 100 and fails >= 100, (holds, fails)


def test_multiple_test_is_exact():
    """The float32 quotient, rounded and verified by one multiply, is an exact divisibility test
    for every distance and run distance of a 32 KiB segment's scale, also with a reciprocal
    that is one float32 step off either way."""
    rng = random.Random(3)
    for _ in range(4000):
        run_d = rng.randrange(1, 32768)
        for d in (run_d * rng.randrange(1, 32768 // run_d + 1), rng.randrange(1, 32768)):
            for ulp in (0, 1, -1):
                assert known_len(40000, d, 0, run_d, ulp) == (d % run_d == 0), (d, run_d, ulp)
