"""Inputs of the parse byte-identity pin (tests/test_gpu_parse_pins.py and
tools/gen_deflate_pins.py, which records tests/golden/parse_pins.json from this module).

They aim at the level-2 parse of the 32 KiB front kernel where it takes match lengths from a
proven terminal run instead of comparing bytes (the run extended one round backwards to run_e;
DESIGN 4.1, "1d. Run-aware parse") and at the literal skip that looks several bitmap words
ahead.  That skip exists only in the walk of segments with a terminal run, so the inputs that aim
at it (literal_skip_run) are random bytes with a period-251 run behind them up to the segment
end; the run-free ones (literal_skip) cover the plain walk those segments keep.  Every input
is seeded, at most 64 KiB, and built from random.Random (deflate_pin_cases' helpers).

Positions are derived from the kernel's geometry: match rounds of 2048 positions (a run is
proven by the round after the first round whose last positions all have a candidate), parse
chunks of 258 bytes, and the round-0 candidate of a position p of period-P data, its first
occurrence in the round: c = p - (p mod P).
"""
from deflate_pin_cases import flipped, period, rnd

SEGS = (16384, 32768, 65536)
LEVELS = (2, 3)
N = 32768
ROUND = 2048
CHUNK = 258
# the distance the run test settles on for a period: the trigger's candidate is
# c = 2047 - (2047 mod P); the test takes c / k for the largest k <= 16 dividing c whose
# quotient is still a period of the data
RUN_D = {251: 251, 502: 502, 97: 291}


def back_ext():
    """One flipped byte in the round before the run: the backward extension ends inside it."""
    out = {}
    spots = (300, 1000, ROUND - 1 - 251, ROUND - 4, ROUND - 3, ROUND - 2, ROUND - 1)
    for q in spots:
        out[f"p251_flip{q}"] = flipped(period(251, N), q)
    for q in spots:  # the run is proven at 6144: the same flips two rounds later
        out[f"rnd4096_p251_flip{4096 + q}"] = flipped(rnd(4096, 11) + period(251, N - 4096), 4096 + q)
    return out


def src_edge():
    """A flip at f < P puts the run's proven start at run_e = f + run_d + 1 (the last mismatch is
    f + run_d against f).  A chunk start p = 258 j with round-0 candidate c = p - s, s = p mod P,
    has its source at s: f = s - 2, s - 1, s puts run_e - run_d one before, at and one after s."""
    out = {}
    for P, d in RUN_D.items():
        js = [j for j in range(1, ROUND // CHUNK + 1)
              if P + d + 2 <= CHUNK * j < ROUND and (CHUNK * j) % P >= 2]
        for j in (js[0], js[-1]):
            s = (CHUNK * j) % P
            for f in (s - 2, s - 1, s):
                out[f"p{P}_chunk{j}_flip{f}"] = flipped(period(P, N), f)
    return out


def other_periods():
    """Candidates inside the verified region that are no multiples of the run distance."""
    out = {}
    for a in (1500, 3000):
        out[f"p97x{a}_p251"] = period(97, a) + period(251, N - a)
    for a in (1300, 5000):
        out[f"p251x{a}_p502"] = period(251, a) + period(502, N - a, seed=1)
    for P in (6, 12):
        for n in (N, N - 3):
            out[f"p{P}_{n}"] = period(P, n)
    return out


def small_divisors():
    return {f"p{P}_{n}": period(P, n) for P in (2, 8, 16, 502, 1004, 2008) for n in (N, N - 3)}


def last_chunk():
    """A last parse chunk of 1..5 bytes inside a run."""
    return {f"p251_{CHUNK * k + r}": period(251, CHUNK * k + r) for k in (20, 126) for r in (1, 2, 3, 4, 5)}


def with_repeat(data, *starts):
    """The 12 bytes that end 28 before each start, copied to it (a match at distance 40)."""
    b = bytearray(data)
    for x in starts:
        b[x:x + 12] = b[x - 40:x - 28]
    return bytes(b)


def literal_skip():
    """Run-free inputs: the plain walk (no look-ahead), at every level and segment size."""
    out = {}
    n = CHUNK * 24
    for j in (5, 8):  # chunk starts 1290 (bit 10 of its bitmap word) and 2064 (bit 16)
        for off in (0, 1, 31, 32, 33, 159, 160, 257):
            out[f"rnd_rep_chunk{j}_off{off}"] = with_repeat(rnd(n, 20 + j), CHUNK * j + off)
    out["rnd_rep_last_word"] = with_repeat(rnd(n, 31), n - 14)
    # chunk 4 ends with literals in the bitmap word [1280, 1312) that chunk 5's repeat shares
    out["rnd_rep_shared_word"] = with_repeat(rnd(n, 32), 1270, 1296)
    for k in (1, 8, 24, 127):
        out[f"rnd_{CHUNK * k}"] = rnd(CHUNK * k, 40 + k)
    for m in (1, 31, 32, 33, 258, 259):
        out[f"lit_{m}"] = rnd(m, 60 + m)
    return out


def literal_skip_run():
    """The quad-wide look-ahead of the 32 KiB level-2 walk: 24 chunks of random bytes, then
    period 251 to the segment end.  The run is proven at 8192 (the round after the first whose
    last positions all have a candidate), so the whole segment, its random chunks included, takes
    the walk with the look-ahead.  A 12-byte repeat in the random part puts the first match bit
    at chosen places: chunk offsets around the chunk start, the bitmap word edges (chunk 5 starts
    at bit 10 of its word: offsets 21..23; chunk 8 at bit 16: offsets 15..17), one to five words
    ahead, the chunk's last word (where the clip at the chunk end acts: chunk 5 ends at 1548,
    bit 12 of the word at 1536) and its last position; two repeats in neighbouring chunks whose
    token bits share one bitmap word; and random chunks alone, every one of which walks to its
    end through a clipped word and ORs into the boundary words it shares with its neighbours."""
    out = {}
    n0 = CHUNK * 24

    def run_after(prefix):
        return prefix + period(251, N - len(prefix))

    edges = {5: (21, 22, 23), 8: (15, 16, 17)}
    for j in (5, 8):
        for off in (0, 1) + edges[j] + (31, 32, 33, 64, 96, 128, 159, 160, 257):
            out[f"rnd_rep_chunk{j}_off{off}_run"] = run_after(with_repeat(rnd(n0, 20 + j), CHUNK * j + off))
    for x in (1535, 1536, 1537, 1540, 1545):  # around and inside chunk 5's last word [1536, 1548)
        out[f"rnd_rep_at{x}_run"] = run_after(with_repeat(rnd(n0, 33), x))
    out["rnd_rep_shared_word_run"] = run_after(with_repeat(rnd(n0, 32), 1270, 1296))
    out["rnd_rep_last_random_word_run"] = run_after(with_repeat(rnd(n0, 31), n0 - 14))
    for m in (CHUNK, CHUNK * 8, n0, 6000, 4096 + 33):
        out[f"rnd_{m}_run"] = run_after(rnd(m, 70 + m % 97))
    return out


GROUPS = {
    "back_ext": back_ext,
    "src_edge": src_edge,
    "other_periods": other_periods,
    "small_divisors": small_divisors,
    "last_chunk": last_chunk,
    "literal_skip": literal_skip,
    "literal_skip_run": literal_skip_run,
}
