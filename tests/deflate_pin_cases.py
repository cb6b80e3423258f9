"""Inputs of the deflate byte-identity pin (tests/test_gpu_deflate_pins.py and
tools/gen_deflate_pins.py, which records tests/golden/deflate_pins.json).

Every input is seeded and built from dmx.corpus and random.Random only.  The groups aim at the
front kernel's run continuation: runs that reach the segment end (terminal runs), runs that
start late, end just before the segment end or break in the middle, and a long stream whose
persistent workgroups alternate between run segments and run-free ones.
"""
import random

import dmx

SEGS = (16384, 32768, 65536)
LEVELS = (2, 3)
LENGTHS = (32768, 32767, 32765, 4099, 2051)
PERIODS = (1, 3, 4, 251, 502, 2008)
STALE_SEG = 32768
STALE_NSEG = 3 * 256 + 5
STALE_TAIL = 1234


def period(p, n, seed=0):
    """n bytes repeating one seeded random pattern of p bytes."""
    pat = random.Random(1000 * p + seed).randbytes(p)
    return (pat * (n // p + 1))[:n]


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def flipped(data, *positions):
    b = bytearray(data)
    for q in positions:
        b[q] ^= 0xFF
    return bytes(b)


def plain_runs():
    out = {}
    for n in LENGTHS:
        for kind in ("repeat", "zeros", "bmp"):
            out[f"{kind}_{n}"] = dmx.corpus(kind, n)
        for p in PERIODS:
            out[f"p{p}_{n}"] = period(p, n)
    # whole and nearly whole segments of the largest segment size
    for n in (65536, 65533):
        out[f"p251_{n}"] = period(251, n)
        out[f"zeros_{n}"] = bytes(n)
    return out


def late_runs():
    """Random bytes first, so the run is found at round 2 or later."""
    out = {}
    for n in (32768, 32765):
        for p in (1, 4, 251, 2008):
            out[f"rnd4096_p{p}_{n}"] = rnd(4096, p) + period(p, n - 4096)
    out["rnd6144_p251_32768"] = rnd(6144, 7) + period(251, 32768 - 6144)
    out["rnd10000_p3_32767"] = rnd(10000, 8) + period(3, 32767 - 10000)
    # the run is first tested in a last, partial round of 1..13 positions (fewer than the
    # eleven that one vector store of candidates needs, and just more)
    for n in (6145, 6147, 6149, 6154, 6155, 6157):
        out[f"rnd4096_p251_{n}"] = rnd(4096, n) + period(251, n - 4096)
    out["rnd4096_p1_6150"] = rnd(4096, 9) + period(1, 6150 - 4096)
    out["rnd8192_p4_10243"] = rnd(8192, 10) + period(4, 10243 - 8192)
    return out


def short_of_end():
    """The run ends k bytes before the segment end: the last k bytes are flipped."""
    out = {}
    for k in (1, 3, 4, 5):
        for p in (1, 251):
            base = period(p, 32768)
            out[f"p{p}_flip_last{k}"] = flipped(base, *range(32768 - k, 32768))
        out[f"rnd4096_p251_flip_last{k}"] = flipped(rnd(4096, k) + period(251, 32768 - 4096),
                                                    *range(32768 - k, 32768))
    return out


def broken_runs():
    """One flipped byte mid-segment; the run resumes at the same or at another period."""
    out = {}
    for q in (20000, 12345, 10241):
        out[f"p251_flip{q}"] = flipped(period(251, 32768), q)
        out[f"p251_then_p97_at{q}"] = period(251, q) + period(97, 32768 - q, seed=1)
    out["p4_flip20000"] = flipped(period(4, 32768), 20000)
    out["p1_then_p502_at20000"] = period(1, 20000) + period(502, 12768)
    return out


def non_run():
    return {f"{kind}_1MiB": dmx.corpus(kind, 1 << 20) for kind in ("text", "random", "mixed")}


GROUPS = {
    "plain_runs": plain_runs,
    "late_runs": late_runs,
    "short_of_end": short_of_end,
    "broken_runs": broken_runs,
    "non_run": non_run,
}


def stale_lds():
    """3 x 256 + 5 segments of 32 KiB and a 1234-byte tail: segment i is text or random when
    (i // 256 + i) % 2 == 0 and period-251 otherwise, so a persistent workgroup (one per CU,
    256 of them) alternates between segments with a terminal run and segments without."""
    text = dmx.corpus("text", (STALE_NSEG // 2 + 2) * STALE_SEG)
    noise = dmx.corpus("random", (STALE_NSEG // 4 + 2) * STALE_SEG)
    run = period(251, STALE_SEG)
    parts, k = [], 0
    for i in range(STALE_NSEG):
        if (i // 256 + i) % 2:
            parts.append(run)
        else:
            src, j = (noise, k // 4) if k % 4 == 3 else (text, k)
            parts.append(src[j * STALE_SEG:(j + 1) * STALE_SEG])
            k += 1
    parts.append(period(251, STALE_TAIL))
    data = b"".join(parts)
    assert len(data) == STALE_NSEG * STALE_SEG + STALE_TAIL
    return data
