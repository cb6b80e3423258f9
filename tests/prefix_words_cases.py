"""Inputs and calls of the prefix-words pin (tests/test_gpu_prefix_words_pins.py and
tools/gen_prefix_words_pins.py, which records tests/golden/prefix_words_pins.json from this module).

They aim at the token words of a run segment in the 32 KiB level-2 front kernel (DESIGN 4.1,
"Prefix words in closed form"): the literals of [D, fm) -- fm the segment's first match bit at or
above the dictionary's end D -- are worded in closed form, W0 = ceil((fm - D) / 3) words written by
the threads in turn, and the threads word only what follows.  Every input is seeded and one
segment; the calls that need more put up to five of them behind each other, and the carried-state
stream alternates five kinds of segment.

The prefix length fm - D is the period of a periodic input (its first period is literals, the
second starts with a match), or the random head plus the period behind it.  A match bit within two
positions of its parse chunk's end (chunks of 258 from D) is clipped below three bytes and becomes
a literal: periods 256, 257, 514 and 515 put a literal token exactly at fm without a fingerprint
collision, which is why no random search for one is made.
"""
from deflate_pin_cases import flipped, period, rnd
from run_probe_cases import G_PINNED, PIPE_SEGMENTS, bundles, check, inflate_open  # noqa: F401
from tail_pin_cases import batch_streams, digest, inflate  # noqa: F401  (re-exported)

N = 32768
RP = 2048
LEVEL = 2
DICT_LEN = 1024
PREFIXES = (1, 2, 3, 4, 31, 32, 33, 95, 96, 97, 251, 1023, 1024, 1025)
LONG_HEAD = 3000  # random bytes, longer than one round; the run behind them has period 251
AT_FM = (256, 257, 514, 515)  # the token at fm is a literal (see above)
OWN_DICTS = (1, 33, 4096)
CARRIED_NSEG = 2 * G_PINNED + 3
CARRIED_TAIL = 1234


def long_head(n=N):
    """fm = 3251, W0 = 1084: more prefix words than threads (the strided loop)."""
    return rnd(LONG_HEAD, 300) + period(251, n - LONG_HEAD)


def lengths(p):
    """Full and ragged: the last bitmap word partial, the smallest with two whole rounds (the
    test that proves the run needs them), and one below it, which ends without a terminal run and
    keeps the grouping by bitmap word."""
    return (N, N - 1, N - 3, 2 * RP + 3, RP + 3 + p)


def prefix_lengths():
    out = {}
    for p in PREFIXES:
        for n in lengths(p):
            out[f"p{p}_{n}"] = period(p, n, seed=5)
    for n in (N, N - 3, 2 * RP + 3 + LONG_HEAD):
        out[f"rnd{LONG_HEAD}_p251_{n}"] = long_head(n)
    out[f"p{LONG_HEAD}_{N}"] = period(LONG_HEAD, N, seed=5)
    return out


def literal_at_fm():
    out = {f"p{p}_{n}": period(p, n, seed=6) for p in AT_FM for n in (N, N - 3)}
    # behind random bytes: fm = 1000 + 256 lies in the middle of bitmap word 39
    out["rnd1000_p256"] = rnd(1000, 310) + period(256, N - 1000, seed=6)
    return out


def other_paths():
    """Runs that are not terminal (the rounds go on to the end; the words are grouped by bitmap
    word as before), one that a later test proves after skipped rounds, and run-free segments."""
    import dmx
    base = period(251, N)
    return {
        "p251_flip_end2": flipped(base, N - 2),
        "p97_flip_end4": flipped(period(97, N), N - 4),
        "p251_flip20000": flipped(base, 20000),
        "p33_flip5000_9000": flipped(period(33, N, seed=5), 5000, 9000),
        "text": dmx.corpus("text", N),
        "random": dmx.corpus("random", N),
    }


GROUPS = {
    "prefix_lengths": prefix_lengths,
    "literal_at_fm": literal_at_fm,
    "other_paths": other_paths,
}


def zdict():
    return rnd(DICT_LEN, 320)


def own_dicts():
    """{name: (dictionary, input)}: one segment whose image is the dictionary and the input (D +
    nb = 32768 and ragged).  Behind D random bytes fm - D is the period; an image that is periodic
    across the dictionary's end has fm = D (a prefix of no literal), and with period 1 the match
    bit of the input's first byte."""
    out = {}
    for D in OWN_DICTS:
        zd = rnd(D, 330 + D)
        for p in (1, 2, 3, 4, 32, 33, 97, 251, 256, 257, 1025):
            for n in (N - D, N - D - 3):
                out[f"dict{D}_p{p}_{n}"] = (zd, period(p, n, seed=7))
        out[f"dict{D}_rnd{LONG_HEAD}_p251"] = (zd, long_head(N - D))
        for p in (1, 251):
            image = period(p, N, seed=8)
            out[f"dict{D}_across_p{p}"] = (image[:D], image[D:])
    return out


def carried_kinds(nseg=CARRIED_NSEG, G=G_PINNED):
    """Segment i's kind: 0 a run with 1023 prefix literals, 1 text, 2 a run behind a long random
    head (W0 > 1024), 3 random, 4 a run of period 2 (W0 = 1).  Workgroup i mod G takes segment i as
    its (i // G)-th, so with G workgroups both neighbouring segments and the segments of one
    workgroup differ."""
    return [(i + 2 * (i // G)) % 5 for i in range(nseg)]


def carried_input():
    import dmx
    kinds = carried_kinds()
    text = dmx.corpus("text", CARRIED_NSEG * N)
    noise = dmx.corpus("random", CARRIED_NSEG * N)
    a, c, e = period(1023, N, seed=5), long_head(), period(2, N, seed=5)
    segs = [(a, text[i * N:i * N + N], c, noise[i * N:i * N + N], e)[k] for i, k in enumerate(kinds)]
    return b"".join(segs) + period(97, CARRIED_TAIL)


def carried_buffers():
    """The carried-state segments as batch buffers, every third five bytes short (never staged)."""
    data = carried_input()
    return [data[i * N:i * N + (N - 5 if i % 3 == 2 else N)] for i in range(CARRIED_NSEG)]


def streams(ctx32, ctx64, ctx_pipe):
    """{route: {name: (stream, input, dictionary or None, final)}} of every pinned call.  ctx_pipe
    is a 32 KiB context created with DMX_DEFLATE_PIPE=s2."""
    out = {}
    zd = zdict()
    for g, make in GROUPS.items():
        made = make()
        names = list(made)
        bufs = [made[n] for n in names]
        out[f"{g}/plain"] = {n: (ctx32.compress(b, LEVEL), b, None, True) for n, b in made.items()}
        out[f"{g}/batch"] = {n: (s, b, None, True) for n, s, b in zip(names, batch_streams(ctx32, bufs), bufs)}
        out[f"{g}/batch_dict"] = {n: (s, b, zd, True) for n, s, b in zip(names, batch_streams(ctx32, bufs, zd), bufs)}
        out[f"{g}/not_final"] = {n: (ctx32.compress_raw_not_final(b, LEVEL), b, None, False) for n, b in made.items()}
        for route, ctx, k in (("pipe", ctx_pipe, PIPE_SEGMENTS), ("halves", ctx64, 2)):
            r = out[f"{g}/{route}"] = {}
            for name, parts in bundles(made, k).items():
                data = b"".join(made[p] for p in parts)
                r[name] = (ctx.compress(data, LEVEL), data, None, True)
    r = out["own_dict/batch_dict"] = {}
    for name, (d, data) in own_dicts().items():
        r[name] = (batch_streams(ctx32, [data], d)[0], data, d, True)
    data = carried_input()
    out["carried/plain"] = {"alternating": (ctx32.compress(data, LEVEL), data, None, True)}
    out["carried/pipe"] = {"alternating": (ctx_pipe.compress(data, LEVEL), data, None, True)}
    bufs = carried_buffers()
    got = batch_streams(ctx32, bufs)
    for s, b in zip(got, bufs):
        assert inflate(s) == b
    # (one digest for the 515 streams: their lengths and bytes in order)
    joined = b"".join(len(s).to_bytes(4, "little") + s for s in got)
    out["carried/batch"] = {"alternating": (joined, b"".join(bufs), None, None)}
    return out
