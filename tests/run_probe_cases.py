"""Inputs and calls of the run-probe pin (tests/test_gpu_run_probe_pins.py and
tools/gen_run_probe_pins.py, which records tests/golden/run_probe_pins.json from this module).

They aim at the 32 KiB level-2 front kernel's run test: the round after a
round whose last positions all found a candidate compares the rest of the segment with itself at
one distance, before any table work of its own.  A test that proves the rest (a terminal run)
ends the rounds; one that proves some whole rounds skips them; one that fails waits 1, 2, 4 ..
rounds.  Every input is seeded and at most 32 KiB; the calls that need more put up to five of
them behind each other, and the carried-state stream alternates four kinds of segment.

Geometry: match rounds of 2048 positions, a 4-byte match key (a mismatch at m ends the verified
positions at m - 3), a pretest of the 256 bytes at the round's start at the divisors dl / k of
the trigger's distance, parse chunks of 258 bytes that start at the dictionary's end.
"""
import random
import zlib

from deflate_pin_cases import flipped, period, rnd
from tail_pin_cases import batch_streams, digest, inflate  # noqa: F401  (digest, inflate: re-exported)

N = 32768
RP = 2048
LEVEL = 2
DICT_LEN = 1024
PIPE_SEGMENTS = 5  # DMX_DEFLATE_PIPE=s2: chunks of two, two and one segment
G_PINNED = 256     # the front kernel's grid on the GPU the pins were recorded for
CARRIED_NSEG = 2 * G_PINNED + 3
CARRIED_TAIL = 1234


def run_after(prefix, n=N, p=251):
    return prefix + period(p, n - len(prefix))


def proving_round():
    """The test proves a terminal run: in round 1 (periodic from offset 0) at full and ragged
    lengths, down to the smallest with two full rounds (4099) and the two below it; and in a later
    round, behind 2048 k - 100 random bytes."""
    out = {f"p251_{n}": period(251, n) for n in (32768, 32767, 30000, 4099, 4098, 4097)}
    for k in (1, 2, 7, 14, 15):
        out[f"rnd{RP * k - 100}_p251"] = run_after(rnd(RP * k - 100, 200 + k))
    out["rnd1948_p251_30000"] = run_after(rnd(RP - 100, 201), 30000)
    return out


def not_terminal():
    """Runs that the test does not prove to the end: one differing byte k before the end (the
    m - 3 edge) and mid-segment with the period resuming after it; breaks early enough that the
    back-off of 1, 2 and 4 rounds is followed by a test that proves a terminal run; and a break
    in the first word the test compares."""
    base = period(251, N)
    out = {f"p251_flip_end{k}": flipped(base, N - k) for k in (1, 2, 3, 4, 5)}
    out["p251_flip20000"] = flipped(base, 20000)
    out["p251_backoff1"] = flipped(base, 5000)
    out["p251_backoff2"] = flipped(base, 5000, 9000)
    out["p251_backoff4"] = flipped(base, 5000, 9000, 15000)
    out["p251_flip_first_word"] = flipped(base, RP + 1)
    out["rnd1948_p251_flip20000"] = flipped(run_after(rnd(RP - 100, 210)), 20000)
    return out


def divisor_decoy():
    """Period 1004 whose bytes [40, 296) repeat at [542, 798): the trigger's distance is
    2008 = 2047 - 39, the 256 bytes at 2048 repeat at 2008 / 4 = 502 (the pretest passes for
    k = 4) and nothing else does: the forward compare at 502 fails at 2304."""
    x = bytearray(random.Random(220).randbytes(1004))
    x[542:798] = x[40:296]
    return (bytes(x) * (N // 1004 + 1))[:N]


def distances():
    out = {f"p{p}": period(p, N) for p in (1, 2, 3, 4, 5, 16, 17, 24, 251, 2047, 2048, 2049, 4099)}
    out["p1004_decoy502"] = divisor_decoy()
    return out


PREFIX_BITS = (3, 31, 32, 33, 257, 258, 259, 2047, 2048)


def literal_prefix():
    """The first period of a run segment is literals: the first match bit lies at the period."""
    return {f"first_bit{p}": period(p, N, seed=3) for p in PREFIX_BITS}


GROUPS = {
    "proving_round": proving_round,
    "not_terminal": not_terminal,
    "distances": distances,
    "literal_prefix": literal_prefix,
}


def zdict():
    return rnd(DICT_LEN, 230)


def prefix_dicts():
    """{name: (dictionary, input)}: the literal-prefix inputs behind dictionaries of 1, 257 and
    4096 random bytes (the first match bit at D + period), and one image that is periodic across
    the dictionary's end, whose run starts below D: the first match bit, at D, lies above run_lo."""
    out = {}
    for dlen in (1, 257, 4096):
        zd = rnd(dlen, 240 + dlen)
        for name, data in literal_prefix().items():
            out[f"dict{dlen}_{name}"] = (zd, data)
    image = period(251, 4096 + N)
    out["dict4096_periodic_across"] = (image[:4096], image[4096:])
    return out


def bundles(made, k):
    """{name: [input names]}: lists of k inputs, k - 1 full segments and then any input, in which
    every input of made occurs; a short input can only be the last."""
    fulls = [n for n in made if len(made[n]) == N]
    rest = [n for n in made if len(made[n]) != N]
    nb = max(-(-len(fulls) // (k - 1)), len(rest))
    out = {}
    for i in range(nb):
        heads = [fulls[(i * (k - 1) + j) % len(fulls)] for j in range(k - 1)]
        tail = rest[i] if i < len(rest) else fulls[(i * (k - 1) + k - 1) % len(fulls)]
        out[f"b{i}_{tail}"] = heads + [tail]
    return out


def carried_kinds(nseg=CARRIED_NSEG, G=G_PINNED):
    """Segment i's kind: 0 a run from offset 0, 1 text, 2 a run behind random bytes, 3 random.
    Workgroup i mod G takes segment i as its (i // G)-th, so with G workgroups both neighbouring
    segments and the segments of one workgroup differ."""
    return [(i + i // G) % 4 for i in range(nseg)]


def carried_input():
    import dmx
    kinds = carried_kinds()
    text = dmx.corpus("text", CARRIED_NSEG * N)
    noise = dmx.corpus("random", CARRIED_NSEG * N)
    run = period(251, N)
    late = run_after(rnd(RP * 2 - 100, 250))
    segs = [(run, text[i * N:i * N + N], late, noise[i * N:i * N + N])[k] for i, k in enumerate(kinds)]
    return b"".join(segs) + period(251, CARRIED_TAIL)


def carried_buffers():
    """The carried-state segments as batch buffers, every third five bytes short (never staged)."""
    data = carried_input()
    return [data[i * N:i * N + (N - 5 if i % 3 == 2 else N)] for i in range(CARRIED_NSEG)]


def inflate_open(comp):
    """A stream without a final block (DMX_DEFLATE_NOT_FINAL), closed by an empty fixed block."""
    z = zlib.decompressobj(-15)
    out = z.decompress(comp)
    assert not z.eof
    out += z.decompress(b"\x03\x00") + z.flush()
    assert z.eof and not z.unused_data
    return out


def check(stream, data, zd, final):
    """The stream decodes to its input with zlib (final None: checked where it was made)."""
    if final is not None:
        assert (inflate(stream, zd) if final else inflate_open(stream)) == data


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
    r = out["literal_prefix/own_dict"] = {}
    for name, (d, data) in prefix_dicts().items():
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
