"""The lane decoder (k_inflate_lanes) on runs of equal matches and on table shapes.

A long run reaches an inflater as equal matches (L, d) back to back, because LEN stops at 258.
While a lane of a wave is inside such a run, the lane decoder's token steps fold up to four equal
matches into one ("Lane pass, round 17").  The streams here put runs at every place
where the fold has a limit: 1..9 copies, a run that ends exactly at output byte 32768 or one
match past it, a run broken by a literal or by a match that differs in the last bit it sends, a
run right before the end-of-block of a middle segment and of the final one, match codes of 2, 9,
13, 21 and 27 bits, and runs in the stream's first segment whose distance reaches before the
output (the reference copies nothing there; as a piece the stream is refused).  The table cases
give the per-segment table build (a lane pair per segment) every code length, both ends of HLIT,
a fixed block, a one-symbol distance code (declined by the lanes) and a second, partly filled
wave.

Streams have 1..40 segments of at most 32 KiB: one block each, closed by an empty stored block
or BFINAL, the layout the lanes accept.  Expected bytes come from zlib's inflate (from the oracle
for the one stream zlib refuses: a distance before the start of the output).  PATHS holds
stats().path of every stream as the library gave it before the fold and the pair build existed.
"""
import zlib

import pytest

import dmx
import lenient_streams as LS
from golden.quirk_streams import DIST_BASE, LEN_BASE, rle_ops

pytestmark = pytest.mark.gpu

CAP = 32768


def _lens(n, d):
    L = [0] * n
    for s, v in d.items():
        L[s] = v
    return L


# name -> (lit/len lengths, distance lengths); None: the fixed code
CODES = {
    # a match (4, 1) or (4, 4) is 1 + 1 bits
    "two": (_lens(259, {97: 3, 98: 3, 256: 2, 258: 1}), _lens(4, {0: 1, 3: 1})),
    # a match (258, 193..256) is 2 + 1 + 6 bits: the shape of libdmx's `repeat` segments
    "nine": (_lens(286, {97: 3, 98: 3, 99: 3, 100: 3, 256: 2, 285: 2}), _lens(16, {14: 1, 15: 1})),
    "fixed": None,
    # every lit/len length 1..9 and every distance length 1..6
    "all_lengths": (_lens(286, {97: 1, 98: 2, 99: 3, 100: 4, 101: 5, 256: 6, 285: 7, 0: 8, 264: 9, 270: 9}),
                    _lens(30, {0: 1, 15: 2, 3: 3, 29: 4, 10: 5, 1: 6, 20: 6})),
    "hlit257": (_lens(257, {97: 1, 98: 2, 0: 3, 255: 4, 256: 4}), _lens(2, {0: 1, 1: 1})),
    "one_dist": (_lens(286, {97: 2, 98: 2, 256: 2, 285: 2}), _lens(1, {0: 1})),
}


def block(code, toks, final=False):
    """One block: toks are ints (literals) and (L, d) pairs; then the end of block.  Not final: an
    empty stored block follows, so the next block starts a segment."""
    W = LS.Writer(LS.Rng(0), LS.Case())
    W.bw.put(1 if final else 0, 1)
    if CODES[code] is None:
        W.bw.put(1, 2)
        lit, dist = LS.FIXED_LIT, LS.FIXED_DIST
    else:
        LL, DL = CODES[code]
        W.bw.put(2, 2)
        ops = rle_ops(LL) + rle_ops(DL)
        W.header(len(LL), len(DL), ops, LS.default_precode(ops))
        lit, dist = LS.Lookup(LL), LS.Lookup(DL)
    for t in toks:
        if isinstance(t, int):
            W.literal(lit, t)
            continue
        L, d = t
        ls = 28 if L == 258 else max(i for i in range(28) if LEN_BASE[i] <= L)
        ds = max(i for i in range(30) if DIST_BASE[i] <= d)
        W.match(lit, dist, 257 + ls, L - LEN_BASE[ls], ds, d - DIST_BASE[ds])
    W.code(lit, 256)
    if final:
        W.bw.align()
    else:
        W.bw.empty_stored()
    return W.bw.bytes()


def stream(*segs):
    """Segments (code, toks); the last one carries BFINAL."""
    return b"".join(block(c, t, final=i == len(segs) - 1) for i, (c, t) in enumerate(segs))


A, B = 97, 98
LEAD = [A, B, 99, 100] * 128  # 512 bytes, 256 steps of literal pairs
RUN9 = (258, 251)             # 9 bits under "nine"
FILL = ("nine", LEAD + [RUN9] * 3 + [A])
# The steps of a wave fold only while one of its lanes is inside a long run (a pending match
# longer than two whole matches, looked at every six steps).  This segment keeps its wave there
# from about step 140 to step 2000: one literal and 8000 matches (4, 1) of 2 bits, four to a
# step.  The runs of the other segments stand behind 150 or more steps of literals.
DRIVER = ("two", [A] + [(4, 1)] * 8000)


def _cases():
    c = {}
    for n in range(1, 10):
        # the run alone in a middle segment and in the BFINAL segment: its last copy stands right
        # before the end-of-block, and the window behind holds the marker or the stream's end
        seg = ("nine", LEAD + [RUN9] * n)
        c["run%d" % n] = stream(DRIVER, seg, FILL, seg)
    # ... and with the same bits going on behind it: the run is cut by a literal whose code starts
    # like the match's, and by a match that differs only in the last bit it sends (the top bit of
    # the distance's extra bits: 251 = 193 + 0b111010, 219 = 193 + 0b011010)
    c["run_cut_literal"] = stream(FILL, ("nine", LEAD + [RUN9] * 5 + [A] + [RUN9] * 6 + [B, B]), DRIVER)
    c["run_cut_last_bit"] = stream(("nine", LEAD + [RUN9] * 5 + [(258, 219)] + [RUN9] * 7 + [(258, 219)] * 2), DRIVER,
                                   FILL)
    # a run that ends exactly at byte 32768: 259 + j * 258 + 1 + (126 - j) * 258, the copies left
    # for the last step differing with j; and one match more (beyond the lanes: declined)
    for j in range(4):
        c["to_cap_%d" % j] = stream(FILL, ("fixed", [0] * 259 + [(258, 1)] * j + [0] + [(258, 1)] * (126 - j)), FILL)
    c["past_cap"] = stream(FILL, ("fixed", [0] * 260 + [(258, 1)] * 127), FILL)
    c["to_cap_nine"] = stream(("nine", [A] * 260 + [RUN9] * 126), FILL)
    c["to_cap_driven"] = stream(DRIVER, ("nine", LEAD + [RUN9] * 125 + [A, B, 99, 100, A, B]), FILL)
    # match codes of 2 bits (crafted), 13 (fixed-code zeros), 21 (two fit a step) and 27 (none)
    c["bits2"] = stream(DRIVER, ("two", [A, B] * 150 + [(4, 4)] * 23 + [B] + [(4, 1)] * 9), ("two", [A] + [(4, 1)] * 40))
    c["bits13"] = stream(DRIVER, ("fixed", [0] * 300 + [(258, 1)] * 11 + [7] + [(258, 2)] * 6))
    c["bits21"] = stream(("fixed", list(range(256)) + list(range(64)) + [(120, 40)] * 9 + [3] + [(120, 56)] * 4),
                         DRIVER, FILL)
    c["bits27"] = stream(DRIVER, ("fixed", list(range(256)) * 5 + [(140, 1100)] * 7))
    # table shapes: all code lengths, HLIT 257 (no length symbol) and 286, a fixed block, a
    # one-symbol distance code (the lanes decline it), random complete codes
    full = ("all_lengths", LEAD + [(258, 251)] * 6 + [0, 101, (10, 1), (25, 4), (24, 2), (10, 1200), (23, 40)])
    c["tables"] = stream(full, ("hlit257", [A, B, 0, 255] * 9), ("fixed", [5] * 40 + [(258, 40)] * 5), full,
                         ("hlit257", [255]), ("nine", LEAD), DRIVER)
    c["one_dist"] = stream(FILL, ("one_dist", [A, B] + [(258, 1)] * 6), FILL)
    lanes = [LS.lane_case(i) for i in range(80)]
    parts = [k.stream for k in lanes if k.far_by == 0]
    c["segments33"] = b"".join(parts[:32]) + stream(full)
    c["segments40"] = b"".join(parts[32:52]) + stream(*[FILL, full] * 10)
    return c


CASES = _cases()
# runs whose distance reaches before the output, in the first segment of the stream: nothing is
# copied (zlib refuses such a stream).  The first run stands at the stream start, the second
# (20 bits a match, so two would fold) behind 150 steps, the third is accepted.
BEFORE_START = stream(("fixed", [0, 1] + [(258, 400)] * 3 + list(range(149)) * 2 + [(258, 400)] * 6 + list(range(200))
                       + [(258, 400)] * 5), DRIVER, FILL)

# stats().path per stream, recorded from the library before the fold
PATHS = {name: 4 for name in CASES}
PATHS["one_dist"] = 1  # (the lanes decline the segment; the wave-per-segment decoder's result stands)
PATHS["past_cap"] = 5  # (a segment beyond 32 KiB: not this layout)
PATH_BEFORE_START = 4
PATH_C4 = 4


@pytest.fixture(scope="module")
def ctx():
    """A context whose plan sends every candidate to the lanes: in a stream of few segments the
    default plan gives those of more than 256 compressed bytes to the workgroup decoder."""
    c = dmx.Context(heavy_bytes=1 << 20)
    yield c
    c.close()


def _inflate(c, s, fn="inflate_device"):
    import torch
    d_in = torch.frombuffer(bytearray(s) + bytearray(16), dtype=torch.uint8).cuda()
    d_o = torch.zeros(41 * CAP, dtype=torch.uint8, device="cuda")
    n = getattr(c, fn)(d_in.data_ptr(), len(s), d_o.data_ptr(), d_o.numel())
    torch.cuda.synchronize()
    return d_o[:n].cpu().numpy().tobytes()


def test_streams_are_in_shape():
    for name, s in CASES.items():
        assert 1 <= s.count(b"\x00\x00\xff\xff") + 1 <= 41, name
        assert len(zlib.decompressobj(-15).decompress(s)) <= 40 * CAP


@pytest.mark.parametrize("name", sorted(CASES))
def test_runs_and_tables(ctx, name):
    s = CASES[name]
    want = zlib.decompressobj(-15).decompress(s)
    got = _inflate(ctx, s)
    path = ctx.stats().path
    print("path %-18s %d" % (name, path))
    assert got == want
    assert path == PATHS[name]


def test_run_before_the_stream_start(ctx, oracle):
    want = oracle.inflate(BEFORE_START)
    assert len(want) == 2 + 298 + 200 + 5 * 258 + 32001 + 512 + 3 * 258 + 1
    assert _inflate(ctx, BEFORE_START) == want
    assert ctx.stats().path == PATH_BEFORE_START
    # as a piece of a larger stream the same reference is an error, not a copy of nothing
    with pytest.raises(dmx.DmxError) as e:
        _inflate(ctx, BEFORE_START, "inflate_piece_device")
    assert e.value.code == dmx.DMX_ERR_DATA


def test_runs_async(ctx):
    import torch
    # (the asynchronous call compacts nothing: every segment but the last fills its 32 KiB)
    whole = ("nine", [A] * 260 + [RUN9] * 126)
    s = stream(whole, ("two", DRIVER[1] + [A] * 767), whole, ("nine", LEAD + [RUN9] * 7))
    want = zlib.decompressobj(-15).decompress(s)
    assert len(want) == 3 * CAP + 512 + 7 * 258
    d_in = torch.frombuffer(bytearray(s) + bytearray(16), dtype=torch.uint8).cuda()
    d_o = torch.zeros(4 * CAP, dtype=torch.uint8, device="cuda")
    d_r = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    ctx.inflate_device_async(d_in.data_ptr(), len(s), d_o.data_ptr(), d_o.numel(), d_r.data_ptr())
    torch.cuda.synchronize()
    assert [int(x) for x in d_r.tolist()] == [len(want), 0]
    assert d_o[:len(want)].cpu().numpy().tobytes() == want


def test_run_across_the_half_of_a_64k_segment():
    """64 KiB segments (the SPLIT instantiation, which does not fold): libdmx's own deflate of
    periodic data, each block one run across its byte 32768."""
    data = (bytes(range(251)) * 1100)[:4 * 65536 + 777]
    c = dmx.Context(segment_bytes=65536, heavy_bytes=1 << 20)
    try:
        s = c.compress(data, 2)
        assert zlib.decompressobj(-15).decompress(s) == data
        assert _inflate(c, s) == data
        assert c.stats().path == PATH_C4
    finally:
        c.close()
