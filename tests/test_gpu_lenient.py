"""Differential test of every inflate route on the seeded lenient / edge-case streams of
tests/lenient_streams.py: over-subscribed and incomplete codes, symbols outside the alphabets,
code-length repeats that overshoot, headers long enough to refill the header reader's window,
odd fixed and stored blocks, and truncations of all of these.

The expected bytes or error of every case come from the oracle at test time (the CPU
restatement of the reference inflate, pinned to the compiled reference on exactly these streams
by test_lenient_streams.py); oracle -1 is DMX_ERR_OVERREAD, -2 DMX_ERR_DATA.  Every route must
give them: a route that cannot honour a lenient rule declines to the serial decoder, whose
result is the same.  The path histograms printed here are recorded in DESIGN.md section 6.
"""
import collections

import pytest

import dmx
import lenient_streams as LS

pytestmark = pytest.mark.gpu

ERR = {-1: dmx.DMX_ERR_OVERREAD, -2: dmx.DMX_ERR_DATA}
N_SINGLE = 128  # cases per family on the single-stream routes; the batch routes take all N_CASES
CAP = LS.MAX_OUT + 64

# route -> (Context arguments, the paths a forced pass may report, RFC mode).  The first path
# is the forced pass's own (as stats().path reports it: 3 for pass 2, 2 for pass 7); 2 is the
# serial decoder, the net under every route.  A plan forced to pass 0 or 2 also ends in the
# wave-per-segment decoder (pass 1, inflate_pass_plan: "if (forced != 1 && forced != 4)
# p.add(1, 0)"), which takes what the forced pass reports as not its layout: path 1 there is
# the plan as designed, not an escape from it.
ROUTES = {
    "default": ({}, None, False),
    "pass0": ({"inflate_pass": 0}, (0, 1, 2), False),
    "pass1": ({"inflate_pass": 1}, (1, 2), False),
    "pass2": ({"inflate_pass": 2}, (3, 1, 2), False),
    "pass4": ({"inflate_pass": 4}, (4, 2), False),
    "pass5": ({"inflate_pass": 5}, (5, 2), False),
    "pass7": ({"inflate_pass": 7}, (2,), False),
    "pass4_heavy64": ({"inflate_pass": 4, "heavy_bytes": 64}, (4, 2), False),
    "pass5_fb_serial": ({"inflate_pass": 5, "fb_serial": True}, (5, 2), False),
    "rfc_strict": ({"rfc_strict": True}, None, True),
}


def _describe(got):
    return "error %d" % got.code if isinstance(got, dmx.DmxError) else "%d bytes" % len(got)


def _mismatch(fam, i, case, want, got):
    """None when `got` (bytes or a DmxError) is what the oracle expects, else a description."""
    out, err = want
    if err is None:
        if isinstance(got, dmx.DmxError) or got != out:
            return "%s[%d]%s: want %d bytes, got %s" % (fam, i, case.note, len(out), _describe(got))
    elif not isinstance(got, dmx.DmxError) or got.code != ERR[err]:
        return "%s[%d]%s: want error %d, got %s" % (fam, i, case.note, ERR[err], _describe(got))
    return None


def _report(bad, total):
    assert not bad, "%d of %d cases differ from the oracle:\n%s" % (len(bad), total, "\n".join(bad[:20]))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_single_stream_routes(route):
    kw, paths, rfc = ROUTES[route]
    forced_path = paths[0] if paths else None
    c = dmx.Context(**kw)
    bad, total, forced_seen = [], 0, False
    try:
        for fam in LS.FAMILIES:
            hist = collections.Counter()
            want = LS.expected_all(fam, rfc=rfc)
            for i, case in enumerate(LS.cases(fam)[:N_SINGLE]):
                try:
                    got = c.decompress(case.stream)
                except dmx.DmxError as e:
                    got = e
                path = c.stats().path
                hist[path] += 1
                total += 1
                m = _mismatch(fam, i, case, want[i], got)
                if m:
                    bad.append(m + " (path %d)" % path)
                if forced_path is not None:
                    if path not in paths:
                        bad.append("%s[%d]: path %d on a route forced to %d" % (fam, i, path, forced_path))
                    if fam == "prefix" and want[i][1] is None and path == forced_path:
                        forced_seen = True
            print("paths %-16s %-11s %s" % (route, fam, dict(sorted(hist.items()))))
    finally:
        c.close()
    _report(bad, total)
    assert forced_path is None or forced_seen, "no decodable prefix case took path %d" % forced_path


def _check_batch(fam, want, vals, res, keep=None):
    bad = []
    for i, case in enumerate(LS.cases(fam)):
        if keep is not None and not keep[i]:
            continue
        m = _mismatch(fam, i, case, want[i], vals[i])
        if m:
            bad.append(m)
        if res[i][2] != dmx.BATCH_PATH:
            bad.append("%s[%d]: path %d, not the batch decoder" % (fam, i, res[i][2]))
    return bad


@pytest.mark.parametrize("rfc", [False, True], ids=["reference", "rfc_strict"])
def test_batch_route(rfc):
    c = dmx.Context(rfc_strict=rfc)
    bad = []
    try:
        for fam in LS.FAMILIES:
            streams = [case.stream for case in LS.cases(fam)]
            vals, res = c.decompress_batch(streams, [CAP] * len(streams), no_route=True, with_results=True)
            bad += _check_batch(fam, LS.expected_all(fam, rfc=rfc), vals, res)
    finally:
        c.close()
    _report(bad, len(LS.FAMILIES) * LS.N_CASES)


def test_batch_async_route(ctx):
    import torch
    bad = []
    ctx.batch_reserve(LS.N_CASES, LS.MAX_STREAM)
    for fam in LS.FAMILIES:
        streams = [case.stream for case in LS.cases(fam)]
        offs, pos = [], 0
        for s in streams:
            offs.append(pos)
            pos += (len(s) + 15) & ~15
        blob = bytearray(pos + 16)
        for o, s in zip(offs, streams):
            blob[o:o + len(s)] = s
        d_blob = torch.frombuffer(blob, dtype=torch.uint8).cuda()
        d_out = torch.zeros(len(streams) * CAP, dtype=torch.uint8, device="cuda")
        i64 = lambda v: torch.tensor(v, dtype=torch.int64).cuda()  # noqa: E731
        d_in, d_n = i64([d_blob.data_ptr() + o for o in offs]), i64([len(s) for s in streams])
        d_op, d_cap = i64([d_out.data_ptr() + i * CAP for i in range(len(streams))]), i64([CAP] * len(streams))
        d_res = torch.zeros(len(streams) * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.inflate_batch_async(d_in.data_ptr(), d_n.data_ptr(), len(streams), LS.MAX_STREAM, d_op.data_ptr(),
                                d_cap.data_ptr(), d_res.data_ptr(), no_route=True)
        torch.cuda.synchronize()
        res = dmx.batch_results(d_res)
        host = d_out.cpu().numpy().tobytes()
        vals = [host[i * CAP:i * CAP + r[0]] if r[1] == dmx.DMX_OK else dmx.DmxError(r[1], "inflate_batch_async")
                for i, r in enumerate(res)]
        bad += _check_batch(fam, LS.expected_all(fam), vals, res)
    _report(bad, len(LS.FAMILIES) * LS.N_CASES)


def test_batch_dictionary_route(ctx, oracle):
    """The same cases behind a 1 KiB preset dictionary: expected is the oracle's result for a
    stored block of the dictionary followed by the case, minus the dictionary bytes.  A copy that
    reaches before the dictionary ("distance beyond the start") copies nothing for the oracle;
    with a dictionary that is not defined, so the cases that do it are dropped (under 10 %)."""
    zdict = dmx.corpus("text", 1024, offset=4321)
    head = b"\x00" + (1024).to_bytes(2, "little") + (1024 ^ 0xFFFF).to_bytes(2, "little") + zdict
    bad, dropped = [], 0
    for fam in LS.FAMILIES:
        cs = LS.cases(fam)
        keep = [case.far_by <= len(zdict) for case in cs]
        dropped += keep.count(False)
        want = []
        for case in cs:
            out, err = LS.expected(oracle, head + case.stream)
            want.append((out[len(zdict):] if err is None else None, err))
        vals, res = ctx.decompress_batch([case.stream for case in cs], [CAP] * len(cs), zdict=zdict, no_route=True,
                                         with_results=True)
        bad += _check_batch(fam, want, vals, res, keep)
    total = len(LS.FAMILIES) * LS.N_CASES
    print("dictionary batch: dropped %d of %d cases (a copy from before the dictionary)" % (dropped, total))
    assert 10 * dropped < total
    _report(bad, total - dropped)


def test_many_lenient_segments_in_one_stream(ctx, oracle):
    """200 decodable, self-contained, non-final lenient blocks (50 each of prefix, incomplete,
    overshoot, sixteen) as segments of one libdmx-layout stream: each followed by an empty stored
    block, a final empty block at the end.  The lane decoder's own header reader declines nearly
    all of them (codes beyond 9 / 6 bits, HLIT above 286, the overshoot and 16 rules, a leading
    empty block), and the patch pass takes at most one candidate in eight (pass_skipped), so the
    200 stand among 1800 segments inside the lane decoder's limits (lane_case: random complete
    codes, the edge matches): the lanes decode those, the patch pass the 200, side by side, and
    the stream stays on path 4."""
    parts = []
    for fam in ("prefix", "incomplete", "overshoot", "sixteen"):
        want = LS.expected_all(fam)
        idx = [i for i, case in enumerate(LS.cases(fam)) if want[i][1] is None and case.far_by == 0][:50]
        assert len(idx) == 50
        parts += [LS.make_case(fam, i, final=False).stream for i in idx]
    i = 0
    while len(parts) < 2000:
        case = LS.lane_case(i)
        i += 1
        if case.far_by == 0:
            parts.append(case.stream)
    LS.Rng(7).shuffle(parts)
    s = b"".join(parts) + b"\x01\x00\x00\xff\xff"
    want = oracle.inflate(s)
    assert len(want) > 2000
    assert ctx.decompress(s) == want
    assert ctx.stats().path == 4


def _pass5(s, fb_serial):
    c = dmx.Context(inflate_pass=5, fb_serial=fb_serial)
    try:
        return c.decompress(s), c.stats()
    finally:
        c.close()


@pytest.mark.parametrize("fb_serial", [False, True])
def test_region_map_over_odd_fixed_blocks(oracle, fb_serial):
    """One run of fixedodd Huffman blocks (286/287, 30/31, overlapping copies and copies from up to
    32768 back; no stored block) of 3 super blocks of 2^18 bits: the fixed-code region map and
    its units, lane-parallel and (fb_serial) one wavefront per unit."""
    s = LS.fixed_run(11, 96 << 10)
    assert len(s) >= 96 << 10
    got, st = _pass5(s, fb_serial)
    assert got == oracle.inflate(s)
    assert st.path == 5
    assert st.segments >= 3


@pytest.mark.parametrize("fb_serial", [False, True])
@pytest.mark.parametrize("kind", ["before_start", "tiny_blocks"])
def test_region_streams_the_block_path_declines(oracle, fb_serial, kind):
    """Two shapes of the same run that the block-parallel path declines by design, to the serial
    decoder: copies that reach before the first output byte (only the unit at bit 0 knows where
    the stream starts; a later unit's open copy that resolves to before it is flagged), and, with
    fb_serial, blocks of 20..400 tokens (a one-wavefront unit leaves a far fixed run after one
    block, FB_SER_FIXED_MAX, so the repair rounds run out).  Declined or not, the bytes are the
    oracle's."""
    s = (LS.fixed_run(12, 96 << 10, before_start=True) if kind == "before_start"
         else LS.fixed_run(13, 96 << 10, 20, 400))
    got, st = _pass5(s, fb_serial)
    print("region stream %s fb_serial %s: path %d" % (kind, fb_serial, st.path))
    assert got == oracle.inflate(s)
    assert st.path in (5, 2)
