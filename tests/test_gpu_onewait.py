"""GPU: the synchronous round trip with one host wait per call.

dmx_inflate_device into a caller's buffer launches its first pass before the candidate count is
known (inflate_plan.h: spec_wanted / spec_decide).  DMX_INFLATE_SPEC is read when a context is
created: "0" keeps the classic flow, "1" is the default, "force" drops the capacity gate so that
small streams reach every branch.  Every case decodes the same stream with the knob at 0 and at
force (and at 1 where the capacity passes the gate); the runs must agree in return code, output
length, stats.path, stats.segments and the decoded bytes.

The cases: 3 segments (the count is at or below the gate: discarded); 2049 segments of `repeat`
(the smallest accepted speculation) and of `repeat` ending in 1 MiB of `text` (dense segments:
within the heavy limit at this count, so the lanes decline them and the plan goes on from its
second pass); the same with the capacity one byte short; 16 KiB segments decoded by a 32 KiB
context with cap equal to the output (more candidates than provisioned); a zlib level-1 stream
(no marker, path 5); the 2049-segment stream truncated and with a corrupted block header; 1 MiB of
dense text (heavy route).

The scan (k_scan_apply sums up to 8 blocks of 8192 values itself, k_scan_part runs above that):
level-0 deflates of n = 1, 8191, 8192, 8193, 65536 and 65537 segments of 16 KiB, whose stored
segments have known sizes -- the stream's length and every segment's offset against numpy's
cumsum, and the decoded bytes against the input.

The deflate's bytes: 1, 2 and 513 segments at levels 0 and 2 against digests recorded with the
library of the commit before this change."""
import ctypes
import hashlib
import os
import zlib

import numpy as np
import pytest

import dmx

pytestmark = pytest.mark.gpu

SEG = 32768
N2049 = 2049 * SEG  # 64 MiB + 32 KiB
DMX_OK = 0


def _context(knob, **kw):
    old = os.environ.get("DMX_INFLATE_SPEC")
    os.environ["DMX_INFLATE_SPEC"] = knob
    try:
        return dmx.Context(**kw)
    finally:
        if old is None:
            del os.environ["DMX_INFLATE_SPEC"]
        else:
            os.environ["DMX_INFLATE_SPEC"] = old


@pytest.fixture(scope="module")
def ctxs():
    c = {k: _context(k) for k in ("0", "1", "force")}
    yield c
    for x in c.values():
        x.close()


def _dev(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


_streams = {}


def _big(kind):
    """(device stream, its length, plain bytes on the device) of the 2049-segment corpora"""
    import torch
    if kind not in _streams:
        if kind == "repeat":
            plain = dmx.corpus("repeat", N2049)
        else:  # repeat ending in 1 MiB of text
            plain = dmx.corpus("repeat", N2049 - (1 << 20)) + dmx.corpus("text", 1 << 20)
        d_in = _dev(plain)
        cap = dmx.deflate_bound(N2049) + 64
        d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        c = _context("0")
        torch.cuda.synchronize()  # (the context's stream is not torch's: the inputs must be there)
        clen = c.deflate_device(d_in.data_ptr(), N2049, 2, d_c.data_ptr(), cap)
        c.close()
        _streams[kind] = (d_c[:clen].clone(), clen, d_in)
    return _streams[kind]


def _inflate(ctx, d_s, n, cap):
    """(rc, output length, path, segments, output bytes [0, min(length, cap)) as a device tensor)"""
    import torch
    d_o = torch.full((max(cap, 1) + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    out_len = ctypes.c_size_t()
    torch.cuda.synchronize()  # the stream and the fill, written on torch's stream
    rc = dmx.lib().dmx_inflate_device(ctx.h, ctypes.c_void_p(d_s.data_ptr()), n, ctypes.c_void_p(d_o.data_ptr()), cap,
                                      ctypes.byref(out_len), None)
    st = ctx.stats()
    torch.cuda.synchronize()
    return rc, out_len.value, st.path, st.segments, d_o[: min(out_len.value, cap)]


def _agree(ctxs, knobs, d_s, n, cap, want=None):
    import torch
    runs = [_inflate(ctxs[k], d_s, n, cap) for k in knobs]
    base = runs[0]
    for k, r in zip(knobs[1:], runs[1:]):
        assert r[:4] == base[:4], f"knob {k}: (rc, length, path, segments) {r[:4]} against {base[:4]} with knob {knobs[0]}"
        if base[0] == DMX_OK or base[0] == dmx.DMX_ERR_CAPACITY:
            assert torch.equal(r[4], base[4]), f"knob {k}: decoded bytes differ"
    if want is not None:
        assert base[0] == DMX_OK and base[1] == want.numel() and torch.equal(base[4], want)
    return base


def test_three_segments_discarded(ctxs):
    data = dmx.corpus("mixed", 3 * SEG - 100)
    s = ctxs["0"].compress(data, 2)
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "force", "1"], _dev(s), len(s), len(data) + 64, want=_dev(data))
    assert (path, segs) == (4, 3)


@pytest.mark.parametrize("kind", ["repeat", "repeat_text"])
def test_2049_segments_accepted(ctxs, kind):
    d_s, clen, d_plain = _big(kind)
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "1", "force"], d_s, clen, N2049 + 64, want=d_plain)
    assert (path, segs) == (4, 2049)


def test_2049_segments_capacity_one_short(ctxs):
    d_s, clen, d_plain = _big("repeat")
    # (cap / segment is 2048 here: the default knob does not speculate, force does)
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "force", "1"], d_s, clen, N2049 - 1)
    assert rc == dmx.DMX_ERR_CAPACITY and olen == N2049


def test_more_candidates_than_provisioned(ctxs):
    data = dmx.corpus("mixed", 3 << 20)
    c16 = _context("0", segment_bytes=16384)
    s = c16.compress(data, 2)
    c16.close()
    # 192 segments of 16 KiB against 3 MiB / 32 KiB + 64 = 160 provisioned candidates
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "force"], _dev(s), len(s), len(data), want=_dev(data))
    assert segs == 192


def test_zlib_stream_without_marker(ctxs):
    data = dmx.corpus("mixed", 1 << 20)
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    s = z.compress(data) + z.flush()
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "force"], _dev(s), len(s), len(data) + 64, want=_dev(data))
    assert path == 5


def test_truncated_and_corrupted(ctxs):
    import torch
    d_s, clen, _ = _big("repeat")
    starts = ctxs["0"].segment_starts_device(d_s.data_ptr(), clen)
    mid = int(starts[999])  # (the list begins with segment 1: segment 0 starts the stream)
    # truncated in the middle of segment 1000
    cut = mid + (int(starts[1000]) - mid) // 2
    a = _agree(ctxs, ["0", "force", "1"], d_s[:cut].clone(), cut, N2049 + 64)
    assert a[0] != DMX_OK
    # one corrupted block header: BTYPE 3 at the start of segment 1000
    bad = d_s.clone()
    bad[mid] = int(bad[mid]) | 0x06
    torch.cuda.synchronize()
    b = _agree(ctxs, ["0", "force", "1"], bad, clen, N2049 + 64)
    assert b[0] != DMX_OK


def test_dense_text_heavy_route(ctxs):
    data = dmx.corpus("text", 1 << 20)
    s = ctxs["0"].compress(data, 2)
    rc, olen, path, segs, _ = _agree(ctxs, ["0", "force", "1"], _dev(s), len(s), len(data) + 64, want=_dev(data))
    assert (path, segs) == (4, 32)


# ---- the scan ------------------------------------------------------------------------------

SEG16 = 16384


@pytest.fixture(scope="module")
def ctx16():
    c = _context("1", segment_bytes=SEG16)
    yield c
    c.close()


@pytest.mark.parametrize("nseg", [1, 8191, 8192, 8193, 65536, 65537])
def test_scan_offsets_against_cumsum(ctx16, nseg):
    import torch
    last = 1000  # bytes of the last segment
    n = (nseg - 1) * SEG16 + last
    d_in = torch.arange(n, dtype=torch.int32, device="cuda").remainder_(251).to(torch.uint8)
    cap = dmx.deflate_bound(n) + 64
    d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the context's stream is not torch's)
    clen = ctx16.deflate_device(d_in.data_ptr(), n, 0, d_c.data_ptr(), cap)
    # a stored segment: 5 header bytes and the data; all but the last end on an empty stored block
    sizes = np.full(nseg, 5 + SEG16 + 5, dtype=np.uint32)
    sizes[-1] = 5 + last
    ends = np.cumsum(sizes, dtype=np.uint64)
    assert clen == int(ends[-1])
    offs = torch.from_numpy((ends - sizes).astype(np.int64)).cuda()
    lens = torch.full((nseg,), SEG16, dtype=torch.int64, device="cuda")
    lens[-1] = last
    final = torch.zeros(nseg, dtype=torch.int64, device="cuda")
    final[-1] = 1

    def pick(k):
        return d_c[offs + k].to(torch.int64)

    assert torch.equal(pick(0), final), "a segment's block header is not at its offset"
    assert torch.equal(pick(1) | (pick(2) << 8), lens)
    assert torch.equal(pick(3) | (pick(4) << 8), lens ^ 0xFFFF)
    d_o = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    olen = ctx16.inflate_device(d_c.data_ptr(), clen, d_o.data_ptr(), n + 64)
    assert olen == n and torch.equal(d_o[:n], d_in)


# ---- the deflate's bytes against the commit before ------------------------------------------

PARENT_DIGESTS = {
    (1, 0): (32773, "82043b0de2dd1d552f16a4020909155d11f15d37d72254932de4e3693ecd4214"),
    (1, 2): (12963, "10d86f224907280391029436b78a9453dbc82d057f1d5103be975058b4eefb2f"),
    (2, 0): (65551, "9d15e950a382ecf818e64751fae64784f4abaabc64a71f7da5cd4607c8483fe4"),
    (2, 2): (26153, "0ee237d826be00728b1c2c7cb1230d36ede38ae92c827b411e173408214931e6"),
    (513, 0): (16813875, "ea78c70bedae340d2e0123d352b52583a8312a0afa17078c06917feac1323743"),
    (513, 2): (6166625, "0e02af85c3f3eace4457951bf203ff1914db2908c6ff893f1aec214d0d5f55b9"),
}


def test_deflate_bytes_equal_the_parents(ctxs):
    full = dmx.corpus("mixed", 513 * SEG)
    for (k, level), (length, digest) in PARENT_DIGESTS.items():
        n = {1: SEG, 2: 2 * SEG, 513: 513 * SEG - 1234}[k]
        s = ctxs["1"].compress(full[:n], level)
        assert (len(s), hashlib.sha256(s).hexdigest()) == (length, digest), f"{k} segments, level {level}"
