"""GPU: the deflate's chunk pipeline (launch_deflate: chunk i's emission on the context's side
stream beside chunk i + 1's front kernel).  DMX_DEFLATE_PIPE=s64 forces chunks of 64 segments, so
that a few MiB run several chunks; the same library with DMX_DEFLATE_PIPE=0 takes the single
launch.  The knob is read when a context is created.

Bytes: the pipeline's stream equals the single launch's, byte for byte, and zlib decodes it to the
input -- six corpora at level 2, text and repeat at level 3; sizes of exactly three chunks, three
chunks and a segment (+ 1, 3, 5 bytes), one chunk and a segment, and one chunk (below the
threshold: the single launch on both sides).  64 KiB blocks ending on a whole block, on a block
and a half, and on short halves.  16 KiB segments and levels 0 / 1 keep their path.
Ordering: events are all that orders the side stream, so the input written just before the call
on the caller's stream, two asynchronous calls from two streams, deflate -> inflate with no host
read between, and a context closed right behind an asynchronous call must all give the bytes."""
import os
import zlib

import pytest

import dmx

pytestmark = pytest.mark.gpu

SEG = 32768
CHUNK = 64  # segments per forced chunk
KINDS = ["repeat", "text", "mixed", "bmp", "zeros", "random"]
CASES = [(k, 2) for k in KINDS] + [("text", 3), ("repeat", 3)]
SIZES = [3 * CHUNK * SEG, (3 * CHUNK + 1) * SEG, (3 * CHUNK + 1) * SEG + 1, (3 * CHUNK + 1) * SEG + 3,
         (3 * CHUNK + 1) * SEG + 5, (CHUNK + 1) * SEG, CHUNK * SEG]
NMAX = max(SIZES)


def _context(knob, **kw):
    old = os.environ.get("DMX_DEFLATE_PIPE")
    os.environ["DMX_DEFLATE_PIPE"] = knob
    try:
        return dmx.Context(**kw)
    finally:
        if old is None:
            del os.environ["DMX_DEFLATE_PIPE"]
        else:
            os.environ["DMX_DEFLATE_PIPE"] = old


@pytest.fixture(scope="module")
def pair():
    off, pipe = _context("0"), _context(f"s{CHUNK}")
    yield off, pipe
    off.close()
    pipe.close()


@pytest.fixture(scope="module")
def pair64():
    off, pipe = _context("0", segment_bytes=65536), _context(f"s{CHUNK}", segment_bytes=65536)
    yield off, pipe
    off.close()
    pipe.close()


_corpora = {}


def _corpus(kind):
    if kind not in _corpora:
        _corpora[kind] = dmx.corpus(kind, NMAX)
    return _corpora[kind]


def _zlib_inflate(s, tail=b""):
    d = zlib.decompressobj(-15)
    out = d.decompress(s)
    assert not d.eof or not tail, "a stream that is not final has no BFINAL block"
    if tail:
        out += d.decompress(tail)
    out += d.flush()
    assert d.eof and not d.unused_data
    return out


@pytest.mark.parametrize("kind,level", CASES)
def test_pipeline_bytes(pair, kind, level):
    off, pipe = pair
    full = _corpus(kind)
    for n in SIZES:
        data = full[:n]
        want = off.compress(data, level)
        got = pipe.compress(data, level)
        assert got == want, f"{kind} level {level} n={n}: the pipeline's stream differs"
        assert _zlib_inflate(got) == data, f"{kind} level {level} n={n}"


def test_pipeline_64k_blocks(pair64):
    off, pipe = pair64
    blk = 65536
    n0 = (2 * CHUNK + 1) * blk
    full = dmx.corpus("mixed", n0 + blk)
    # a whole block; a block and one half; a short second half; a short first half
    for n in (n0, n0 + 32768, n0 + 32768 + 1000, n0 + 1000):
        data = full[:n]
        want = off.compress(data, 2)
        got = pipe.compress(data, 2)
        assert got == want, f"64 KiB blocks n={n}"
        assert _zlib_inflate(got) == data


def test_other_paths_keep_their_bytes(pair):
    off, pipe = pair
    data = _corpus("mixed")[: (3 * CHUNK + 1) * SEG + 5]
    for level in (0, 1):
        assert pipe.compress(data, level) == off.compress(data, level)
    a, b = _context("0", segment_bytes=16384), _context(f"s{CHUNK}", segment_bytes=16384)
    try:
        for level in (2, 3):
            s = b.compress(data, level)
            assert s == a.compress(data, level)
            assert _zlib_inflate(s) == data
    finally:
        a.close()
        b.close()


def _dev(torch, data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def test_not_final(pair):
    import torch
    off, pipe = pair
    data = _corpus("text")[: (3 * CHUNK + 1) * SEG + 3]
    d_in = _dev(torch, data)
    cap = dmx.deflate_bound(len(data)) + 64
    outs = []
    for c in (off, pipe):
        d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        clen = c.deflate_device(d_in.data_ptr(), len(data), 2, d_c.data_ptr(), cap, not_final=True)
        outs.append(d_c[:clen].cpu().numpy().tobytes())
    assert outs[0] == outs[1]
    assert _zlib_inflate(outs[1], tail=b"\x03\x00") == data


def test_input_written_just_before_the_call(pair):
    """The emission of a stored block reads the input itself, on the side stream: it must be
    ordered behind the caller's stream, where the input is still being written."""
    import torch
    off, pipe = pair
    data = _corpus("random")[: (3 * CHUNK + 1) * SEG + 5]
    want = off.compress(data, 2)
    src = _dev(torch, data)
    torch.cuda.synchronize()
    cap = dmx.deflate_bound(len(data)) + 64
    d_in = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    big = torch.zeros(1 << 28, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(150):  # some twenty milliseconds of work ahead of the input's copy
            big.add_(1)
        d_in.copy_(src, non_blocking=True)
    pipe.deflate_device_async(d_in.data_ptr(), len(data), 2, d_c.data_ptr(), cap, d_len.data_ptr(),
                              stream=s.cuda_stream)
    torch.cuda.synchronize()
    n = int(d_len[0])
    assert n == len(want)
    assert d_c[:n].cpu().numpy().tobytes() == want


def test_two_async_calls_from_two_streams(pair):
    import torch
    off, pipe = pair
    a = _corpus("mixed")[: (3 * CHUNK + 1) * SEG + 1]
    b = _corpus("random")[: 3 * CHUNK * SEG]
    wa, wb = off.compress(a, 2), off.compress(b, 3)
    da, db = _dev(torch, a), _dev(torch, b)
    cap = dmx.deflate_bound(len(a)) + 64
    oa = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    ob = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(2, dtype=torch.int64, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    pipe.deflate_device_async(da.data_ptr(), len(a), 2, oa.data_ptr(), cap, d_len.data_ptr(), stream=s1.cuda_stream)
    pipe.deflate_device_async(db.data_ptr(), len(b), 3, ob.data_ptr(), cap, d_len.data_ptr() + 8,
                              stream=s2.cuda_stream)
    torch.cuda.synchronize()
    la, lb = (int(x) for x in d_len.tolist())
    assert (la, lb) == (len(wa), len(wb))
    assert oa[:la].cpu().numpy().tobytes() == wa
    assert ob[:lb].cpu().numpy().tobytes() == wb


def test_async_deflate_then_async_inflate(pair):
    import torch
    off, pipe = pair
    data = _corpus("mixed")[: (3 * CHUNK + 1) * SEG + 3]
    want = off.compress(data, 2)  # (the length the inflate call needs on the host)
    d_in = _dev(torch, data)
    cap = dmx.deflate_bound(len(data)) + 64
    d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_o = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_r = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    pipe.deflate_device_async(d_in.data_ptr(), len(data), 2, d_c.data_ptr(), cap, d_len.data_ptr(),
                              stream=s.cuda_stream)
    pipe.inflate_device_async(d_c.data_ptr(), len(want), d_o.data_ptr(), d_o.numel(), d_r.data_ptr(),
                              stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert int(d_len[0]) == len(want)
    assert tuple(int(x) for x in d_r.tolist()) == (len(data), 0)
    assert d_o[: len(data)].cpu().numpy().tobytes() == data


def test_context_closed_behind_an_async_call(pair):
    import torch
    off, _ = pair
    data = _corpus("text")[: (3 * CHUNK + 1) * SEG + 5]
    want = off.compress(data, 2)
    d_in = _dev(torch, data)
    cap = dmx.deflate_bound(len(data)) + 64
    d_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    c = _context(f"s{CHUNK}")
    c.deflate_device_async(d_in.data_ptr(), len(data), 2, d_c.data_ptr(), cap, d_len.data_ptr(), stream=s.cuda_stream)
    c.close()
    torch.cuda.synchronize()
    n = int(d_len[0])
    assert n == len(want)
    assert d_c[:n].cpu().numpy().tobytes() == want
