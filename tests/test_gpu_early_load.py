"""GPU: the front kernel's early load (DMX_DF_EARLYLOAD, DESIGN 4.1 "Early load").

A persistent workgroup loads its next segment into the match rounds' table while the parse walk
of the current one runs, and the byte image and the table swap roles on every segment.  A
segment is staged only when it is a full one at a 16-aligned address without a dictionary; any
other loads at its own start, into whichever buffer is the image then.  The pins
(test_gpu_deflate_pins.py, test_gpu_parse_pins.py) tie the aligned host path to the streams of
the builds before; here staged and unstaged segments follow each other inside one workgroup,
at every source alignment, and the grid's edges are crossed.

G = the front kernel's grid (CUs x workgroups per CU: 1 at 32 and 64 KiB, 2 at 16 KiB), S = its
segment size (64 KiB blocks are matched as two 32 KiB halves).  n = (2G + 3) S + 1234: every
workgroup takes two or three segments, and the short last segment follows staged ones.
"""
import zlib

import numpy as np
import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu
KINDS = ("repeat", "text", "zeros", "random")


def front(seg):
    """(G, S) of a context with segment_bytes = seg."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (2 * cus, 16384) if seg == 16384 else (cus, 32768)


@pytest.fixture(scope="module")
def ctxs():
    c = {seg: dmx.Context(segment_bytes=seg) for seg in (16384, 32768, 65536)}
    yield c
    for x in c.values():
        x.close()


_corpora = {}


def corpus(kind, n):
    """The first n bytes of a corpus (generated once at the largest size asked for)."""
    have = _corpora.get(kind)
    if have is None or len(have) < n:
        have = _corpora[kind] = np.frombuffer(dmx.corpus(kind, n), dtype=np.uint8)
    return have[:n]


_mixes = {}


def interleaved(G, S, n):
    """n bytes whose segment i comes from corpus (i + i // G) mod 4 (its own bytes [i S, i S + S)):
    neighbouring segments differ, and so do the segments i, i + G, i + 2G of one workgroup, so run
    segments and run-free ones alternate on every workgroup."""
    if (G, S, n) not in _mixes:
        nseg = (n + S - 1) // S
        src = np.stack([corpus(k, nseg * S).reshape(nseg, S) for k in KINDS])
        i = np.arange(nseg)
        _mixes[(G, S, n)] = src[(i + i // G) % len(KINDS), i].reshape(-1)[:n].tobytes()
    return _mixes[(G, S, n)]


def inflate(comp, zdict=None):
    z = zlib.decompressobj(-15, zdict=zdict) if zdict is not None else zlib.decompressobj(-15)
    out = z.decompress(comp)
    assert z.eof and not z.unused_data
    return out


def deflate_at(ctx, data, level, offset):
    """The stream of deflate_device for data placed `offset` bytes into a device buffer."""
    n = len(data)
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    cap = dmx.deflate_bound(n) + 64
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    clen = ctx.deflate_device(buf.data_ptr() + offset, n, level, out.data_ptr(), cap)
    return out[:clen].cpu().numpy().tobytes()


@pytest.mark.parametrize("level", (2, 3))
@pytest.mark.parametrize("seg", (16384, 32768, 65536))
def test_alignment(ctxs, seg, level):
    """Offsets 1 and 8 make every segment unstaged; 0 and 16 stage all but the last."""
    G, S = front(seg)
    data = interleaved(G, S, (2 * G + 3) * S + 1234)
    ref = ctxs[seg].compress(data, level)
    assert inflate(ref) == data
    for offset in (0, 1, 8, 16):
        assert deflate_at(ctxs[seg], data, level, offset) == ref, f"offset {offset}"


def batch_streams(ctx, bufs, level, zdict=None):
    """deflate_batch_device over buffers cycling through three kinds of placement: S bytes at a
    16-aligned address (staged), S bytes at an odd address, and S - 5 bytes (both unstaged)."""
    slot = 32768 + 64
    arena = torch.zeros(len(bufs) * slot, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    host = np.zeros(len(bufs) * slot, dtype=np.uint8)
    ptrs, sizes = [], []
    for i, b in enumerate(bufs):
        at = i * slot + (1 if i % 3 == 1 else 0)
        host[at:at + len(b)] = np.frombuffer(b, dtype=np.uint8)
        ptrs.append(arena.data_ptr() + at)
        sizes.append(len(b))
    arena.copy_(torch.from_numpy(host))
    cap = dmx.deflate_bound(32768) + 64
    outs = torch.empty(len(bufs) * cap, dtype=torch.uint8, device="cuda")
    optrs = [outs.data_ptr() + i * cap for i in range(len(bufs))]
    kw = {}
    if zdict is not None:
        d = torch.frombuffer(bytearray(zdict), dtype=torch.uint8).cuda()
        kw = dict(dict_ptr=d.data_ptr(), dict_len=len(zdict))
    res = ctx.deflate_batch_device(ptrs, sizes, level, optrs, [cap] * len(bufs), **kw)
    torch.cuda.synchronize()
    h = outs.cpu().numpy()
    assert all(status == 0 for _, status, _ in res)
    return [h[i * cap:i * cap + nbytes].tobytes() for i, (nbytes, _, _) in enumerate(res)]


def batch_buffers():
    G, S = front(32768)
    data = interleaved(G, S, (2 * G + 7) * S)
    return [data[i * S:i * S + (S - 5 if i % 3 == 2 else S)] for i in range(2 * G + 7)]


def test_alternation_in_a_workgroup(ctxs):
    """Staged, unstaged and short segments follow each other on every workgroup (G and 3 have no
    common pattern over 2G + 7 buffers); each stream is that of the buffer compressed alone."""
    ctx = ctxs[32768]
    bufs = batch_buffers()
    for i, (b, s) in enumerate(zip(bufs, batch_streams(ctx, bufs, 2))):
        assert s == ctx.compress(b, 2), i
        assert inflate(s) == b, i


def test_alternation_with_a_dictionary(ctxs):
    """Dictionary segments are never staged, but the buffers swap around them."""
    zdict = corpus("text", 65536)[40000:40000 + 4096].tobytes()
    bufs = batch_buffers()
    for i, s in enumerate(batch_streams(ctxs[32768], bufs, 2, zdict=zdict)):
        assert inflate(s, zdict) == bufs[i], i


def test_grid_edges(ctxs):
    """G + 1 full segments is the smallest input for which exactly one workgroup prefetches."""
    ctx = ctxs[32768]
    G, S = front(32768)
    rep = corpus("repeat", 2 * G * S)
    for nseg in (1, G - 1, G, G + 1, 2 * G):
        data = rep[:nseg * S].tobytes()
        ref = ctx.compress(data, 2)
        assert inflate(ref) == data, nseg
        assert deflate_at(ctx, data, 2, 0) == ref, nseg


def test_context_reuse(ctxs):
    """A 3-segment call right after a (2G + 3)-segment one, whose launch issued prefetches."""
    G, S = front(32768)
    big = interleaved(G, S, (2 * G + 3) * S + 1234)
    small = interleaved(G, S, 3 * S)
    ctx = ctxs[32768]
    deflate_at(ctx, big, 2, 0)
    got = deflate_at(ctx, small, 2, 0)
    fresh = dmx.Context(segment_bytes=32768)
    try:
        assert got == deflate_at(fresh, small, 2, 0)
    finally:
        fresh.close()
    assert inflate(got) == small
