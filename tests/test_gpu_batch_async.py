"""GPU: the asynchronous batch calls (dmx_deflate_batch_async / dmx_inflate_batch_async): the
pointer, size and capacity arrays and the results live in device memory, and a call only
enqueues.  Per buffer the bytes and the result must equal the synchronous batch call's; a buffer
above max_n or beyond the segment table's capacity gets DMX_ERR_ARG and no output; a stream the
synchronous call would route is DMX_BATCH_DEFERRED; and the call must return while earlier work
on its stream -- the writes of its own descriptor arrays included -- is still running.

The helpers pack / out_area are those of test_gpu_batch.py (FILL-guarded output regions)."""
import json
import os
import sys
import time

import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from zgen import stream_of  # noqa: E402

MAN = json.load(open(os.path.join(GOLD, "manifest.json")))
VECS = [v for v in MAN["vectors"] if "stream" in v or "zgen" in v]

SIZES = [0, 1, 2, 3, 255, 4095, 16384, 32767, 32768, 32769, 65536, 65537, 100000, 98304]
KINDS = ["zeros", "random", "text", "mixed"]
ALIGNS = [0, 1, 7, 16]
FILL = 0xA5
GAP = 64
MAX_N = 100000
POISON = 0xEE  # the result records before a call


def inputs():
    bufs = [dmx.corpus(KINDS[i % 4], n, offset=1000 * i) for i, n in enumerate(SIZES)]
    aligns = [ALIGNS[(i + i // 4) % 4] for i in range(len(SIZES))]
    return bufs, aligns


def pack(bufs, aligns, mod):
    """One device tensor holding every buffer back to back, buffer i at an offset that is
    aligns[i] modulo `mod`; returns the tensor (kept alive by the caller) and the offsets."""
    offs, pos = [], 0
    for b, a in zip(bufs, aligns):
        pos += (a - pos) % mod
        offs.append(pos)
        pos += len(b)
    host = bytearray(pos + 16)
    for b, o in zip(bufs, offs):
        host[o:o + len(b)] = b
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 256 == 0
    return t, offs


def out_area(caps, gap=GAP):
    """A device tensor filled with FILL with one region of caps[i] + gap bytes per buffer."""
    offs, pos = [], 0
    for c in caps:
        offs.append(pos)
        pos += c + gap
    return torch.full((max(1, pos),), FILL, dtype=torch.uint8, device="cuda"), offs


def dev_i64(vals):
    return torch.tensor(list(vals), dtype=torch.int64).cuda()


def new_res(count):
    return torch.full((max(1, count) * 16,), POISON, dtype=torch.uint8, device="cuda")


def split(host, ooffs, res, caps):
    return [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)]


def untouched(host, ooffs, caps, i, written=0):
    """Region i holds FILL from `written` to its end, guard bytes included."""
    return host[ooffs[i] + written:ooffs[i] + caps[i] + GAP] == bytes([FILL]) * (caps[i] + GAP - written)


class Call:
    """The device side of one asynchronous call: descriptor tensors, output area, results."""

    def __init__(self, ptrs, sizes, caps):
        self.count = len(ptrs)
        self.caps = list(caps)
        self.out, self.ooffs = out_area(self.caps)
        self.d_in, self.d_n = dev_i64(ptrs), dev_i64(sizes)
        self.d_out, self.d_cap = dev_i64([self.out.data_ptr() + o for o in self.ooffs]), dev_i64(self.caps)
        self.res = new_res(self.count)

    def args(self):
        return self.d_in.data_ptr(), self.d_n.data_ptr()

    def outs(self):
        return self.d_out.data_ptr(), self.d_cap.data_ptr(), self.res.data_ptr()

    def read(self):
        """(results, bytes per buffer, the whole output area) after the caller has synchronised"""
        res = dmx.batch_results(self.res)[:self.count]
        host = self.out.cpu().numpy().tobytes()
        return res, split(host, self.ooffs, res, self.caps), host


def deflate_async(ctx, bufs, aligns, level, caps=None, max_n=MAX_N, max_total=0, dict_ptr=None, dict_len=0, stream=None):
    t, offs = pack(bufs, aligns, 16)
    caps = caps if caps is not None else [dmx.deflate_bound(len(b)) for b in bufs]
    c = Call([t.data_ptr() + o for o in offs], [len(b) for b in bufs], caps)
    torch.cuda.synchronize()  # the tensors above are written on torch's stream
    ctx.deflate_batch_async(*c.args(), c.count, max_n, level, *c.outs(), max_total=max_total, dict_ptr=dict_ptr,
                            dict_len=dict_len, stream=stream)
    c.keep = t
    return c


def inflate_async(ctx, streams, caps, aligns=None, max_n=None, no_route=False, dict_ptr=None, dict_len=0, stream=None):
    aligns = aligns if aligns is not None else [i % 4 for i in range(len(streams))]
    t, offs = pack(streams, aligns, 4)
    c = Call([t.data_ptr() + o for o in offs], [len(s) for s in streams], caps)
    torch.cuda.synchronize()
    ctx.inflate_batch_async(*c.args(), c.count, max_n if max_n is not None else max(len(s) for s in streams), *c.outs(),
                            no_route=no_route, dict_ptr=dict_ptr, dict_len=dict_len, stream=stream)
    c.keep = t
    return c


def deflate_sync(ctx, bufs, aligns, level, caps=None, dict_ptr=None, dict_len=0):
    t, offs = pack(bufs, aligns, 16)
    caps = caps if caps is not None else [dmx.deflate_bound(len(b)) for b in bufs]
    out, ooffs = out_area(caps)
    torch.cuda.synchronize()
    res = ctx.deflate_batch_device([t.data_ptr() + o for o in offs], [len(b) for b in bufs], level,
                                   [out.data_ptr() + o for o in ooffs], caps, dict_ptr=dict_ptr, dict_len=dict_len)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return res, split(host, ooffs, res, caps), host


def inflate_sync(ctx, streams, caps, aligns=None, dict_ptr=None, dict_len=0):
    aligns = aligns if aligns is not None else [i % 4 for i in range(len(streams))]
    t, offs = pack(streams, aligns, 4)
    out, ooffs = out_area(caps)
    torch.cuda.synchronize()
    res = ctx.inflate_batch_device([t.data_ptr() + o for o in offs], [len(s) for s in streams],
                                   [out.data_ptr() + o for o in ooffs], caps, no_route=True, dict_ptr=dict_ptr,
                                   dict_len=dict_len)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return res, split(host, ooffs, res, caps), host


@pytest.fixture(scope="module")
def ctx16():
    c = dmx.Context(segment_bytes=16384)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctxs(ctx, ctx16):
    return {32768: ctx, 16384: ctx16}


_REF = {}


def sync_ref(ctxs, seg, level):
    """deflate_batch_device of the test-1 buffers, computed once per context and level"""
    if (seg, level) not in _REF:
        bufs, aligns = inputs()
        _REF[seg, level] = deflate_sync(ctxs[seg], bufs, aligns, level)
    return _REF[seg, level]


def segments(n, seg, du=0):
    seg0 = seg - du
    return (1 if n else 0) if n <= seg0 else 1 + (n - seg0 + seg - 1) // seg


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact_total", [False, True])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("seg", [32768, 16384])
def test_deflate_equals_sync_batch(ctxs, seg, level, exact_total):
    bufs, aligns = inputs()
    want_res, want, want_host = sync_ref(ctxs, seg, level)
    c = deflate_async(ctxs[seg], bufs, aligns, level, max_total=sum(SIZES) if exact_total else 0)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res == want_res
    assert all(r[1:] == (dmx.DMX_OK, 0) for r in res)
    assert got == want
    assert host == want_host  # the same layout: every guard and unused byte is still FILL
    for i, r in enumerate(res):
        assert untouched(host, c.ooffs, c.caps, i, r[0]), i


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
def test_dictionary_both_directions(ctx, level):
    bufs, aligns = inputs()
    zdict = dmx.corpus("text", 20000, offset=77)
    dt = torch.frombuffer(bytearray(b"\0" + zdict), dtype=torch.uint8).cuda()
    dptr = dt.data_ptr() + 1  # an odd address
    want_res, want, want_host = deflate_sync(ctx, bufs, aligns, level, dict_ptr=dptr, dict_len=len(zdict))
    assert want != sync_ref({32768: ctx}, 32768, level)[1]  # the dictionary is used
    c = deflate_async(ctx, bufs, aligns, level, dict_ptr=dptr, dict_len=len(zdict))
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res == want_res and got == want and host == want_host
    caps = [len(b) for b in bufs]
    iw_res, iw, iw_host = inflate_sync(ctx, want, caps, dict_ptr=dptr, dict_len=len(zdict))
    assert iw == bufs
    d = inflate_async(ctx, want, caps, dict_ptr=dptr, dict_len=len(zdict))
    torch.cuda.synchronize()
    res, got, host = d.read()
    assert res == iw_res and got == iw and host == iw_host


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [32768, 16384])
def test_buffer_above_max_n(ctxs, seg):
    bufs, aligns = inputs()
    want_res, want, _ = sync_ref(ctxs, seg, 2)
    k = 5
    bufs2 = bufs[:k] + [dmx.corpus("text", MAX_N + 1, offset=31)] + bufs[k:]
    aligns2 = aligns[:k] + [1] + aligns[k:]
    c = deflate_async(ctxs[seg], bufs2, aligns2, 2)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res[k] == (0, dmx.DMX_ERR_ARG, 0)
    assert untouched(host, c.ooffs, c.caps, k)
    assert res[:k] + res[k + 1:] == want_res
    assert got[:k] + got[k + 1:] == want
    for i, r in enumerate(res):
        assert untouched(host, c.ooffs, c.caps, i, r[0]), i


@pytest.mark.parametrize("seg", [32768, 16384])
def test_max_total_one_segment_short(ctxs, seg):
    bufs, aligns = inputs()
    want_res, want, _ = sync_ref(ctxs, seg, 2)
    counts = [segments(n, seg) for n in SIZES]
    need = sum(counts)
    # capacity = ceil(max_total / S) + count = need - 1 (below count * K, K = the segments of MAX_N bytes)
    max_total = (need - 1 - len(SIZES)) * seg
    assert max_total > 0 and need - 1 < len(SIZES) * segments(MAX_N, seg)
    first_out, run = len(SIZES), 0
    for i, k in enumerate(counts):
        run += k
        if run > need - 1:
            first_out = i
            break
    assert 0 < first_out < len(SIZES)
    c = deflate_async(ctxs[seg], bufs, aligns, 2, max_total=max_total)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res[:first_out] == want_res[:first_out] and got[:first_out] == want[:first_out]
    for i in range(len(SIZES)):
        if i >= first_out:
            assert res[i] == (0, dmx.DMX_ERR_ARG, 0), i
        assert untouched(host, c.ooffs, c.caps, i, res[i][0]), i


# 4 ------------------------------------------------------------------------------------------
def short_caps(needed):
    return [(0, 1, max(0, n - 1), n)[i % 4] for i, n in enumerate(needed)]


@pytest.mark.parametrize("seg", [32768, 16384])
def test_short_capacities_deflate(ctxs, seg):
    bufs, aligns = inputs()
    full_res, _, _ = sync_ref(ctxs, seg, 2)
    caps = short_caps([r[0] for r in full_res])
    want_res, want, want_host = deflate_sync(ctxs[seg], bufs, aligns, 2, caps=caps)
    assert any(r[1] == dmx.DMX_ERR_CAPACITY for r in want_res) and any(r[1] == dmx.DMX_OK for r in want_res)
    c = deflate_async(ctxs[seg], bufs, aligns, 2, caps=caps)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res == want_res and got == want and host == want_host
    for i, (r, full) in enumerate(zip(res, full_res)):
        assert r[0] == full[0] and r[1] == (dmx.DMX_ERR_CAPACITY if caps[i] < full[0] else dmx.DMX_OK), i
        assert untouched(host, c.ooffs, caps, i, caps[i]), i  # nothing past cap[i]


def test_short_capacities_inflate(ctx):
    bufs, _ = inputs()
    streams = sync_ref({32768: ctx}, 32768, 2)[1]
    caps = short_caps([len(b) for b in bufs])
    want_res, want, want_host = inflate_sync(ctx, streams, caps)
    c = inflate_async(ctx, streams, caps)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res == want_res and got == want and host == want_host
    for i, (r, b) in enumerate(zip(res, bufs)):
        assert r == (len(b), dmx.DMX_ERR_CAPACITY if caps[i] < len(b) else dmx.DMX_OK, dmx.BATCH_PATH), i
        assert untouched(host, c.ooffs, caps, i, caps[i]), i


# 5 ------------------------------------------------------------------------------------------
def test_64k_context(ctx):
    bufs, aligns = inputs()
    streams = sync_ref({32768: ctx}, 32768, 2)[1]
    c64 = dmx.Context(segment_bytes=65536)
    try:
        with pytest.raises(dmx.DmxError) as e:
            deflate_async(c64, bufs, aligns, 2)
        assert e.value.code == dmx.DMX_ERR_ARG
        c = inflate_async(c64, streams, [len(b) for b in bufs])
        torch.cuda.synchronize()
        res, got, _ = c.read()
        assert got == bufs
        assert res == [(len(b), dmx.DMX_OK, dmx.BATCH_PATH) for b in bufs]
    finally:
        c64.close()


# 6 ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strict_ctx():
    c = dmx.Context(rfc_strict=True)
    yield c
    c.close()


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("strict", [False, True])
def test_inflate_equals_sync_batch_on_golden_vectors(ctx, strict_ctx, strict, shift):
    c = strict_ctx if strict else ctx
    streams = [stream_of(v, GOLD) for v in VECS]
    bad = [bool(v.get("reference_reads_past_buffer") or not v["ref_ok"]) for v in VECS]
    caps = [(2 << 20) if b else v["out_len"] for v, b in zip(VECS, bad)]
    aligns = [(i + shift) % 4 for i in range(len(streams))]
    want_res, want, want_host = inflate_sync(c, streams, caps, aligns=aligns)
    assert any(r[1] != dmx.DMX_OK for r in want_res) and any(r[1] == dmx.DMX_OK for r in want_res)
    a = inflate_async(c, streams, caps, aligns=aligns, no_route=True)
    torch.cuda.synchronize()
    res, got, host = a.read()
    for v, r, w in zip(VECS, res, want_res):
        assert r == w, v["name"]
    assert got == want and host == want_host


# 7 ------------------------------------------------------------------------------------------
def test_deferred_stream(ctx):
    small = [dmx.corpus("text", 4096, offset=4096 * i) for i in range(10)]
    big = dmx.corpus("random", 1100 * 1024 + 77, offset=5)
    plain = small[:5] + [big] + small[5:]
    streams = [ctx.compress(p, 0 if p is big else 2) for p in plain]
    assert len(streams[5]) > (1 << 20)  # above the routing threshold
    caps = [len(p) for p in plain]
    c = inflate_async(ctx, streams, caps)
    torch.cuda.synchronize()
    res, got, host = c.read()
    assert res[5] == (0, dmx.DMX_BATCH_DEFERRED, 0)
    assert untouched(host, c.ooffs, caps, 5)
    for i, p in enumerate(plain):
        if i != 5:
            assert res[i] == (len(p), dmx.DMX_OK, dmx.BATCH_PATH) and got[i] == p, i
    c = inflate_async(ctx, streams, caps, no_route=True)
    torch.cuda.synchronize()
    res, got, _ = c.read()
    assert res == [(len(p), dmx.DMX_OK, dmx.BATCH_PATH) for p in plain]
    assert got == plain


# 8 ------------------------------------------------------------------------------------------
def test_chain_without_the_host(ctx):
    bufs, aligns = inputs()
    s = torch.cuda.Stream()
    t, offs = pack(bufs, aligns, 16)
    bounds = [dmx.deflate_bound(len(b)) for b in bufs]
    a = Call([t.data_ptr() + o for o in offs], [len(b) for b in bufs], bounds)
    b = Call([0] * len(bufs), [0] * len(bufs), [len(x) for x in bufs])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ctx.deflate_batch_async(*a.args(), a.count, MAX_N, 2, *a.outs(), stream=s.cuda_stream)
        sizes = a.res.view(torch.int64).view(-1, 2)[:, 0].contiguous()  # the compressed sizes, never on the host
        ctx.inflate_batch_async(a.d_out.data_ptr(), sizes.data_ptr(), b.count, max(bounds), *b.outs(),
                                stream=s.cuda_stream)
    torch.cuda.synchronize()
    res, got, host = b.read()
    assert got == bufs
    assert res == [(len(x), dmx.DMX_OK, dmx.BATCH_PATH) for x in bufs]
    for i, r in enumerate(res):
        assert untouched(host, b.ooffs, b.caps, i, r[0]), i


# 9 ------------------------------------------------------------------------------------------
@pytest.mark.skipif(not hasattr(torch.cuda, "_sleep"), reason="torch.cuda._sleep is absent")
def test_calls_do_not_wait(ctx):
    bufs, aligns = inputs()
    want_res, want, _ = sync_ref({32768: ctx}, 32768, 2)
    n = len(bufs)
    s = torch.cuda.Stream()
    ctx.batch_reserve(n, MAX_N)
    t, offs = pack(bufs, aligns, 16)
    zt, zoffs = pack(want, [i % 4 for i in range(n)], 4)
    bounds = [dmx.deflate_bound(len(x)) for x in bufs]

    def fresh():
        d = Call([t.data_ptr() + o for o in offs], [len(x) for x in bufs], bounds)
        i = Call([zt.data_ptr() + o for o in zoffs], [len(x) for x in want], [len(x) for x in bufs])
        return d, i

    def enqueue(d, i):
        ctx.deflate_batch_async(*d.args(), n, MAX_N, 2, *d.outs(), stream=s.cuda_stream)
        ctx.inflate_batch_async(*i.args(), n, max(bounds), *i.outs(), no_route=True, stream=s.cuda_stream)

    d, i = fresh()  # the warm-up of the same shape
    torch.cuda.synchronize()
    enqueue(d, i)
    torch.cuda.synchronize()
    assert d.read()[0] == want_res
    # the device cycles of ~0.2 s, from a short timed sleep (the length only has to exceed the
    # calls' enqueue time; it is not a measured quantity)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        torch.cuda._sleep(20_000_000)
        e1.record()
    torch.cuda.synchronize()
    cycles = int(20_000_000 * 0.2 * 1000 / max(e0.elapsed_time(e1), 1e-3))
    # the descriptors are written on the stream BEHIND the sleep, from pinned host memory
    d, i = fresh()
    torch.cuda.synchronize()
    pinned = [(x, x.cpu().pin_memory()) for x in (d.d_in, d.d_n, d.d_out, d.d_cap, i.d_in, i.d_n, i.d_out, i.d_cap)]
    for x, _ in pinned:
        x.zero_()
    torch.cuda.synchronize()
    es, ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        es.record()
        torch.cuda._sleep(cycles)
        ev.record()
        for x, h in pinned:
            x.copy_(h, non_blocking=True)
    t0 = time.perf_counter()
    enqueue(d, i)
    dt = time.perf_counter() - t0
    running = not ev.query()
    torch.cuda.synchronize()
    assert running, "a call waited for the stream (or read a descriptor on the host)"
    sleep_s = es.elapsed_time(ev) / 1000  # what the sleep really took
    assert dt < sleep_s / 4, (dt, sleep_s)  # the calls returned long before the sleep could end
    res, got, _ = d.read()
    assert res == want_res and got == want
    res, got, _ = i.read()
    assert got == bufs and res == [(len(x), dmx.DMX_OK, dmx.BATCH_PATH) for x in bufs]


# 10 -----------------------------------------------------------------------------------------
def test_two_streams_one_context(ctx):
    bufs, aligns = inputs()
    want_res, want, _ = sync_ref({32768: ctx}, 32768, 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    rbufs, raligns = bufs[::-1], aligns[::-1]
    t1, o1 = pack(bufs, aligns, 16)
    t2, o2 = pack(rbufs, raligns, 16)
    bounds = [dmx.deflate_bound(len(x)) for x in bufs]
    a = Call([t1.data_ptr() + o for o in o1], [len(x) for x in bufs], bounds)
    b = Call([t2.data_ptr() + o for o in o2], [len(x) for x in rbufs], bounds[::-1])
    torch.cuda.synchronize()
    ctx.deflate_batch_async(*a.args(), a.count, MAX_N, 2, *a.outs(), stream=s1.cuda_stream)
    ctx.deflate_batch_async(*b.args(), b.count, MAX_N, 2, *b.outs(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    res, got, _ = a.read()
    assert res == want_res and got == want
    res, got, _ = b.read()
    assert res == want_res[::-1] and got == want[::-1]


# 11 -----------------------------------------------------------------------------------------
def test_count_zero(ctx):
    res = new_res(1)
    torch.cuda.synchronize()
    ctx.deflate_batch_async(0, 0, 0, MAX_N, 2, 0, 0, res.data_ptr())
    ctx.inflate_batch_async(0, 0, 0, MAX_N, 0, 0, res.data_ptr())
    ctx.batch_reserve(0, MAX_N)
    torch.cuda.synchronize()
    assert res.cpu().numpy().tobytes() == bytes([POISON]) * 16
