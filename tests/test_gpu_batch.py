"""GPU: the batched API (dmx_deflate_batch_device / dmx_inflate_batch_device and their host
forms).  Batch deflate must write, per buffer, exactly the bytes of the single-buffer call;
batch inflate must give, per stream, exactly the single-stream result, errors included."""
import hashlib
import json
import os
import random
import sys
import zlib

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


def inputs():
    """The buffers of test 1: sizes x corpus kinds (fixed offsets) and their pointer alignments."""
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


def out_area(caps, gap=64):
    """A device tensor filled with FILL with one region of caps[i] + gap bytes per buffer."""
    offs, pos = [], 0
    for c in caps:
        offs.append(pos)
        pos += c + gap
    return torch.full((max(1, pos),), FILL, dtype=torch.uint8, device="cuda"), offs


def deflate_batch(ctx, bufs, aligns, level, caps=None):
    """Batch deflate through the device API; returns (results, output bytes per buffer up to
    min(bytes, cap), the whole output area, its offsets)."""
    t, offs = pack(bufs, aligns, 16)
    caps = caps if caps is not None else [dmx.deflate_bound(len(b)) for b in bufs]
    out, ooffs = out_area(caps)
    res = ctx.deflate_batch_device([t.data_ptr() + o for o in offs], [len(b) for b in bufs], level,
                                   [out.data_ptr() + o for o in ooffs], caps)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    got = [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)]
    return res, got, host, ooffs


def inflate_batch(ctx, streams, caps, aligns=None, no_route=False):
    aligns = aligns if aligns is not None else [i % 4 for i in range(len(streams))]
    t, offs = pack(streams, aligns, 4)
    out, ooffs = out_area(caps)
    res = ctx.inflate_batch_device([t.data_ptr() + o for o in offs], [len(s) for s in streams],
                                   [out.data_ptr() + o for o in ooffs], caps, no_route=no_route)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    got = [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)]
    return res, got, host, ooffs


@pytest.fixture(scope="module")
def ctx16():
    c = dmx.Context(segment_bytes=16384)
    yield c
    c.close()


@pytest.fixture(scope="module")
def single_streams(ctx):
    """ctx.compress of every test-1 buffer at every level (32 KiB segments): the reference the
    batch is compared with, computed once."""
    bufs, _ = inputs()
    return {lvl: [ctx.compress(b, lvl) for b in bufs] for lvl in range(4)}


def raw_inflate(s):
    z = zlib.decompressobj(-15)
    out = z.decompress(s)
    assert z.eof and z.unused_data == b""
    return out


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_deflate_batch_equals_single_32k(ctx, oracle, single_streams, level):
    bufs, aligns = inputs()
    res, got, _, _ = deflate_batch(ctx, bufs, aligns, level)
    for i, (b, r, g) in enumerate(zip(bufs, res, got)):
        assert r[1:] == (dmx.DMX_OK, 0), (i, r)
        assert g == single_streams[level][i], (i, len(b))
        assert oracle.inflate(g) == b, i
        assert raw_inflate(g) == b, i


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_deflate_batch_equals_single_16k(ctx16, oracle, level):
    bufs, aligns = inputs()
    res, got, _, _ = deflate_batch(ctx16, bufs, aligns, level)
    for i, (b, r, g) in enumerate(zip(bufs, res, got)):
        assert r[1:] == (dmx.DMX_OK, 0), (i, r)
        assert g == ctx16.compress(b, level), (i, len(b))
        assert oracle.inflate(g) == b, i
        assert raw_inflate(g) == b, i


def test_compress_batch_host_api(ctx, single_streams):
    bufs, _ = inputs()
    assert ctx.compress_batch(bufs, 2) == single_streams[2]
    assert ctx.compress_batch([], 2) == []


# 2 ------------------------------------------------------------------------------------------
def test_deflate_batch_more_segments_than_one_grid_round(ctx):
    rng = random.Random(20240611)
    lens = [rng.randint(100, 3000) for _ in range(5000)]
    src = dmx.corpus("text", sum(lens) // 2 + 3000, offset=4096) + dmx.corpus("mixed", sum(lens) // 2 + 3000, offset=8192)
    bufs, pos = [], 0
    for n in lens:
        bufs.append(src[pos:pos + n])
        pos += n
    res, got, _, _ = deflate_batch(ctx, bufs, [rng.choice(ALIGNS) for _ in bufs], 2)
    for i, (b, r, g) in enumerate(zip(bufs, res, got)):
        assert r[1] == dmx.DMX_OK and r[0] == len(g), (i, r)
        assert ctx.decompress(g) == b, i
    for i in rng.sample(range(len(bufs)), 50):
        assert got[i] == ctx.compress(bufs[i], 2), i


# 3 ------------------------------------------------------------------------------------------
def test_deflate_batch_capacity(ctx, single_streams):
    bufs, aligns = inputs()
    ref = single_streams[2]
    k = SIZES.index(100000)
    caps = [dmx.deflate_bound(len(b)) for b in bufs]
    caps[k] = len(ref[k]) // 2
    res, got, host, ooffs = deflate_batch(ctx, bufs, aligns, 2, caps)
    assert res[k] == (len(ref[k]), dmx.DMX_ERR_CAPACITY, 0)
    assert host[ooffs[k] + caps[k]:ooffs[k] + caps[k] + 64] == bytes([FILL]) * 64
    for i in range(len(bufs)):
        if i != k:
            assert res[i][1] == dmx.DMX_OK and got[i] == ref[i], i


# 4 ------------------------------------------------------------------------------------------
def test_deflate_batch_64k_segments_is_arg_error():
    c = dmx.Context(segment_bytes=65536)
    try:
        with pytest.raises(dmx.DmxError) as e:
            c.compress_batch([b"abc" * 100], 2)
        assert e.value.code == dmx.DMX_ERR_ARG
        d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
        with pytest.raises(dmx.DmxError) as e:
            c.deflate_batch_device([d.data_ptr()], [512], 2, [d.data_ptr() + 512], [512])
        assert e.value.code == dmx.DMX_ERR_ARG
    finally:
        c.close()


# 5 ------------------------------------------------------------------------------------------
def test_inflate_batch_golden_vectors(ctx):
    streams = [stream_of(v, GOLD) for v in VECS]
    bad = [bool(v.get("reference_reads_past_buffer") or not v["ref_ok"]) for v in VECS]
    caps = [(2 << 20) if b else v["out_len"] for v, b in zip(VECS, bad)]
    vals, res = ctx.decompress_batch(streams, caps, with_results=True)
    for v, b, out, r in zip(VECS, bad, vals, res):
        assert r[2] == dmx.BATCH_PATH, v["name"]
        if b:
            assert isinstance(out, dmx.DmxError), v["name"]
        else:
            assert not isinstance(out, dmx.DmxError), (v["name"], out)
            assert len(out) == v["out_len"] and hashlib.sha256(out).hexdigest() == v["out_sha256"], v["name"]


# 6 ------------------------------------------------------------------------------------------
def zraw(d, lvl=6, st=0):
    z = zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, st)
    return z.compress(d) + z.flush()


def test_inflate_batch_mixed_producers(ctx, oracle, single_streams):
    bufs, _ = inputs()
    streams, plain = [], []
    for lvl in range(4):  # libdmx's own streams, the 4-segment 100000-byte ones included
        streams += single_streams[lvl]
        plain += bufs
    for n in (4096, 65536, 300 * 1024):  # 300 KiB wraps the 32 KiB window ring several times
        for kind in ("text", "mixed"):
            d = dmx.corpus(kind, n, offset=31 * n)
            for lvl, st in ((1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_RLE)):
                streams.append(zraw(d, lvl, st))
                plain.append(d)
    d = dmx.corpus("mixed", 70000, offset=5)
    streams.append(zraw(d, 0))  # stored blocks
    plain.append(d)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    parts = [dmx.corpus("text", 3000 + 517 * k, offset=9000 * k) for k in range(10)]
    s = b"".join(z.compress(p) + z.flush(zlib.Z_SYNC_FLUSH) for p in parts) + z.flush()
    streams.append(s)  # ten sync-flushed blocks
    plain.append(b"".join(parts))
    res, got, _, _ = inflate_batch(ctx, streams, [len(p) for p in plain])
    for i, (s, p, r, g) in enumerate(zip(streams, plain, res, got)):
        assert r == (len(p), dmx.DMX_OK, dmx.BATCH_PATH), (i, r)
        assert g == p, i
        assert ctx.decompress(s) == g, i
        assert oracle.inflate(s) == g, i


# 7 ------------------------------------------------------------------------------------------
def test_inflate_batch_error_isolation(ctx):
    plain = [dmx.corpus(KINDS[i % 4], 3000 + 211 * i, offset=777 * i) for i in range(23)]
    streams = [zraw(p, 6) if i % 2 else ctx.compress(p, 2) for i, p in enumerate(plain)]
    caps = [len(p) for p in plain]
    streams[5] = streams[5][:-5]   # truncated
    streams[11] = b""              # empty input
    caps[17] = len(plain[17]) // 3  # too small
    res, got, host, ooffs = inflate_batch(ctx, streams, caps)
    assert res[5][1] == dmx.DMX_ERR_OVERREAD
    assert res[11][1] == dmx.DMX_ERR_OVERREAD
    assert res[17] == (len(plain[17]), dmx.DMX_ERR_CAPACITY, dmx.BATCH_PATH)
    assert got[17] == plain[17][:caps[17]]
    assert host[ooffs[17] + caps[17]:ooffs[17] + caps[17] + 64] == bytes([FILL]) * 64
    for i in range(23):
        if i not in (5, 11, 17):
            assert res[i] == (len(plain[i]), dmx.DMX_OK, dmx.BATCH_PATH) and got[i] == plain[i], i
    # the host form reports the same per stream
    vals = ctx.decompress_batch(streams, caps)
    assert [v.code for v in vals if isinstance(v, dmx.DmxError)] == [dmx.DMX_ERR_OVERREAD, dmx.DMX_ERR_OVERREAD,
                                                                      dmx.DMX_ERR_CAPACITY]
    assert all(v == p for i, (v, p) in enumerate(zip(vals, plain)) if i not in (5, 11, 17))


# 8 ------------------------------------------------------------------------------------------
def test_inflate_batch_routing(ctx):
    big = dmx.corpus("mixed", 8 << 20, offset=12345)
    small = [dmx.corpus("text", 4096, offset=4096 * i) for i in range(10)]
    plain = small[:5] + [big] + small[5:]
    streams = [ctx.compress(p, 2) for p in plain]
    assert len(streams[5]) > (1 << 20)  # above the routing threshold
    caps = [len(p) for p in plain]
    for no_route in (False, True):
        res, got, _, _ = inflate_batch(ctx, streams, caps, no_route=no_route)
        for i, (p, r, g) in enumerate(zip(plain, res, got)):
            want = 4 if (i == 5 and not no_route) else dmx.BATCH_PATH
            assert r == (len(p), dmx.DMX_OK, want), (no_route, i, r)
            assert g == p, (no_route, i)


# 9 ------------------------------------------------------------------------------------------
def test_existing_api_unchanged_after_batch_calls(ctx):
    d = dmx.corpus("text", 1 << 20, offset=99)
    fresh = dmx.Context()
    try:
        ref = fresh.compress(d, 2)
    finally:
        fresh.close()
    bufs, aligns = inputs()
    _, got, _, _ = deflate_batch(ctx, bufs, aligns, 2)
    inflate_batch(ctx, got, [len(b) for b in bufs])
    assert ctx.compress(d, 2) == ref
    assert ctx.decompress(ref) == d
