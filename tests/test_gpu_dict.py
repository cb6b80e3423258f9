"""GPU: preset dictionaries for the batched deflate and inflate (dmx_deflate_batch_dict* /
dmx_inflate_batch_dict*).  The yardstick is CPU zlib with zdict on raw streams: libdmx's streams
must decode with zlib.decompressobj(-15, zdict=d), zlib's must decode here given d."""
import random
import zlib

import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu

S = 32768
FILL = 0xA5
DICT_LENS = [1, 3, 258, 8192, 16384, 16385, 40000]
DICT_OFFS = [0, 1, 7]  # the dictionary pointer mod 16
BATCH_SIZES = [0, 1, 2, 3, 255, 4095, 16384, 32767, 32768, 32769, 65536, 65537, 100000, 98304]  # test_gpu_batch.py
KINDS = ["zeros", "random", "text", "mixed"]

HOSTS = ["gpu-node-%02d.cluster.example" % i for i in range(12)]
LEVELS = ["INFO", "WARN", "ERROR", "DEBUG"]
MSGS = ["kernel launch completed", "allocation of device buffer failed", "segment table uploaded",
        "stream synchronised", "checksum verified", "window hand-off finished"]
_records = {}


def records(seed, nbytes):
    """Deterministic JSON-ish log lines: fixed keys, seeded values."""
    have = _records.get(seed, b"")
    if len(have) < nbytes:
        r = random.Random(seed)
        out = bytearray()
        while len(out) < nbytes:
            out += ('{"timestamp":"2026-10-%02dT%02d:%02d:%02dZ","host":"%s","level":"%s","message":"%s",'
                    '"bytes":%d,"latency_us":%d}\n' % (
                        r.randrange(1, 29), r.randrange(24), r.randrange(60), r.randrange(60), r.choice(HOSTS),
                        r.choice(LEVELS), r.choice(MSGS), r.randrange(1 << 20), r.randrange(100000))).encode()
        have = _records[seed] = bytes(out)
    return have[:nbytes]


def zdeflate(data, level, zdict=None):
    z = (zlib.compressobj(level, zlib.DEFLATED, -15, zdict=zdict) if zdict is not None
         else zlib.compressobj(level, zlib.DEFLATED, -15))
    return z.compress(data) + z.flush()


def zinflate(s, zdict=None):
    z = zlib.decompressobj(-15, zdict=zdict) if zdict is not None else zlib.decompressobj(-15)
    out = z.decompress(s)
    assert z.eof and z.unused_data == b""
    return out


def pack(bufs, aligns, mod):
    """One device tensor with every buffer, buffer i at an offset that is aligns[i] modulo mod."""
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
    offs, pos = [], 0
    for c in caps:
        offs.append(pos)
        pos += c + gap
    return torch.full((max(1, pos),), FILL, dtype=torch.uint8, device="cuda"), offs


def dev_dict(d, off=0):
    """The dictionary in device memory at an address that is off modulo 16; (tensor, pointer)."""
    t, offs = pack([d], [off], 16)
    return t, t.data_ptr() + offs[0]


def deflate_dict(ctx, bufs, level, d, doff=0, aligns=None, caps=None, null_dict=False):
    aligns = aligns if aligns is not None else [(0, 1, 7, 16)[i % 4] for i in range(len(bufs))]
    t, offs = pack(bufs, aligns, 16)
    caps = caps if caps is not None else [dmx.deflate_bound(len(b)) for b in bufs]
    out, ooffs = out_area(caps)
    dt, dp = dev_dict(d, doff)
    res = ctx.deflate_batch_device([t.data_ptr() + o for o in offs], [len(b) for b in bufs], level,
                                   [out.data_ptr() + o for o in ooffs], caps,
                                   dict_ptr=0 if null_dict else dp, dict_len=len(d))
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return res, [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)]


def inflate_dict(ctx, streams, caps, d, doff=0, aligns=None, null_dict=False, no_route=False):
    aligns = aligns if aligns is not None else [i % 4 for i in range(len(streams))]
    t, offs = pack(streams, aligns, 4)
    out, ooffs = out_area(caps)
    dt, dp = dev_dict(d, doff)
    res = ctx.inflate_batch_device([t.data_ptr() + o for o in offs], [len(s) for s in streams],
                                   [out.data_ptr() + o for o in ooffs], caps, no_route=no_route,
                                   dict_ptr=0 if null_dict else dp, dict_len=len(d))
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return res, [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)], host, ooffs


def the_dict(dlen):
    return records(1, dlen)


def pages_for(dlen):
    """Test 1's pages for a dictionary of dlen bytes: every size from records and from random."""
    du = min(dlen, 16384)
    sizes = [0, 1, 3, 255, 4095, 4096, S - du - 1, S - du, S - du + 1, 32768, 65537]
    rec = records(100 + dlen % 97, 140000)
    pages = []
    for i, n in enumerate(sizes):
        pages.append(rec[1000 * i:1000 * i + n])
        pages.append(dmx.corpus("random", n, offset=7000 * i))
    return pages


_own = {}


def own_streams(ctx, level, dlen):
    """libdmx's streams of pages_for(dlen) made with the_dict(dlen) at `level` (one batch, made once)."""
    if (level, dlen) not in _own:
        doff = DICT_OFFS[DICT_LENS.index(dlen) % 3]
        _own[(level, dlen)] = deflate_dict(ctx, pages_for(dlen), level, the_dict(dlen), doff)
    return _own[(level, dlen)]


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dlen", DICT_LENS)
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_round_trip_through_zlib(ctx, level, dlen):
    d, pages = the_dict(dlen), pages_for(dlen)
    res, got = own_streams(ctx, level, dlen)
    for i, (p, r, g) in enumerate(zip(pages, res, got)):
        assert r == (len(g), dmx.DMX_OK, 0), (i, r)
        assert len(g) <= dmx.deflate_bound(len(p)), (i, len(p), len(g))
        assert zinflate(g, d) == p, (i, len(p))
    if level < 2:  # no matcher: the dictionary is ignored and the streams are the plain ones
        assert got == ctx.compress_batch(pages, level)


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3])
def test_dictionary_is_used(ctx, level):
    d = dmx.corpus("text", 16384)
    page = d[-4096:]
    bar = len(zdeflate(page, 1))
    zd = len(zdeflate(page, 1, d))
    res, got = deflate_dict(ctx, [page], level, d)
    print("level", level, "libdmx with dictionary", len(got[0]), "zlib level 1 without", bar, "with", zd)
    assert res[0][1] == dmx.DMX_OK
    assert zinflate(got[0], d) == page
    assert len(got[0]) < bar
    try:
        z = zlib.decompressobj(-15)
        wrong = z.decompress(got[0])
    except zlib.error:
        wrong = None
    assert wrong != page


# 3 ------------------------------------------------------------------------------------------
def test_saving_on_small_pages(ctx):
    """libdmx's saving 1 - bytes_with / bytes_without on 64 x 1 KiB record pages at level 2 is at
    least half of zlib level 1's on the same pages and dictionary."""
    d = the_dict(8192)
    pages = [records(100 + i, 1024) for i in range(64)]
    z_without = sum(len(zdeflate(p, 1)) for p in pages)
    z_with = sum(len(zdeflate(p, 1, d)) for p in pages)
    z_saving = 1 - z_with / z_without
    res, got = deflate_dict(ctx, pages, 2, d)
    res0, got0 = deflate_dict(ctx, pages, 2, b"")
    plain = ctx.compress_batch(pages, 2)
    for p, g in zip(pages, got):
        assert zinflate(g, d) == p
    assert got0 == plain
    without = sum(len(g) for g in plain)
    with_ = sum(r[0] for r in res)
    saving = 1 - with_ / without
    print("zlib level 1: without", z_without, "with", z_with, "saving %.3f" % z_saving)
    print("libdmx level 2: without", without, "with", with_, "saving %.3f" % saving)
    assert saving >= z_saving / 2


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_empty_dictionary_is_the_plain_call(ctx, level):
    bufs = [dmx.corpus(KINDS[i % 4], n, offset=1000 * i) for i, n in enumerate(BATCH_SIZES)]
    aligns = [(0, 1, 7, 16)[(i + i // 4) % 4] for i in range(len(bufs))]
    t, offs = pack(bufs, aligns, 16)
    caps = [dmx.deflate_bound(len(b)) for b in bufs]
    caps[BATCH_SIZES.index(100000)] = 10  # a capacity error is part of the result
    ptrs, sizes = [t.data_ptr() + o for o in offs], [len(b) for b in bufs]
    outs = []
    for kw in ({}, {"dict_ptr": 0, "dict_len": 0}, {"dict_ptr": t.data_ptr(), "dict_len": 0}):
        out, ooffs = out_area(caps)
        res = ctx.deflate_batch_device(ptrs, sizes, level, [out.data_ptr() + o for o in ooffs], caps, **kw)
        torch.cuda.synchronize()
        outs.append((res, out.cpu().numpy().tobytes()))
    assert outs[1] == outs[0] and outs[2] == outs[0]
    assert outs[0][0][BATCH_SIZES.index(100000)][1] == dmx.DMX_ERR_CAPACITY
    streams = [s for s in ctx.compress_batch(bufs, level)]
    streams[5] = streams[5][:-3]  # an error is part of the result, too
    st, soffs = pack(streams, [i % 4 for i in range(len(streams))], 4)
    icaps = [len(b) for b in bufs]
    icaps[7] = 100
    outs = []
    for kw in ({}, {"dict_ptr": 0, "dict_len": 0}, {"dict_ptr": t.data_ptr(), "dict_len": 0}):
        out, ooffs = out_area(icaps)
        res = ctx.inflate_batch_device([st.data_ptr() + o for o in soffs], [len(s) for s in streams],
                                       [out.data_ptr() + o for o in ooffs], icaps, **kw)
        torch.cuda.synchronize()
        outs.append((res, out.cpu().numpy().tobytes()))
    assert outs[1] == outs[0] and outs[2] == outs[0]
    assert outs[0][0][7][1] == dmx.DMX_ERR_CAPACITY and outs[0][0][5][1] != dmx.DMX_OK


# 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dlen", [8192, 32768, 40000])
def test_inflate_of_zlib_streams(ctx, dlen):
    d = records(1, dlen)
    pages, streams = [], []
    for i, n in enumerate([1, 2, 100, 4096, 33000, 100000]):
        for j, p in enumerate((records(200 + i, n), dmx.corpus("text", n, offset=5000 * i))):
            for lvl in (1, 6, 9):
                pages.append(p)
                streams.append(zdeflate(p, lvl, d))
    aligns = [i % 4 for i in range(len(streams))]
    res, got, _, _ = inflate_dict(ctx, streams, [len(p) for p in pages], d, DICT_OFFS[(dlen // 8192) % 3], aligns)
    for i, (p, r, g) in enumerate(zip(pages, res, got)):
        assert r == (len(p), dmx.DMX_OK, dmx.BATCH_PATH), (i, r)
        assert g == p, i


@pytest.mark.parametrize("dlen", DICT_LENS)
def test_inflate_of_own_streams(ctx, dlen):
    d, pages = the_dict(dlen), pages_for(dlen)
    for level in (0, 1, 2, 3):
        _, streams = own_streams(ctx, level, dlen)
        res, got, _, _ = inflate_dict(ctx, streams, [len(p) for p in pages], d, DICT_OFFS[(dlen + level) % 3])
        for i, (p, r, g) in enumerate(zip(pages, res, got)):
            assert r == (len(p), dmx.DMX_OK, dmx.BATCH_PATH), (level, i, r)
            assert g == p, (level, i)


# 6 ------------------------------------------------------------------------------------------
def test_window_edge(ctx):
    """Hand-built fixed-code streams whose distances touch the edges of the dictionary."""
    d = dmx.corpus("random", 32768)
    more = d + dmx.corpus("random", 7232, offset=50000)
    cases = [
        ("1bbdffdf1100", d, d[:258] + b"A", True),         # distance 32768 at position 0
        ("1bbdff1f00", more, more[-32768:][:258], True),   # the last 32768 of a longer dictionary
        ("03dae10800", d[:100], d[:3] + b"A", True),       # the dictionary's first bytes
        ("035ae20800", d[:100], b"A", False),              # distance 101: one too far, nothing copied
        ("434000", d[:100], d[98:100] * 5, True),          # an overlapping copy out of the dictionary
    ]
    for k, (hexs, dic, want, in_zlib) in enumerate(cases):
        s = bytes.fromhex(hexs)
        if in_zlib:
            assert zinflate(s, dic) == want, hexs
        for doff in DICT_OFFS:
            res, got, _, _ = inflate_dict(ctx, [s, s], [len(want) + 8, len(want) + 8], dic, doff, aligns=[0, 3])
            assert res == [(len(want), dmx.DMX_OK, dmx.BATCH_PATH)] * 2, (hexs, doff, res)
            assert got == [want, want], (hexs, doff)


# 7 ------------------------------------------------------------------------------------------
def test_errors_stay_per_buffer(ctx):
    d, other = the_dict(8192), records(2, 8192)
    plain = [records(300 + i, 2000 + 211 * i) for i in range(12)]
    streams = [zdeflate(p, 6, d) if i % 2 else None for i, p in enumerate(plain)]
    _, own = deflate_dict(ctx, [p for i, p in enumerate(plain) if i % 2 == 0], 2, d)
    for k, i in enumerate(range(0, 12, 2)):
        streams[i] = own[k]
    streams[3] = zdeflate(plain[3], 6, other)  # made with another dictionary
    streams[4] = streams[4][:-5]              # truncated
    caps = [len(p) for p in plain]
    caps[7] = len(plain[7]) // 3              # too small
    res, got, host, ooffs = inflate_dict(ctx, streams, caps, d)
    assert res[3][2] == dmx.BATCH_PATH and got[3] != plain[3]
    assert res[3][1] in (dmx.DMX_OK, dmx.DMX_ERR_DATA, dmx.DMX_ERR_CAPACITY, dmx.DMX_ERR_OVERREAD)
    assert res[4][1] == dmx.DMX_ERR_OVERREAD
    assert res[7] == (len(plain[7]), dmx.DMX_ERR_CAPACITY, dmx.BATCH_PATH)
    assert got[7] == plain[7][:caps[7]]
    for i in range(12):
        assert host[ooffs[i] + caps[i]:ooffs[i] + caps[i] + 64] == bytes([FILL]) * 64, i
        if i not in (3, 4, 7):
            assert res[i] == (len(plain[i]), dmx.DMX_OK, dmx.BATCH_PATH) and got[i] == plain[i], i
    # deflate: a short capacity is that buffer's alone, too
    pages = [records(400 + i, 3000) for i in range(4)]
    full, ref = deflate_dict(ctx, pages, 2, d)
    caps = [dmx.deflate_bound(3000)] * 4
    caps[2] = full[2][0] // 2
    res, got = deflate_dict(ctx, pages, 2, d, caps=caps)
    assert res[2] == (full[2][0], dmx.DMX_ERR_CAPACITY, 0)
    assert [g for i, g in enumerate(got) if i != 2] == [g for i, g in enumerate(ref) if i != 2]
    # a null dictionary of non-zero length is an argument error of the call
    dt = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for call in (lambda: ctx.deflate_batch_device([dt.data_ptr()], [100], 2, [dt.data_ptr() + 2048], [2048],
                                                  dict_ptr=0, dict_len=1),
                 lambda: ctx.inflate_batch_device([dt.data_ptr()], [100], [dt.data_ptr() + 2048], [2048],
                                                  dict_ptr=0, dict_len=1)):
        with pytest.raises(dmx.DmxError) as e:
            call()
        assert e.value.code == dmx.DMX_ERR_ARG


# 8 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
def test_no_routing_with_a_dictionary(ctx, level):
    d = the_dict(8192)
    big = dmx.corpus("random", 1200 * 1024, offset=777)
    small = [records(500 + i, 4096) for i in range(6)]
    plain = small[:3] + [big] + small[3:]
    res, streams = deflate_dict(ctx, plain, level, d)
    assert all(r[1] == dmx.DMX_OK for r in res)
    assert len(streams[3]) > (1 << 20)  # above the plain call's routing threshold
    for no_route in (False, True):
        res, got, _, _ = inflate_dict(ctx, streams, [len(p) for p in plain], d, no_route=no_route)
        for i, (p, r, g) in enumerate(zip(plain, res, got)):
            assert r == (len(p), dmx.DMX_OK, dmx.BATCH_PATH), (no_route, i, r)
            assert g == p, (no_route, i)


# 9 ------------------------------------------------------------------------------------------
def test_context_sizes(ctx):
    d = the_dict(8192)
    pages = [records(600 + i, 5000) for i in range(3)]
    _, streams = deflate_dict(ctx, pages, 2, d)
    for seg in (16384, 65536):
        c = dmx.Context(segment_bytes=seg)
        try:
            for level in (0, 2):
                with pytest.raises(dmx.DmxError) as e:
                    deflate_dict(c, pages, level, d)
                assert e.value.code == dmx.DMX_ERR_ARG
                with pytest.raises(dmx.DmxError) as e:
                    c.compress_batch(pages, level, zdict=d)
                assert e.value.code == dmx.DMX_ERR_ARG
            res, got, _, _ = inflate_dict(c, streams, [len(p) for p in pages], d)
            assert res == [(len(p), dmx.DMX_OK, dmx.BATCH_PATH) for p in pages]
            assert got == pages
        finally:
            c.close()


# 10 -----------------------------------------------------------------------------------------
def test_host_forms(ctx):
    d = the_dict(8192)
    pages = [records(700 + i, 100 + 97 * i) for i in range(32)]
    for level in (1, 2, 3):
        streams = ctx.compress_batch(pages, level, zdict=d)
        for p, s in zip(pages, streams):
            assert zinflate(s, d) == p
        assert ctx.decompress_batch(streams, [len(p) for p in pages], zdict=d) == pages
    assert sum(len(s) for s in ctx.compress_batch(pages, 2, zdict=d)) < sum(len(s) for s in ctx.compress_batch(pages, 2))
    assert ctx.compress_batch(pages, 2, zdict=b"") == ctx.compress_batch(pages, 2)
    vals, res = ctx.decompress_batch([zdeflate(p, 6, d) for p in pages], [len(p) for p in pages], zdict=d,
                                     with_results=True)
    assert vals == pages and all(r[2] == dmx.BATCH_PATH for r in res)
