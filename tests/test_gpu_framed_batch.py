"""GPU: the framed batch calls (dmx_deflate_batch_framed* / dmx_inflate_batch_framed*: zlib, gzip
and BGZF around the batched API, checksums of all buffers in one launch) and the BGZF codec
(dmx_deflate_bgzf / dmx_inflate_bgzf).

Python's zlib and gzip are the references; for "zlib" and "gzip" the framed batch must also equal
the single-buffer container calls byte for byte and status for status.  Everything is byte
equality or an exact status."""
import gzip
import struct
import zlib

import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 4095, 16383, 16384, 16385, 32767, 32768, 32769, 65280, 65535, 65537,
         100003, (3 << 20) + 5]
KINDS = ["text", "mixed", "zeros", "random"]
FILL = 0xA5
BGZF_MAX = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEAD = {"zlib": 2, "gzip": 10, "bgzf": 18}
TAIL = {"zlib": 4, "gzip": 8, "bgzf": 8}

_cache = {}


def buffers():
    """SIZES x KINDS, computed once."""
    if "bufs" not in _cache:
        _cache["bufs"] = [dmx.corpus(k, n, offset=977 * i + 13 * j) for i, n in enumerate(SIZES)
                          for j, k in enumerate(KINDS)]
    return _cache["bufs"]


def singles(ctx, what, level):
    """The single-buffer call's output for every buffer, computed once per (call, level)."""
    key = (what, level)
    if key not in _cache:
        fn = {"zlib": ctx.compress_zlib, "gzip": ctx.compress_gzip, "raw": ctx.compress}[what]
        _cache[key] = [fn(b, level) if what != "raw" or len(b) <= BGZF_MAX else None for b in buffers()]
    return _cache[key]


def single_inflate(ctx, fmt, s, verify=True):
    """(status, bytes or None) of inflate_zlib / inflate_gzip for one buffer alone."""
    try:
        d = (ctx.inflate_zlib if fmt == "zlib" else ctx.inflate_gzip)(s, verify=verify)
        return dmx.DMX_OK, d
    except dmx.DmxError as e:
        return e.code, None


def pack(bufs, mod_offsets=(0, 1, 7, 13), fill=0xEE, gap=0):
    """One device tensor with every buffer at an offset that is mod_offsets[i % 4] modulo 16, as
    close to its predecessor as that allows (+ gap); the bytes between buffers are `fill`."""
    offs, pos = [], 0
    for i, b in enumerate(bufs):
        pos += (mod_offsets[i % len(mod_offsets)] - pos) % 16
        offs.append(pos)
        pos += len(b) + gap
    host = bytearray([fill]) * (pos + 32)
    for b, o in zip(bufs, offs):
        host[o:o + len(b)] = b
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, offs


def out_area(caps, gap=0):
    """Outputs packed like the inputs (gap more bytes after each), pre-filled with FILL."""
    return pack([bytes([FILL]) * c for c in caps], fill=FILL, gap=gap)


def check_fill(host, offs, caps, used, total):
    """Every output byte outside [offs[i], offs[i] + used[i]) is still FILL."""
    pos = 0
    for o, u in zip(offs, used):
        assert host[pos:o] == bytes([FILL]) * (o - pos), ("before", o)
        pos = o + u
    assert host[pos:total] == bytes([FILL]) * (total - pos)


def deflate_dev(ctx, bufs, level, fmt, caps=None, gap=0):
    t, offs = pack(bufs)
    caps = caps if caps is not None else [dmx.lib().dmx_batch_framed_bound(dmx.FRAME[fmt], len(b)) for b in bufs]
    out, ooffs = out_area(caps, gap)
    res = ctx.deflate_batch_framed_device([t.data_ptr() + o for o in offs], [len(b) for b in bufs], level,
                                          [out.data_ptr() + o for o in ooffs], caps, format=fmt)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return res, host, ooffs, caps


def inflate_dev(ctx, streams, caps, fmt, verify=True, no_route=False):
    t, offs = pack(streams)
    out, ooffs = out_area(caps)
    res = ctx.inflate_batch_framed_device([t.data_ptr() + o for o in offs], [len(s) for s in streams],
                                          [out.data_ptr() + o for o in ooffs], caps, format=fmt, verify=verify,
                                          no_route=no_route)
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    got = [host[o:o + min(r[0], c)] for o, r, c in zip(ooffs, res, caps)]
    return res, got, host, ooffs


def bgzf_member(d, level=6, before=b""):
    """A BGZF member built by hand around zlib's raw stream."""
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = z.compress(d) + z.flush()
    extra = before + b"BC\x02\x00" + struct.pack("<H", 12 + len(before) + 6 + len(raw) + 8 - 1)
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(extra)) + extra + raw +
            struct.pack("<II", zlib.crc32(d), len(d) & 0xFFFFFFFF))


def bgzf_split(f):
    """The members of a BGZF file, by BSIZE."""
    out, o = [], 0
    while o < len(f):
        assert f[o:o + 4] == b"\x1f\x8b\x08\x04" and f[o + 12:o + 16] == b"BC\x02\x00", o
        size = struct.unpack_from("<H", f, o + 16)[0] + 1
        out.append(f[o:o + size])
        o += size
    assert o == len(f)
    return out


@pytest.fixture(scope="module")
def ctx16():
    c = dmx.Context(segment_bytes=16384)
    yield c
    c.close()


# sizes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_deflate_framed_equals_single(ctx, fmt, level):
    bufs = buffers()
    got = ctx.compress_batch_framed(bufs, level, fmt)
    want = singles(ctx, fmt, level)
    for i, (b, g, w) in enumerate(zip(bufs, got, want)):
        assert g == w, (i, len(b))
    if level == 2:  # the references themselves, once
        for b, g in zip(bufs, got):
            assert (zlib.decompress(g) if fmt == "zlib" else gzip.decompress(g)) == b


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_deflate_framed_bgzf_members(ctx, level):
    bufs = buffers()
    caps = [dmx.lib().dmx_batch_framed_bound(dmx.DMX_FRAME_BGZF, len(b)) for b in bufs]
    outs, res = ctx._batch_host("dmx_deflate_batch_framed", bufs, caps, mid=(level, dmx.DMX_FRAME_BGZF))
    raws = singles(ctx, "raw", level)
    xfl = {0: 4, 1: 4, 2: 0, 3: 2}[level]
    for i, (b, o, r, raw) in enumerate(zip(bufs, outs, res, raws)):
        if len(b) > BGZF_MAX:  # only that buffer is refused
            assert (r.status, r.bytes) == (dmx.DMX_ERR_ARG, 0), (i, len(b))
            continue
        assert r.status == dmx.DMX_OK and r.path == 0, (i, r.status)
        m = o.raw[:r.bytes]
        assert m[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, xfl, 255, 6, 0, 0x42, 0x43, 2, 0]), i
        assert struct.unpack_from("<H", m, 16)[0] + 1 == len(m) <= 65536, i
        assert m[18:-8] == raw, i
        assert m[-8:] == struct.pack("<II", zlib.crc32(b), len(b)), i
        assert gzip.decompress(m) == b, i


def test_out_of_range_level_behaves_like_1(ctx):
    bufs = [b for b in buffers() if len(b) <= 20000]
    for fmt in ("zlib", "gzip"):
        for level in (-1, 4, 9):
            assert ctx.compress_batch_framed(bufs, level, fmt) == ctx.compress_batch_framed(bufs, 1, fmt)
        assert ctx.compress_batch_framed(bufs[:6], 7, fmt) == \
            [(ctx.compress_zlib if fmt == "zlib" else ctx.compress_gzip)(b, 7) for b in bufs[:6]]


@pytest.mark.parametrize("fmt", ["zlib", "gzip", "bgzf"])
def test_inflate_framed_own_streams(ctx, fmt):
    bufs = [b for b in buffers() if fmt != "bgzf" or len(b) <= BGZF_MAX]
    comp = ctx.compress_batch_framed(bufs, 2, fmt)
    vals, res = ctx.decompress_batch_framed(comp, [len(b) for b in bufs], fmt, with_results=True)
    for i, (b, v, r) in enumerate(zip(bufs, vals, res)):
        assert r[:2] == (len(b), dmx.DMX_OK), (i, r)
        assert v == b, i


# foreign streams in ----------------------------------------------------------------------------
def test_foreign_streams_decode_verified(ctx):
    datas = [dmx.corpus("text", 50000), dmx.corpus("mixed", 70001, offset=5), dmx.corpus("zeros", 4096),
             dmx.corpus("random", 3000), b"", b"a"]
    zs, gs, ds = [], [], []
    for lv in (1, 6, 9):
        for d in datas:
            zs.append(zlib.compress(d, lv))
            gs.append(gzip.compress(d, lv))
            ds.append(d)
    # hand-built gzip headers, every combination of FEXTRA | FNAME | FCOMMENT | FHCRC
    hs, hd = [], []
    for k in range(16):
        flg = (4 if k & 1 else 0) | (8 if k & 2 else 0) | (16 if k & 4 else 0) | (2 if k & 8 else 0)
        d = dmx.corpus("text", 3000 + 321 * k, offset=k)
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        hdr = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3])
        hdr += b"\x03\x00abc" if flg & 4 else b""
        hdr += b"name.txt\x00" if flg & 8 else b""
        hdr += b"a comment\x00" if flg & 16 else b""
        hdr += (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little") if flg & 2 else b""
        g = hdr + z.compress(d) + z.flush() + struct.pack("<II", zlib.crc32(d), len(d))
        assert gzip.decompress(g) == d
        hs.append(g)
        hd.append(d)
    bd = [dmx.corpus("text", n, offset=n) for n in (0, 1, 777, 65280)] + [dmx.corpus("random", 60000)]
    bs = [bgzf_member(d) for d in bd[:4]] + [bgzf_member(bd[4], before=b"XY\x03\x00abc")]
    for m, d in zip(bs, bd):
        assert gzip.decompress(m) == d
    for fmt, streams, want in (("zlib", zs, ds), ("gzip", gs + hs + bs, ds + hd + bd), ("bgzf", bs, bd)):
        vals, res = ctx.decompress_batch_framed(streams, [len(d) for d in want], fmt, verify=True, with_results=True)
        for i, (d, v, r) in enumerate(zip(want, vals, res)):
            assert r == (len(d), dmx.DMX_OK, dmx.BATCH_PATH), (fmt, i, r)
            assert v == d, (fmt, i)
    # BGZF additionally requires the BC subfield with BSIZE + 1 == n
    vals = ctx.decompress_batch_framed(gs[:3] + [bs[2] + b"\x00", bs[2]], [70001] * 5, "bgzf")
    assert [v.code for v in vals[:4]] == [dmx.DMX_ERR_DATA] * 4 and vals[4] == bd[2]


# device form, neighbours -----------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["zlib", "gzip", "bgzf"])
def test_device_form_misaligned_neighbours(ctx, fmt):
    sizes = [0, 1, 2, 15, 16, 17, 63, 64, 65, 4095, 16383, 16384, 16385, 32769, 65280, 100003, 3, 31, 33, 49153]
    bufs = [dmx.corpus(KINDS[i % 4], n, offset=31 * i) for i, n in enumerate(sizes) if fmt != "bgzf" or n <= BGZF_MAX]
    res, host, ooffs, caps = deflate_dev(ctx, bufs, 2, fmt)
    comp = []
    for i, (b, r, o) in enumerate(zip(bufs, res, ooffs)):
        assert r[1:] == (dmx.DMX_OK, 0), (i, r)
        comp.append(host[o:o + r[0]])
        if fmt == "zlib":
            assert comp[-1] == ctx.compress_zlib(b, 2) and zlib.decompress(comp[-1]) == b, i
        elif fmt == "gzip":
            assert comp[-1] == ctx.compress_gzip(b, 2) and gzip.decompress(comp[-1]) == b, i
        else:
            assert gzip.decompress(comp[-1]) == b and struct.unpack_from("<H", comp[-1], 16)[0] + 1 == r[0], i
    check_fill(host, ooffs, caps, [r[0] for r in res], len(host))
    # inflate: outputs of exactly the decoded size, back to back at odd alignments
    caps = [len(b) for b in bufs]
    res, got, host, ooffs = inflate_dev(ctx, comp, caps, fmt)
    for i, (b, r, g) in enumerate(zip(bufs, res, got)):
        assert r == (len(b), dmx.DMX_OK, dmx.BATCH_PATH), (i, r)
        assert g == b, i
    check_fill(host, ooffs, caps, caps, len(host))


# isolation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["zlib", "gzip"])
def test_isolation_in_a_batch_of_24(ctx, fmt):
    datas = [dmx.corpus(KINDS[i % 2], 1500 + 1371 * i, offset=i) for i in range(24)]
    streams = [bytearray(zlib.compress(d, 6) if fmt == "zlib" else gzip.compress(d, 6)) for d in datas]
    caps = [len(d) for d in datas]
    gz = fmt == "gzip"
    streams[3][-5 if gz else -1] ^= 0x10                  # a trailer bit: CRC-32 / Adler-32
    streams[7][-1 if gz else -4] ^= 0x01                  # gzip: ISIZE; zlib: another Adler-32 byte
    streams[11][1 if gz else 0] ^= 0x04                   # bad magic / CM
    if gz:
        streams[13][2] = 9                                # CM
    else:
        streams[13][1] = 0xBB                             # 78 bb: FDICT with a valid FCHECK
    streams[17] = streams[17][:17 if gz else 5]           # shorter than the smallest container
    caps[21] = len(datas[21]) - 100                       # a short output
    streams = [bytes(s) for s in streams]
    want = {3: dmx.DMX_ERR_CHECKSUM, 7: dmx.DMX_ERR_CHECKSUM, 11: dmx.DMX_ERR_DATA, 13: dmx.DMX_ERR_DATA,
            17: dmx.DMX_ERR_OVERREAD, 21: dmx.DMX_ERR_CAPACITY}
    for verify in (True, False):
        res, got, host, ooffs = inflate_dev(ctx, streams, caps, fmt, verify=verify)
        for i, (d, r, g) in enumerate(zip(datas, res, got)):
            st, alone = single_inflate(ctx, fmt, streams[i], verify)
            if i == 21:  # the single call has no capacity: the batch's meaning holds
                assert (st, alone) == (dmx.DMX_OK, d)
                assert r[:2] == (len(d), dmx.DMX_ERR_CAPACITY) and g == d[:caps[i]], (i, r)
                continue
            exp = want.get(i, dmx.DMX_OK) if verify or i not in (3, 7) else dmx.DMX_OK
            assert st == exp and r[1] == exp, (i, verify, st, r)
            if exp == dmx.DMX_OK:
                assert r[0] == len(d) and g == d and alone == d, (i, r)
            elif exp == dmx.DMX_ERR_CHECKSUM:  # the data is there all the same
                assert r[0] == len(d) and g == d, (i, r)
            else:
                assert r[0] == 0, (i, r)
        used = [min(r[0], c) for r, c in zip(res, caps)]
        check_fill(host, ooffs, caps, used, len(host))
    # the host form hands the data out with DMX_ERR_CHECKSUM's neighbours untouched
    vals = ctx.decompress_batch_framed(streams, caps, fmt)
    for i, (d, v) in enumerate(zip(datas, vals)):
        if i in want:
            assert isinstance(v, dmx.DmxError) and v.code == want[i], i
        else:
            assert v == d, i


# routing ---------------------------------------------------------------------------------------
def test_routed_stream_is_framed_and_verified_alike(ctx):
    big = dmx.corpus("random", (1 << 20) + (1 << 20) // 5)
    datas = [dmx.corpus("text", 2000 + 97 * i, offset=i) for i in range(5)]
    datas.insert(2, big)
    streams = [ctx.compress_gzip(d, 0) if d is big else gzip.compress(d, 6) for d in datas]
    assert len(streams[2]) > (1 << 20)
    caps = [len(d) for d in datas]
    results = {}
    for no_route in (False, True):
        res, got, _, _ = inflate_dev(ctx, streams, caps, "gzip", no_route=no_route)
        for i, (d, r, g) in enumerate(zip(datas, res, got)):
            assert r[:2] == (len(d), dmx.DMX_OK) and g == d, (i, r)
            assert (r[2] != dmx.BATCH_PATH) == (i == 2 and not no_route), (i, r)
        bad = list(streams)
        b = bytearray(bad[2])
        b[-6] ^= 0x40  # a CRC byte
        bad[2] = bytes(b)
        res, got, _, _ = inflate_dev(ctx, bad, caps, "gzip", no_route=no_route)
        for i, (d, r, g) in enumerate(zip(datas, res, got)):
            assert r[:2] == (len(d), dmx.DMX_ERR_CHECKSUM if i == 2 else dmx.DMX_OK) and g == d, (i, r)
        results[no_route] = [r[:2] for r in res]
        res, _, _, _ = inflate_dev(ctx, bad, caps, "gzip", verify=False, no_route=no_route)
        assert [r[1] for r in res] == [dmx.DMX_OK] * 6
    assert results[False] == results[True]
    # a routed stream with a header error, and one whose output is short
    bad = list(streams)
    bad[2] = b"\x1f\x8c" + streams[2][2:]
    res, _, _, _ = inflate_dev(ctx, bad, caps, "gzip")
    assert [r[:2] for r in res] == [(len(d), dmx.DMX_OK) if i != 2 else (0, dmx.DMX_ERR_DATA) for i, d in enumerate(datas)]
    caps[2] -= 1000
    res, got, _, _ = inflate_dev(ctx, streams, caps, "gzip")
    assert res[2][:2] == (len(big), dmx.DMX_ERR_CAPACITY)
    assert all(r[:2] == (len(d), dmx.DMX_OK) for i, (d, r) in enumerate(zip(datas, res)) if i != 2)


# deflate capacity ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["zlib", "gzip", "bgzf"])
def test_deflate_capacity(ctx, fmt):
    bufs = [dmx.corpus(KINDS[i % 4], n, offset=i) for i, n in enumerate([0, 1, 500, 40000, 65280, 20])]
    full, _, _, _ = deflate_dev(ctx, bufs, 2, fmt)
    sizes = [r[0] for r in full]
    caps = list(sizes)
    for i in (0, 2, 3):
        caps[i] -= 1  # one byte short
    caps[5] = HEAD[fmt] + TAIL[fmt] - 1  # not even the frame
    res, host, ooffs, _ = deflate_dev(ctx, bufs, 2, fmt, caps, gap=1)
    for i, (r, o, c, s) in enumerate(zip(res, ooffs, caps, sizes)):
        short = i in (0, 2, 3, 5)
        assert r[:2] == (s, dmx.DMX_ERR_CAPACITY if short else dmx.DMX_OK), (i, r)
        assert host[o + c] == FILL, i  # the byte at d_out[i] + cap[i]
        if not short:
            assert gzip.decompress(host[o:o + s]) == bufs[i] if fmt != "zlib" else zlib.decompress(host[o:o + s]) == bufs[i]
    # cap 0 with a null output is accepted
    t, offs = pack(bufs)
    res = ctx.deflate_batch_framed_device([t.data_ptr() + o for o in offs], [len(b) for b in bufs], 2,
                                          [0] * len(bufs), [0] * len(bufs), format=fmt)
    assert [r[:2] for r in res] == [(s, dmx.DMX_ERR_CAPACITY) for s in sizes]


# BGZF deflate limits ---------------------------------------------------------------------------
def test_bgzf_deflate_limits(ctx, ctx16):
    bufs = [dmx.corpus("text", n) for n in (65280, 65281, 100, 200000, 0)]
    for c in (ctx, ctx16):
        caps = [dmx.lib().dmx_batch_framed_bound(dmx.DMX_FRAME_BGZF, len(b)) for b in bufs]
        outs, res = c._batch_host("dmx_deflate_batch_framed", bufs, caps, mid=(2, dmx.DMX_FRAME_BGZF))
        assert [r.status for r in res] == [dmx.DMX_OK, dmx.DMX_ERR_ARG, dmx.DMX_OK, dmx.DMX_ERR_ARG, dmx.DMX_OK]
        for b, o, r in zip(bufs, outs, res):
            if r.status == dmx.DMX_OK:
                assert gzip.decompress(o.raw[:r.bytes]) == b
        with pytest.raises(dmx.DmxError) as e:
            c.compress_batch_framed(bufs, 2, "bgzf")
        assert e.value.code == dmx.DMX_ERR_ARG
    c64 = dmx.Context(segment_bytes=65536)
    try:
        for fmt in ("zlib", "gzip", "bgzf"):
            with pytest.raises(dmx.DmxError) as e:
                c64.compress_batch_framed(bufs[2:3], 2, fmt)
            assert e.value.code == dmx.DMX_ERR_ARG
        # inflate takes any stream with any context
        assert c64.decompress_batch_framed([gzip.compress(bufs[2])], [100], "gzip") == [bufs[2]]
        with pytest.raises(dmx.DmxError) as e:
            c64.compress_bgzf(bufs[2])
        assert e.value.code == dmx.DMX_ERR_ARG
    finally:
        c64.close()


# BGZF codec ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65280, 65281, (1 << 20) + 3])
def test_bgzf_codec_roundtrip(ctx, n):
    d = dmx.corpus("text", n, offset=n % 1000)
    f = ctx.compress_bgzf(d)
    assert gzip.decompress(f) == d
    assert f[-28:] == EOF_BLOCK
    members = bgzf_split(f)
    assert len(members) == -(-n // BGZF_MAX) + 1 and all(len(m) <= 65536 for m in members)
    assert b"".join(gzip.decompress(m) for m in members[:-1]) == d
    assert all(len(gzip.decompress(m)) == BGZF_MAX for m in members[:-2])
    assert ctx.decompress_bgzf(f) == d
    assert ctx.decompress_bgzf(f, verify=False) == d
    assert len(f) <= dmx.lib().dmx_bgzf_bound(n)


def test_bgzf_codec_foreign_files_and_errors(ctx):
    parts = [dmx.corpus("text", 65280), dmx.corpus("mixed", 30000, offset=9), b"", dmx.corpus("random", 1234), b"x"]
    members = [bgzf_member(p) for p in parts]
    whole = b"".join(parts)
    for tail in (EOF_BLOCK, b""):  # the EOF block included or omitted
        f = b"".join(members) + tail
        assert gzip.decompress(f) == whole
        assert ctx.decompress_bgzf(f) == whole
        assert ctx.decompress_bgzf(f, verify=False) == whole
    assert ctx.decompress_bgzf(EOF_BLOCK) == b"" and ctx.decompress_bgzf(b"") == b""
    f = b"".join(members) + EOF_BLOCK

    def code(data, verify=True):
        with pytest.raises(dmx.DmxError) as e:
            ctx.decompress_bgzf(data, verify=verify)
        return e.value.code

    assert code(f[:-5]) == dmx.DMX_ERR_OVERREAD                          # a cut chain
    assert code(f[:len(members[0]) + 40]) == dmx.DMX_ERR_OVERREAD
    assert code(gzip.compress(parts[1])) == dmx.DMX_ERR_DATA            # a plain gzip member
    assert code(members[0] + b"\x1f\x8c" + members[1][2:]) == dmx.DMX_ERR_DATA
    for delta in (1, -1):  # a member whose ISIZE lies: the layout rests on it
        m = bytearray(members[1])
        m[-4:] = struct.pack("<I", len(parts[1]) + delta)
        lie = members[0] + bytes(m) + members[3]
        assert code(lie, True) == dmx.DMX_ERR_CHECKSUM and code(lie, False) == dmx.DMX_ERR_CHECKSUM
    m = bytearray(members[1])
    m[-7] ^= 0x20  # a CRC byte
    bad = members[0] + bytes(m) + members[3] + EOF_BLOCK
    assert code(bad, True) == dmx.DMX_ERR_CHECKSUM
    assert ctx.decompress_bgzf(bad, verify=False) == parts[0] + parts[1] + parts[3]


# count == 0, and the plain batch after framed calls ----------------------------------------------
def test_count_zero_and_plain_batch_unchanged(ctx):
    for fmt in ("zlib", "gzip", "bgzf"):
        assert ctx.compress_batch_framed([], 2, fmt) == []
        assert ctx.decompress_batch_framed([], [], fmt) == []
        assert ctx.deflate_batch_framed_device([], [], 2, [], [], format=fmt) == []
        assert ctx.inflate_batch_framed_device([], [], [], [], format=fmt) == []
    bufs = [dmx.corpus(KINDS[i % 4], 3000 + 4001 * i, offset=i) for i in range(8)]
    before = ctx.compress_batch(bufs, 2)
    framed = ctx.compress_batch_framed(bufs, 2, "gzip")
    assert [g[10:-8] for g in framed] == before
    assert ctx.decompress_batch_framed(framed, [len(b) for b in bufs], "gzip") == bufs
    # unknown formats and flags
    import ctypes
    k, a_in, a_n, a_out, a_cap, res = ctx._batch_arrays([0], [0], [0], [0])
    lib = dmx.lib()
    for fmt in (0, 4):
        assert lib.dmx_deflate_batch_framed_device(ctx.h, a_in, a_n, 1, 2, fmt, a_out, a_cap, res, None) == dmx.DMX_ERR_ARG
        assert lib.dmx_inflate_batch_framed_device(ctx.h, a_in, a_n, 1, fmt, a_out, a_cap, res, 0, None) == dmx.DMX_ERR_ARG
        assert lib.dmx_deflate_batch_framed(ctx.h, a_in, a_n, 1, 2, fmt, a_out, a_cap, res) == dmx.DMX_ERR_ARG
        assert lib.dmx_inflate_batch_framed(ctx.h, a_in, a_n, 1, fmt, a_out, a_cap, res, 0) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_batch_framed_device(ctx.h, a_in, a_n, 1, 2, a_out, a_cap, res, 4, None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_batch_framed(ctx.h, a_in, a_n, 1, 2, a_out, a_cap, res, 8) == dmx.DMX_ERR_ARG
    p, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    assert lib.dmx_inflate_bgzf(ctx.h, EOF_BLOCK, 28, 2, ctypes.byref(p), ctypes.byref(ln)) == dmx.DMX_ERR_ARG
    # the plain batch still rejects every flag but DMX_BATCH_NO_ROUTE, and gives the same bytes
    assert lib.dmx_inflate_batch(ctx.h, a_in, a_n, 1, a_out, a_cap, res, dmx.DMX_BATCH_VERIFY) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_batch_device(ctx.h, a_in, a_n, 1, a_out, a_cap, res, dmx.DMX_BATCH_VERIFY,
                                        None) == dmx.DMX_ERR_ARG
    assert ctx.compress_batch(bufs, 2) == before
    assert ctx.decompress_batch(before, [len(b) for b in bufs]) == bufs
