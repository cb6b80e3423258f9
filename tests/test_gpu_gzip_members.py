"""GPU: multi-member gzip files -- dmx_inflate_gzip_members_device, dmx_inflate_gzip_members
(csrc/gzip_members.hip, csrc/gzip_members.cpp).

The oracle is Python: gzip.decompress gives the bytes, a zlib.decompressobj(31) / unused_data walk
gives where each member starts.  Files are built with gzip / zlib, by hand around stored blocks
where an exact stream size matters, and with ctx.compress_gzip.  The file and the output area sit
at offsets 0, 1 and 7 modulo 16 inside tensors filled with a canary byte, which is checked after
every call."""
import ctypes
import gzip
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
T = 1 << 20     # the measuring limit: the batch calls' routing threshold
TILE = 4096     # the candidate scan's tile
MODS = ((0, 0), (1, 7), (7, 1))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streams")

_cache = {}


# ---- files -----------------------------------------------------------------------------------------
def gz(d, level=6, name=None, extra=None, comment=None, hcrc=False, raw=None):
    """One gzip member built by hand (raw: the DEFLATE stream to put inside instead of zlib's)."""
    if raw is None:
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = z.compress(d) + z.flush()
    flg = (2 if hcrc else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0) | \
        (16 if comment is not None else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\x00\x00\x00\x00\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw + struct.pack("<II", zlib.crc32(d), len(d) & 0xFFFFFFFF)


def stored_raw(d, block=65535):
    """A raw stream of stored blocks of `block` bytes: 5 bytes per block on top of the payload."""
    out, o = [], 0
    while True:
        part = d[o:o + block]
        o += len(part)
        out.append(bytes([1 if o >= len(d) else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part)
        if o >= len(d):
            return b"".join(out)


def text(n, offset=0):
    key = ("text", n, offset)
    if key not in _cache:
        _cache[key] = dmx.corpus("text", n, offset=offset)
    return _cache[key]


def walk(f):
    """The serial walk of a well-formed file with zlib -> the (members + 1, 2) index."""
    mv, rows, o, u = memoryview(f), [], 0, 0
    while o < len(f):
        if f[o] == 0 and o:
            o += 1
            continue
        d, p, got = zlib.decompressobj(31), o, 0
        while not d.eof:
            assert p < len(f), "truncated"
            chunk = mv[p:p + 65536]
            got += len(d.decompress(chunk))
            p += len(chunk)
        rows.append((o, u))
        u += got
        o = p - len(d.unused_data)
    return np.array(rows + [(len(f), u)], dtype=np.uint64).reshape(-1, 2)


# ---- device plumbing (the canary pattern of tests/test_gpu_bgzf_device.py) ---------------------------
def dev(data, mod=0):
    off = PAD + mod
    host = bytearray([FILL]) * (off + len(data) + PAD)
    host[off:off + len(data)] = data
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, off


def area(n, mod=0):
    return dev(bytes([FILL]) * n, mod)


def host_of(t):
    return t.cpu().numpy().tobytes()


def canaries_ok(h, off, used):
    return h[:off] == bytes([FILL]) * off and h[off + used:] == bytes([FILL]) * (len(h) - off - used)


class Result:
    pass


def run(ctx, f, verify=True, mod=1, omod=7, cap=None, want=None):
    """One call -> status, bytes (DMX_OK) or the error, members, index, and the canary verdicts."""
    if cap is None:
        cap = len(want) if want is not None else len(gzip.decompress(f))
    t, off = dev(f, mod)
    before = host_of(t)
    out, ooff = area(cap, omod)
    r = Result()
    try:
        n, r.members, r.index = ctx.inflate_gzip_members_device(t.data_ptr() + off, len(f), out.data_ptr() + ooff, cap,
                                                                verify=verify, want_index=True)
        r.status, r.error = dmx.DMX_OK, None
    except dmx.DmxError as e:
        n, r.members, r.index, r.status, r.error = 0, None, None, e.code, e
    torch.cuda.synchronize()
    h = host_of(out)
    r.bytes = h[ooff:ooff + n]
    r.inside = h[ooff:ooff + cap]
    r.canaries = canaries_ok(h, ooff, cap) and host_of(t) == before  # nothing outside cap; the input only read
    return r


def check_ok(ctx, f, want=None, mods=MODS, verify=True, layout=None):
    """layout: a file with the same member layout that zlib accepts, where f's trailers are wrong"""
    want = gzip.decompress(f) if want is None else want
    idx = walk(f if layout is None else layout)
    for mod, omod in mods:
        r = run(ctx, f, verify=verify, mod=mod, omod=omod, want=want)
        assert r.status == dmx.DMX_OK, (mod, omod, r.status)
        assert r.bytes == want, (mod, omod)
        assert r.members == idx.shape[0] - 1, (mod, omod, r.members)
        assert np.array_equal(r.index, idx), (mod, omod)
        assert r.canaries, (mod, omod)
    return idx


def check_status(ctx, f, status, cap=4096, mods=MODS, verify=True):
    for mod, omod in mods:
        r = run(ctx, f, verify=verify, mod=mod, omod=omod, cap=cap)
        assert r.status == status, (mod, omod, r.status)
        assert r.canaries, (mod, omod)


# ---- the cases -------------------------------------------------------------------------------------
def test_one_member_equals_inflate_gzip(ctx):
    d = text(50000, 3)
    f = gzip.compress(d, 6)
    assert ctx.inflate_gzip(f) == d
    idx = check_ok(ctx, f, want=d)
    assert idx.tolist() == [[0, 0], [len(f), len(d)]]
    bad = f[:-6] + bytes([f[-6] ^ 1]) + f[-5:]  # the same status as the one-member call
    with pytest.raises(dmx.DmxError) as e:
        ctx.inflate_gzip(bad)
    check_status(ctx, bad, e.value.code, cap=len(d))
    assert e.value.code == dmx.DMX_ERR_CHECKSUM


def test_empty_file(ctx):
    for mod, omod in MODS:
        r = run(ctx, b"", mod=mod, omod=omod, cap=0)
        assert (r.status, r.bytes, r.members) == (dmx.DMX_OK, b"", 0) and r.canaries
        assert r.index.tolist() == [[0, 0]]
    assert ctx.decompress_gzip_members(b"") == b""


def test_header_variety(ctx):
    parts = [b"", b"q", text(70000, 9)]
    f = (gz(parts[0], name=b"empty.txt") + gz(parts[1], extra=b"XY\x03\x00abc") +
         gz(parts[2], comment=b"a comment, then a header CRC", hcrc=True))
    assert gzip.decompress(f) == b"".join(parts)
    idx = check_ok(ctx, f)
    a = len(gz(parts[0], name=b"empty.txt"))
    b = a + len(gz(parts[1], extra=b"XY\x03\x00abc"))
    assert idx.tolist() == [[0, 0], [a, 0], [b, 1], [len(f), 70001]]


def test_4096_members(ctx):
    src = text(4096 * 1024, 17)
    ms = []
    for k in range(4096):
        d = src[1024 * k:1024 * k + 1024]
        ms.append(ctx.compress_gzip(d, 2) if k % 16 == 5 else gz(d, level=(1, 6, 9)[k % 3]))
    f = b"".join(ms)
    idx = check_ok(ctx, f, want=src, mods=MODS[1:2])
    assert idx.shape == (4097, 2)


def nested_file(outer_fill=3000):
    inner = gz(text(500, 1), name=b"inner.txt")
    pay = text(outer_fill, 2) + inner + text(100, 3) + b"\x1f\x8b\x08\x00" + text(200, 4)
    return gz(pay, level=0) + gz(text(900, 5)) + gz(b""), pay


def test_nested_gz_is_not_a_member(ctx):
    f, pay = nested_file()
    assert f.count(b"\x1f\x8b\x08") == 5  # the outer member exposes two more than the chain has
    assert gzip.decompress(f) == pay + text(900, 5)
    idx = check_ok(ctx, f)
    assert idx.shape[0] - 1 == 3


@pytest.mark.parametrize("long_name", [False, True])
def test_tile_edge_candidates(ctx, long_name):
    """The second member starts 0-3 bytes before and behind a multiple of the scan's tile in the
    16-byte aligned view of the file; with a long FNAME the header crosses the edge."""
    second = gz(text(300, 6), name=(b"n" * 200 if long_name else None))
    third = gz(text(40, 7))
    for mod in (0, 5):
        for edge in (TILE, 2 * TILE):
            for delta in range(-3, 4):
                start = edge + delta - mod - (100 if long_name else 0)  # the first member's size
                first_plain = text(start - 23, 8)  # header 10, one stored block 5, trailer 8
                first = gz(first_plain, raw=stored_raw(first_plain))
                assert len(first) == start
                f = first + second + third
                idx = check_ok(ctx, f, want=first_plain + text(300, 6) + text(40, 7), mods=((mod, 7),))
                assert idx[1, 0] == start


def test_zero_padding(ctx):
    a, b, c = gz(text(2000, 10)), gz(text(10, 11), name=b"x"), gz(b"")
    for pad in (1, 7, 512):
        z = bytes(pad)
        check_ok(ctx, a + z + b + z + c + z)
        check_ok(ctx, a + b + c + z, mods=MODS[:1])


def test_garbage_and_leading_zeros(ctx):
    a = gz(text(2000, 10))
    check_status(ctx, a + b"xy", dmx.DMX_ERR_DATA)
    check_status(ctx, a + bytes(5) + b"xy", dmx.DMX_ERR_DATA)
    check_status(ctx, a + gz(text(10, 1)) + b"xy", dmx.DMX_ERR_DATA)
    check_status(ctx, bytes(3) + a, dmx.DMX_ERR_DATA)
    check_status(ctx, bytes(64), dmx.DMX_ERR_DATA)
    check_status(ctx, b"x", dmx.DMX_ERR_DATA)


def test_truncated_last_member(ctx):
    a, b = gz(text(2000, 10)), gz(text(3000, 12), name=b"last.txt")
    f = a + b
    for cut in (len(f) - 300, len(f) - 9,          # inside the stream
                len(f) - 8, len(f) - 3, len(f) - 1,  # inside the trailer
                len(a) + 2, len(a) + 3, len(a) + 12, len(a) + 17):  # inside the header, behind the magic
        check_status(ctx, f[:cut], dmx.DMX_ERR_OVERREAD, mods=MODS[1:2])
    check_status(ctx, a[:len(a) - 2], dmx.DMX_ERR_OVERREAD, mods=MODS[:1])  # the first member, too
    check_status(ctx, a + b"\x1f", dmx.DMX_ERR_OVERREAD, mods=MODS[:1])
    check_status(ctx, a + b"\x1f\x8c", dmx.DMX_ERR_DATA, mods=MODS[:1])


def test_checksum(ctx):
    parts = [text(1500, k) for k in range(4)]
    ms = [gz(p) for p in parts]
    want = b"".join(parts)
    for at in (-8, -5, -4, -1):  # CRC-32 bytes, ISIZE bytes of member 2 of 4
        m = bytearray(ms[1])
        m[at] ^= 0x10
        f = ms[0] + bytes(m) + ms[2] + ms[3]
        check_status(ctx, f, dmx.DMX_ERR_CHECKSUM, cap=len(want))
        check_ok(ctx, f, want=want, verify=False, mods=MODS[1:2], layout=b"".join(ms))


def limit_file(kind):
    if kind in ("T-1", "T", "T+1"):
        size = T + ("T-1", "T", "T+1").index(kind) - 1
        mid_plain = text(size - 5 * 16, 20)  # 16 stored blocks of at most 65535 bytes
        raw = stored_raw(mid_plain)
        assert len(raw) == size
        mid = gz(mid_plain, raw=raw)
    elif kind == "random":
        mid_plain = dmx.corpus("random", 3 << 19)
        mid = gz(mid_plain, level=1)
        assert len(mid) > T + (1 << 18)
    else:
        mid_plain = text(10 << 20, 21)
        mid = gz(mid_plain, level=1)
        assert len(mid) > 3 << 20, len(mid)
    small = [text(700, 22), text(5000, 23)]
    return gz(small[0]) + mid + gz(small[1], name=b"tail") + gz(b""), small[0] + mid_plain + small[1]


@pytest.mark.parametrize("kind", ["T-1", "T", "T+1", "random", "text"])
def test_the_measuring_limit(ctx, kind):
    f, want = limit_file(kind)
    check_ok(ctx, f, want=want, mods=MODS[1:2] if kind == "text" else MODS[1:])


def stats_of(ctx):
    s = ctx.stats()
    return {"segments": s.segments, "path": s.path, "in_bytes": s.in_bytes, "out_bytes": s.out_bytes}


@pytest.mark.parametrize("verify", [True, False])
def test_stats(ctx, verify):
    """dmx_last_stats after the call: the member count (not the batch's), path 6, and the bytes --
    for a file the batch decodes alone and for one with a long member between two short ones."""
    parts = [text(100, 1), text(101, 2), text(99, 3)]
    f = b"".join(gz(p) for p in parts)
    r = run(ctx, f, verify=verify)
    assert r.status == dmx.DMX_OK and r.bytes == b"".join(parts) and r.members == 3
    assert stats_of(ctx) == {"segments": 3, "path": 6, "in_bytes": len(f), "out_bytes": 300}
    lf, lwant = limit_file("T+1")
    r = run(ctx, lf, verify=verify, want=lwant)
    assert r.status == dmx.DMX_OK and r.bytes == lwant and r.members == 4
    assert stats_of(ctx) == {"segments": 4, "path": 6, "in_bytes": len(lf), "out_bytes": len(lwant)}


def test_long_member_with_a_false_candidate_behind_its_limit(ctx):
    inner = gz(text(500, 1), name=b"inner.txt")
    pay = text(1200 << 10, 30) + inner + text(800 << 10, 31)
    f = gz(text(100, 32)) + gz(pay, raw=stored_raw(pay)) + gz(text(100, 33)) + gz(text(64, 34))
    idx = check_ok(ctx, f, want=text(100, 32) + pay + text(100, 33) + text(64, 34), mods=MODS[1:2])
    assert idx.shape[0] - 1 == 4


def test_lenient_count_equals_the_batch_decoder(ctx):
    """A copy with a distance beyond the member's start: the measuring pass must count what the
    batch decoder writes."""
    raw = open(os.path.join(GOLDEN, "lenient_far_distance.deflate"), "rb").read()
    m = gz(b"", raw=raw)  # (the trailer is not that of the bytes: verify is off)
    t, off = dev(m, 1)
    out, ooff = area(64, 7)
    res = ctx.inflate_batch_framed_device([t.data_ptr() + off], [len(m)], [out.data_ptr() + ooff], [64], format="gzip",
                                          verify=False)
    torch.cuda.synchronize()
    nbytes, status = res[0][0], res[0][1]
    assert status == dmx.DMX_OK
    alone = host_of(out)[ooff:ooff + nbytes]
    f = gz(text(50, 1)) + m + gz(text(60, 2))
    r = run(ctx, f, verify=False, cap=200)
    assert r.status == dmx.DMX_OK and r.canaries
    assert r.bytes == text(50, 1) + alone + text(60, 2)
    assert r.members == 3 and r.index[2, 1] - r.index[1, 1] == nbytes


def test_capacity(ctx):
    ms = [gz(text(1000 + k, k)) for k in range(40)]
    f = b"".join(ms)
    total = len(gzip.decompress(f))
    r = run(ctx, f, cap=total - 1)
    assert r.status == dmx.DMX_ERR_CAPACITY and r.error.needed == total
    assert r.canaries and r.inside == bytes([FILL]) * (total - 1)  # nothing was written
    # a table too small: the member count comes back
    t, off = dev(f, 1)
    out, ooff = area(total, 7)
    ent = (dmx.BgzfEntry * 40)()
    m, n = ctypes.c_size_t(), ctypes.c_size_t(5)
    rc = dmx.lib().dmx_inflate_gzip_members_device(ctx.h, ctypes.c_void_p(t.data_ptr() + off), len(f), dmx.DMX_VERIFY,
                                                   ctypes.c_void_p(out.data_ptr() + ooff), total, ent, 40,
                                                   ctypes.byref(m), ctypes.byref(n), None)
    torch.cuda.synchronize()
    assert (rc, m.value, n.value) == (dmx.DMX_ERR_CAPACITY, 40, 0)
    assert canaries_ok(host_of(out), ooff, total)
    # a long member that does not fit what is left: the size is not known
    lf, lwant = limit_file("T+1")
    r = run(ctx, lf, cap=len(lwant) - 6000, mod=7, omod=1)
    assert r.status == dmx.DMX_ERR_CAPACITY and not r.error.needed and r.canaries


def test_host_form_and_python(ctx):
    parts = [bytes(4 << 20), text(3000, 40), bytes([7]) * (3 << 20), b""]
    f = b"".join(gzip.compress(p, 6) for p in parts) + bytes(9)
    want = b"".join(parts)
    assert len(want) > max(1 << 20, 8 * len(f))  # the first capacity is too small: the call is repeated
    assert ctx.decompress_gzip_members(f) == want
    assert ctx.decompress_gzip_members(f, verify=False, cap=len(want)) == want
    with pytest.raises(dmx.DmxError) as e:
        ctx.decompress_gzip_members(f, cap=len(want) - 1)
    assert e.value.code == dmx.DMX_ERR_CAPACITY and e.value.needed == len(want)
    with pytest.raises(dmx.DmxError) as e:
        ctx.decompress_gzip_members(f + b"xy")
    assert e.value.code == dmx.DMX_ERR_DATA
    with pytest.raises(dmx.DmxError) as e:
        ctx.decompress_gzip_members(f[:len(f) - 12])
    assert e.value.code == dmx.DMX_ERR_OVERREAD
    lf, lwant = limit_file("random")  # a long member through the host form
    assert ctx.decompress_gzip_members(lf) == lwant
