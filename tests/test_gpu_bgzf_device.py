"""GPU: BGZF files in device memory -- dmx_deflate_bgzf_device, dmx_bgzf_index_device,
dmx_inflate_bgzf_device, dmx_inflate_bgzf_range_device (csrc/bgzf_chain.hip).

References: Python's gzip / zlib, a Python walk of the member chain from offset 0, and the host
calls compress_bgzf / decompress_bgzf.  Every file is built once and every call is made once."""
import gzip
import struct
import zlib

import numpy as np
import pytest
import torch

import dmx

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
BLOCK = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

_cache = {}


def member(d, level=6, before=b"", stored=False):
    """A BGZF member built by hand around zlib's raw stream (stored: around a stored block)."""
    if stored:  # one final stored block, written out: the payload starts 5 bytes behind the header
        raw = b"\x01" + struct.pack("<HH", len(d), len(d) ^ 0xFFFF) + d
    else:
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = z.compress(d) + z.flush()
    extra = before + b"BC\x02\x00" + struct.pack("<H", 12 + len(before) + 6 + len(raw) + 8 - 1)
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(extra)) + extra + raw +
            struct.pack("<II", zlib.crc32(d), len(d) & 0xFFFFFFFF))


def walk(f):
    """The serial walk from offset 0 of a well-formed file -> the (members + 1, 2) index."""
    rows, o, u = [], 0, 0
    while o < len(f):
        assert f[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", f, o + 10)[0]
        p, size = o + 12, None
        while p + 4 <= o + 12 + xlen:
            slen = struct.unpack_from("<H", f, p + 2)[0]
            if f[p:p + 2] == b"BC" and slen == 2:
                size = struct.unpack_from("<H", f, p + 4)[0] + 1
                break
            p += 4 + slen
        assert size is not None, o
        rows.append((o, u))
        u += struct.unpack_from("<I", f, o + size - 4)[0]
        o += size
    assert o == len(f)
    return np.array(rows + [(len(f), u)], dtype=np.uint64).reshape(-1, 2)


def dev(data, mod=0, extra=0):
    """`data` at an offset that is `mod` modulo 16 inside a FILL-filled device tensor, PAD bytes of
    canary before it and PAD + extra behind -> (tensor, offset)."""
    off = PAD + mod
    host = bytearray([FILL]) * (off + len(data) + extra + PAD)
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


def status_of(fn, *a, **k):
    try:
        return dmx.DMX_OK, fn(*a, **k)
    except dmx.DmxError as e:
        return e.code, e


def inflate_dev(ctx, f, verify=True, mod=1, omod=7, cap=None, stream=None):
    """-> (status, plain bytes or the error, the output area's bytes, its offset)"""
    t, off = dev(f, mod)
    cap = len(gzip.decompress(f)) if cap is None else cap
    out, ooff = area(cap, omod)
    st, val = status_of(ctx.inflate_bgzf_device, t.data_ptr() + off, len(f), out.data_ptr() + ooff, cap,
                        verify=verify, stream=stream)
    torch.cuda.synchronize()
    h = host_of(out)
    return st, (h[ooff:ooff + val] if st == dmx.DMX_OK else val), h, ooff


def index_dev(ctx, f, mod=7):
    t, off = dev(f, mod)
    idx = ctx.bgzf_index_device(t.data_ptr() + off, len(f))
    assert host_of(t) == host_of(dev(f, mod)[0])  # the input is only read
    return idx


# ---- deflate ------------------------------------------------------------------------------------
DEFLATE_SIZES = [0, 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7, (1 << 20) + 3]


def plain(n):
    if ("plain", n) not in _cache:
        _cache[("plain", n)] = dmx.corpus("text", n // 2, offset=11) + dmx.corpus("mixed", n - n // 2, offset=5)
    return _cache[("plain", n)]


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_deflate_equals_host_form(ctx, level):
    for i, n in enumerate(DEFLATE_SIZES):
        d = plain(n)
        want = ctx.compress_bgzf(d, level)
        assert gzip.decompress(want) == d
        bound = dmx.bgzf_bound(n)
        assert len(want) <= bound
        for imod, omod in ((0, 0), (1, 7), (7, 1)):
            t, off = dev(d, imod)
            out, ooff = area(bound, omod)
            got = ctx.deflate_bgzf_device(t.data_ptr() + off, n, level, out.data_ptr() + ooff, bound)
            torch.cuda.synchronize()
            h = host_of(out)
            assert got == len(want), (n, imod, omod)
            assert h[ooff:ooff + got] == want, (n, imod, omod)
            assert canaries_ok(h, ooff, got), (n, imod, omod)
        # one byte short: the size needed is reported, nothing is written past cap
        cap = len(want) - 1
        t, off = dev(d, (i * 5) % 16)
        out, ooff = area(cap, 7)
        st, e = status_of(ctx.deflate_bgzf_device, t.data_ptr() + off, n, level, out.data_ptr() + ooff, cap)
        torch.cuda.synchronize()
        assert st == dmx.DMX_ERR_CAPACITY and e.needed == len(want), n
        h = host_of(out)
        assert h[ooff + cap:] == bytes([FILL]) * (len(h) - ooff - cap) and h[:ooff] == bytes([FILL]) * ooff


def test_deflate_needs_a_segmented_context(ctx):
    c64 = dmx.Context(segment_bytes=65536)
    try:
        t, off = dev(plain(1000))
        out, ooff = area(dmx.bgzf_bound(1000))
        st, _ = status_of(c64.deflate_bgzf_device, t.data_ptr() + off, 1000, 2, out.data_ptr() + ooff,
                          dmx.bgzf_bound(1000))
        assert st == dmx.DMX_ERR_ARG
    finally:
        c64.close()


# ---- member counts across wave / workgroup / tile edges -------------------------------------------
def tiny_members(count, empties=()):
    if ("tiny", 2500) not in _cache:
        src = dmx.corpus("text", 100 * 2500, offset=3)
        _cache[("tiny", 2500)] = [member(src[100 * k:100 * k + 100]) for k in range(2500)]
    ms = list(_cache[("tiny", 2500)][:count])
    for e in empties:
        ms[e] = EOF_BLOCK
    return ms


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2500])
def test_member_counts(ctx, count):
    ms = tiny_members(count)
    for tail in (EOF_BLOCK, b""):
        f = b"".join(ms) + tail
        want = gzip.decompress(f)
        assert np.array_equal(index_dev(ctx, f, mod=count % 16), walk(f))
        st, got, h, ooff = inflate_dev(ctx, f, mod=(count * 3) % 16)
        assert st == dmx.DMX_OK and got == want
        assert canaries_ok(h, ooff, len(want))


def test_empty_members_in_the_middle(ctx):
    f = b"".join(tiny_members(300, empties=(0, 5, 6, 64, 255, 299))) + EOF_BLOCK
    idx = index_dev(ctx, f)
    assert np.array_equal(idx, walk(f))
    st, got, h, ooff = inflate_dev(ctx, f)
    assert st == dmx.DMX_OK and got == gzip.decompress(f) and canaries_ok(h, ooff, len(got))
    assert dmx.gzi_bytes(idx)[:8] == struct.pack("<Q", 300)


def test_empty_files(ctx):
    for f in (b"", EOF_BLOCK):
        assert np.array_equal(index_dev(ctx, f), walk(f))
        st, got, h, ooff = inflate_dev(ctx, f, cap=0)
        assert st == dmx.DMX_OK and got == b"" and canaries_ok(h, ooff, 0)


TILE = 4096  # the candidate scan's tile (csrc/cand_scan.h)


def test_tile_edge_members(ctx):
    """The second of three members starts 0-3 bytes before and behind a multiple of the scan's tile
    in the 16-byte aligned view of the file, whose first byte sits at `mod` in that view."""
    src = dmx.corpus("text", 2 * TILE + 400, offset=17)
    second, third = member(src[:300]), member(src[300:340])
    for mod in (0, 5):
        for edge in (TILE, 2 * TILE):
            for delta in range(-3, 4):
                start = edge + delta - mod  # the first member's size
                first = member(src[340:340 + start - 31], stored=True)  # header 18, stored block 5, trailer 8
                assert len(first) == start
                f = first + second + third
                want = walk(f)
                assert want[1, 0] == start
                assert np.array_equal(index_dev(ctx, f, mod=mod), want), (mod, edge, delta)
                st, got, h, ooff = inflate_dev(ctx, f, mod=mod)
                assert st == dmx.DMX_OK and got == gzip.decompress(f), (mod, edge, delta)
                assert canaries_ok(h, ooff, len(got)), (mod, edge, delta)


# ---- hostile candidates ----------------------------------------------------------------------------
def stored_again(inner, block=BLOCK):
    return b"".join(member(inner[o:o + block], stored=True) for o in range(0, len(inner), block)) + EOF_BLOCK


def fake_headers(payload=BLOCK):
    """One stored member whose payload is back-to-back fake 18-byte headers, then real members.
    Fake k's BSIZE: k % 3 == 0 lands exactly on the next real member's start, k % 3 == 1 points
    past the end of the file, k % 3 == 2 lands on a later fake header."""
    tails = member(dmx.corpus("text", 300)) + member(dmx.corpus("mixed", 40)) + EOF_BLOCK
    pay_at = 18 + 5
    next_real = pay_at + payload + 8
    n = next_real + len(tails)
    pay = bytearray(payload)
    for k in range(payload // 18):
        at = pay_at + 18 * k
        size = next_real - at if k % 3 == 0 else n - at + 1 + k % 7 if k % 3 == 1 else 18 * (2 + k % 5)
        if size < 26 or size > 65536:
            size = 65536
        pay[18 * k:18 * k + 18] = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", size - 1)
    f = member(bytes(pay), stored=True) + tails
    assert len(f) == n
    return f


@pytest.mark.parametrize("which", ["stored_again", "fake_headers"])
def test_hostile_candidates(ctx, which):
    if which == "stored_again":
        f = stored_again(b"".join(tiny_members(1500)) + EOF_BLOCK)
    else:
        f = fake_headers()
    want = gzip.decompress(f)
    assert np.array_equal(index_dev(ctx, f), walk(f))
    st, got, h, ooff = inflate_dev(ctx, f)
    assert st == dmx.DMX_OK and got == want and canaries_ok(h, ooff, len(want))


# ---- errors equal the host's -----------------------------------------------------------------------
def mutated_files():
    parts = [dmx.corpus("text", 200, offset=1), dmx.corpus("mixed", 77, offset=2), dmx.corpus("text", 130, offset=3)]
    ms = [member(p) for p in parts]
    f = b"".join(ms)
    starts = [0, len(ms[0]), len(ms[0]) + len(ms[1])]
    out = []
    cuts = {0, 1, 17, 18, 19, 25, 26, 27} | set(range(len(f) - 9, len(f)))
    for s in starts[1:]:
        cuts |= {s - 1, s, s + 1, s + 17, s + 18, s + 19}
    out += [("cut %d" % n, f[:n]) for n in sorted(cuts)]

    def flip(at, x, what):
        b = bytearray(f)
        b[at] ^= x
        out.append(("%s at %d" % (what, at), bytes(b)))

    for k, s in enumerate(starts):
        size = len(ms[k])
        for at, x, what in ((0, 0x01, "magic"), (1, 0x80, "magic"), (2, 0x01, "CM"), (3, 0x04, "FLG"),
                            (10, 0x01, "XLEN"), (10, 0x80, "XLEN"), (11, 0x01, "XLEN"), (12, 0x01, "SI"),
                            (14, 0x01, "SLEN"), (16, 0x01, "BSIZE"), (16, 0x80, "BSIZE"), (17, 0x01, "BSIZE"),
                            (17, 0x80, "BSIZE")):
            flip(s + at, x, what)
        for b in range(3 if k else 4):  # (the top ISIZE byte once: 16 MiB of claimed output)
            flip(s + size - 4 + b, 0x01, "ISIZE")
        for b in (0, 3):
            flip(s + size - 8 + b, 0x10, "CRC")
        flip(s + 18, 0x04, "payload")
        flip(s + 18 + (size - 26) // 2, 0x40, "payload")
        flip(s + size - 9, 0x80, "payload")
    for delta in (1, -1, 1000):  # a member whose ISIZE lies
        m = bytearray(ms[1])
        m[-4:] = struct.pack("<I", len(parts[1]) + delta)
        out.append(("ISIZE %+d" % delta, ms[0] + bytes(m) + ms[2] + EOF_BLOCK))
    out.append(("plain gzip", gzip.compress(parts[0])))
    out.append(("subfield before BC", member(parts[0], before=b"XY\x03\x00abc") + ms[1] + EOF_BLOCK))
    return out


def claimed_bytes(f):
    """The sum of ISIZE along the BSIZE chain when it covers the file, else 0: a broken chain is
    reported before any capacity is looked at."""
    o, u = 0, 0
    while o + 18 <= len(f) and f[o:o + 4] == b"\x1f\x8b\x08\x04" and f[o + 12:o + 16] == b"BC\x02\x00":
        size = struct.unpack_from("<H", f, o + 16)[0] + 1
        if size < 26 or o + size > len(f):
            break
        u += struct.unpack_from("<I", f, o + size - 4)[0]
        o += size
    return u if o == len(f) else 0


def test_errors_equal_the_host_form(ctx):
    seen = set()
    for what, f in mutated_files():
        for verify in (True, False):
            hst, hval = status_of(ctx.decompress_bgzf, f, verify=verify)
            # (room for what the trailers claim: the capacity check precedes the decode)
            cap = max(2000, claimed_bytes(f))
            st, got, h, ooff = inflate_dev(ctx, f, verify=verify, cap=cap)
            assert st == hst, (what, verify, st, hst)
            if st == dmx.DMX_OK:
                assert got == hval, (what, verify)
            assert canaries_ok(h, ooff, cap), (what, verify)
            seen.add(st)
    assert {dmx.DMX_OK, dmx.DMX_ERR_DATA, dmx.DMX_ERR_OVERREAD, dmx.DMX_ERR_CHECKSUM} <= seen
    # the index reports the chain's errors and trusts ISIZE
    f = mutated_files()[5][1]
    t, off = dev(f)
    st, _ = status_of(ctx.bgzf_index_device, t.data_ptr() + off, len(f))
    assert st == dmx.DMX_ERR_OVERREAD


def test_flags_and_arguments(ctx):
    import ctypes
    f = b"".join(tiny_members(3)) + EOF_BLOCK
    t, off = dev(f)
    out, ooff = area(300)
    n = ctypes.c_size_t()
    lib = dmx.lib()
    p, q = ctypes.c_void_p(t.data_ptr() + off), ctypes.c_void_p(out.data_ptr() + ooff)
    assert lib.dmx_inflate_bgzf_device(ctx.h, p, len(f), 2, q, 300, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    m = ctypes.c_size_t()
    entries = (dmx.BgzfEntry * 3)()
    assert lib.dmx_bgzf_index_device(ctx.h, p, len(f), entries, 3, ctypes.byref(m), None, None) == dmx.DMX_ERR_CAPACITY
    assert m.value == 4
    torch.cuda.synchronize()
    assert canaries_ok(host_of(out), ooff, 0)


# ---- capacity ----------------------------------------------------------------------------------------
def test_inflate_capacity(ctx):
    f = b"".join(tiny_members(70)) + EOF_BLOCK
    total = len(gzip.decompress(f))
    st, e, h, ooff = inflate_dev(ctx, f, cap=total - 1)
    assert st == dmx.DMX_ERR_CAPACITY and e.needed == total
    assert h == bytes([FILL]) * len(h)


# ---- ranged reads ------------------------------------------------------------------------------------
def range_file():
    if "range" not in _cache:
        parts = [dmx.corpus("text", BLOCK, offset=1), dmx.corpus("mixed", BLOCK, offset=2), b"",
                 dmx.corpus("text", BLOCK, offset=3), dmx.corpus("mixed", 1000, offset=4)]
        _cache["range"] = ([member(p) for p in parts], b"".join(parts))
    return _cache["range"]


def range_dev(ctx, f, idx, u, ln, verify=True):
    t, off = dev(f, 3)
    out, ooff = area(ln, 9)
    st, _ = status_of(ctx.inflate_bgzf_range_device, t.data_ptr() + off, len(f), idx, u, ln,
                      out.data_ptr() + ooff, verify=verify)
    torch.cuda.synchronize()
    h = host_of(out)
    outside = h[:ooff] + h[ooff + ln:]  # nothing outside [d_out, d_out + len) is touched
    return st, h[ooff:ooff + ln], outside == bytes([FILL]) * len(outside)


def test_ranges(ctx):
    ms, whole = range_file()
    f = b"".join(ms) + EOF_BLOCK
    assert gzip.decompress(f) == whole and len(whole) == 3 * BLOCK + 1000
    idx = index_dev(ctx, f)
    assert np.array_equal(idx, walk(f)) and idx.shape == (7, 2)
    total = len(whole)
    for u, ln in ((0, 0), (0, 1), (BLOCK - 1, 2), (BLOCK, 1), (65000, 70000), (0, total), (total - 1, 1),
                  (2 * BLOCK - 5, 10), (2 * BLOCK, BLOCK + 1000)):
        for verify in (True, False):
            st, got, fill_ok = range_dev(ctx, f, idx, u, ln, verify)
            assert st == dmx.DMX_OK, (u, ln)
            assert got == whole[u:u + ln], (u, ln)
            assert fill_ok, (u, ln)
    for u, ln in ((total, 1), (total - 1, 2), (total + 1, 0)):  # past the end
        st, _, fill_ok = range_dev(ctx, f, idx, u, ln)
        assert st == dmx.DMX_ERR_ARG and fill_ok
    bad = idx.copy()
    bad[2, 1] = bad[3, 1] + 1  # not monotone
    assert range_dev(ctx, f, bad, 0, 10)[0] == dmx.DMX_ERR_ARG


def test_range_verifies_the_touched_members_only(ctx):
    ms, whole = range_file()
    m = bytearray(ms[1])
    m[-7] ^= 0x20  # a CRC byte of member 1
    f = ms[0] + bytes(m) + b"".join(ms[2:]) + EOF_BLOCK
    idx = walk(f)
    st, got, fill_ok = range_dev(ctx, f, idx, 10, 5000)                 # member 0 only
    assert st == dmx.DMX_OK and got == whole[10:5010] and fill_ok
    st, got, fill_ok = range_dev(ctx, f, idx, 2 * BLOCK + 1, BLOCK)     # members 3 and 4
    assert st == dmx.DMX_OK and got == whole[2 * BLOCK + 1:3 * BLOCK + 1] and fill_ok
    st, _, fill_ok = range_dev(ctx, f, idx, BLOCK - 1, 2)               # members 0 and 1
    assert st == dmx.DMX_ERR_CHECKSUM and fill_ok
    st, got, _ = range_dev(ctx, f, idx, BLOCK - 1, 2, verify=False)
    assert st == dmx.DMX_OK and got == whole[BLOCK - 1:BLOCK + 1]
    lie = idx.copy()
    lie[2:, 1] += 1  # the index gives member 1 one plain byte too many: the ISIZE rule, unverified too
    assert range_dev(ctx, f, lie, BLOCK, 10, verify=False)[0] == dmx.DMX_ERR_CHECKSUM


# ---- the call's figures --------------------------------------------------------------------------------
def stats_of(ctx):
    s = ctx.stats()
    return {"segments": s.segments, "path": s.path, "in_bytes": s.in_bytes, "out_bytes": s.out_bytes}


@pytest.mark.parametrize("verify", [True, False])
def test_stats(ctx, verify):
    """dmx_last_stats after the two decoding calls: the members decoded (the EOF member is one),
    path 6, and the bytes."""
    parts = [dmx.corpus("text", 3000, offset=1), dmx.corpus("mixed", BLOCK, offset=2), dmx.corpus("text", 500, offset=3)]
    whole = b"".join(parts)
    f = b"".join(member(p) for p in parts) + EOF_BLOCK
    st, got, _, _ = inflate_dev(ctx, f, verify=verify)
    assert st == dmx.DMX_OK and got == whole
    assert stats_of(ctx) == {"segments": 4, "path": 6, "in_bytes": len(f), "out_bytes": len(whole)}
    # a range over the end of member 0 and the start of member 1
    st, got, fill_ok = range_dev(ctx, f, walk(f), 2990, 100, verify=verify)
    assert st == dmx.DMX_OK and got == whole[2990:3090] and fill_ok
    s = stats_of(ctx)
    assert (s["segments"], s["path"], s["out_bytes"]) == (2, 6, 100)


# ---- stream order ------------------------------------------------------------------------------------
def test_calls_are_ordered_on_the_callers_stream(ctx):
    n = 3 * BLOCK + 7
    d = plain(n)
    want = ctx.compress_bgzf(d, 2)
    src = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    bound = dmx.bgzf_bound(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
        f = torch.full((bound + 16,), FILL, dtype=torch.uint8, device="cuda")
        back = torch.full((n + 16,), FILL, dtype=torch.uint8, device="cuda")
        part = torch.full((1000 + 16,), FILL, dtype=torch.uint8, device="cuda")
        t[1:1 + n] = src ^ 0x5A  # kernels on s write the input ...
        t[1:1 + n] ^= 0x5A
        got = ctx.deflate_bgzf_device(t.data_ptr() + 1, n, 2, f.data_ptr() + 3, bound, stream=s.cuda_stream)
        idx = ctx.bgzf_index_device(f.data_ptr() + 3, got, stream=s.cuda_stream)
        m = ctx.inflate_bgzf_device(f.data_ptr() + 3, got, back.data_ptr() + 5, n, stream=s.cuda_stream)
        ctx.inflate_bgzf_range_device(f.data_ptr() + 3, got, idx, BLOCK - 500, 1000, part.data_ptr() + 7,
                                      stream=s.cuda_stream)
    s.synchronize()
    assert got == len(want) and host_of(f)[3:3 + got] == want
    assert np.array_equal(idx, walk(want))
    assert m == n and host_of(back)[5:5 + n] == d
    assert host_of(part)[7:1007] == d[BLOCK - 500:BLOCK + 500]
