"""GPU: the seek index and ranged reads of unblocked DEFLATE streams -- dmx_inflate_index_device,
dmx_inflate_range_device (csrc/inflate_span.hip, seek_plan.cpp, the checkpoint hand-over of paths 4
and 5).

References: the plain bytes themselves, and -- for every checkpoint, independently of libdmx --
zlib started at the checkpoint's bit behind the checkpoint's window.  Every stream is built and
indexed once; the tests share the result and leave it unchanged."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import deflate_inspect
import dmx
import streams

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
W = dmx.DMX_SEEK_WINDOW
NOWINDOW = dmx.DMX_SEEK_NOWINDOW

_cache = {}


def zraw(d, lvl=6, st=0):  # (tests/test_gpu_parity.py: the streams it asserts path 5 for)
    z = zlib.compressobj(lvl, zlib.DEFLATED, -15, 9, st)
    return z.compress(d) + z.flush()


def dev(data, mod=0, extra=0):
    """`data` at an offset that is `mod` modulo 16 inside a FILL-filled device tensor, PAD bytes
    before it and PAD + extra behind -> (tensor, offset)."""
    off = PAD + mod
    host = bytearray([FILL]) * (off + len(data) + extra + PAD)
    host[off:off + len(data)] = data
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, off


def host_of(t):
    return t.cpu().numpy().tobytes()


def status_of(fn, *a, **k):
    try:
        return dmx.DMX_OK, fn(*a, **k)
    except dmx.DmxError as e:
        return e.code, e


class Indexed:
    """A stream in device memory, decoded and indexed once."""

    def __init__(self, ctx, stream, data, spacing, mod=3):
        self.stream, self.data, self.spacing = stream, data, spacing
        self.t, self.off = dev(stream, mod)
        self.out, self.ooff = dev(bytes(len(data)), 5)
        self.out_len, self.entries, self.windows = ctx.inflate_index_device(
            self.t.data_ptr() + self.off, len(stream), self.out.data_ptr() + self.ooff, len(data), spacing)
        self.path = ctx.stats().path
        torch.cuda.synchronize()
        self.count = self.entries.shape[0] - 1

    @property
    def d_in(self):
        return self.t.data_ptr() + self.off

    def decoded(self):
        h = host_of(self.out)
        outside = h[:self.ooff] + h[self.ooff + len(self.data):]
        return h[self.ooff:self.ooff + len(self.data)], outside == bytes([FILL]) * len(outside)


def read(ctx, ix, u, ln, entries=None, n=None):
    """A ranged read into pointer offset 1 of a FILL-filled area -> (status, bytes, nothing outside
    [d_out, d_out + ln) touched -- the 64 guard bytes behind it included)."""
    area = torch.full((1 + ln + 64 + 15,), FILL, dtype=torch.uint8, device="cuda")
    st, _ = status_of(ctx.inflate_range_device, ix.d_in, len(ix.stream) if n is None else n,
                      ix.entries if entries is None else entries, ix.windows, u, ln, area.data_ptr() + 1)
    torch.cuda.synchronize()
    h = host_of(area)
    outside = h[:1] + h[1 + ln:]
    return st, h[1:1 + ln], outside == bytes([FILL]) * len(outside)


def check_ranges(ctx, ix, ranges):
    for u, ln in ranges:
        st, got, guard_ok = read(ctx, ix, u, ln)
        assert st == dmx.DMX_OK, (u, ln, st)
        assert got == ix.data[u:u + ln], (u, ln)
        assert guard_ok, (u, ln)


# ---- third-party streams: path 5 --------------------------------------------------------------------
FOREIGN = [("text", 1), ("mixed", 6)]


def foreign(ctx, kind, lvl):
    if (kind, lvl) not in _cache:
        d = dmx.corpus(kind, 4 << 20, offset=99)
        _cache[(kind, lvl)] = Indexed(ctx, zraw(d, lvl), d, 262144)
    return _cache[(kind, lvl)]


def block_map(ctx, kind, lvl):
    """tests/deflate_inspect (a Python decoder that shares nothing with libdmx) over the whole stream,
    once -> ({header bit of every block: plain bytes before it}, [plain offsets of the stored blocks])."""
    if ("blocks", kind, lvl) not in _cache:
        s = foreign(ctx, kind, lvl).stream
        out, at, stored, pos = bytearray(), {}, [], 0
        while True:
            before = len(out)
            b = deflate_inspect.read_block(s, pos, out)
            at[b.start] = before
            if b.btype == 0:
                stored.append(before)
            pos = b.end
            if b.bfinal:
                break
        assert bytes(out) == foreign(ctx, kind, lvl).data
        _cache[("blocks", kind, lvl)] = (at, stored)
    return _cache[("blocks", kind, lvl)]


@pytest.mark.parametrize("kind,lvl", FOREIGN)
def test_foreign_stream_index(ctx, kind, lvl):
    """zlib's streams of 4 MiB: every checkpoint is a block header the block-parallel decoder's
    chain passed, at least 256 KiB of plain bytes apart, with the 32 KiB before it in its slot.

    Blocks counted on the CPU with tests/deflate_inspect -- text level 1: 28 blocks, none stored;
    mixed level 6: 37 blocks, 14 of them stored -- so a floor of 4 checkpoints is far below what a
    working index gives.  Checkpoints observed: text level 1: 14, mixed level 6: 12 (the most a
    spacing of 256 KiB allows in 4 MiB is 16).

    Each checkpoint is verified without libdmx, twice.  deflate_inspect's walk of the stream must
    have a block header at exactly `bit` with exactly `uoffset` plain bytes before it.  And zlib,
    given the stream shifted to start at `bit` and the 32 KiB before `uoffset` as its dictionary,
    must give the plain bytes from `uoffset` on.  The shift moves the byte boundaries, and a stored
    block's LEN sits at the next byte boundary: when `bit` is not a multiple of 8 the shifted
    stream means the same only up to the next stored block, so zlib is then asked for the bytes up
    to one short of that block (one short: with room for the last byte zlib would go on to read the
    moved header and fail) -- for the text stream, which has no stored block, that is all of them."""
    ix = foreign(ctx, kind, lvl)
    d, s, e = ix.data, ix.stream, ix.entries
    got, outside_ok = ix.decoded()
    assert ix.out_len == len(d) and got == d and outside_ok
    assert ix.path == 5
    assert tuple(e[0]) == (0, 0, 0, NOWINDOW)
    # the sentinel: the byte past the final block (zlib ends the stream there), the plain bytes
    assert tuple(e[-1]) == (8 * len(s), len(d), 0, 0)
    print(f"\n{kind} level {lvl}: {ix.count} checkpoints")
    assert ix.count >= 4, ix.count
    assert np.all(np.diff(e[:ix.count, 1].astype(np.int64)) >= ix.spacing)
    assert np.all(e[1:ix.count, 2] == W) and np.all(e[1:ix.count, 3] == 0)
    assert ix.windows.numel() == ix.count * W
    header_at, stored = block_map(ctx, kind, lvl)
    bits = np.unpackbits(np.frombuffer(s, dtype=np.uint8), bitorder="little")
    win = host_of(ix.windows)
    whole = bounded = 0
    for k in range(1, ix.count):
        bit, u = int(e[k, 0]), int(e[k, 1])
        assert 0 < bit < 8 * len(s) and W <= u <= len(d)
        assert header_at.get(bit) == u, (k, bit, u)
        shifted = np.packbits(bits[bit:], bitorder="little").tobytes()
        z = zlib.decompressobj(-15, zdict=d[u - W:u])
        behind = [x for x in stored if x >= u]
        if bit % 8 == 0 or not behind:
            assert z.decompress(shifted) == d[u:], k
            assert z.eof, k
            whole += 1
        elif behind[0] - u - 1 > 0:
            assert z.decompress(shifted, behind[0] - u - 1) == d[u:behind[0] - 1], k
            bounded += 1
        assert win[k * W:(k + 1) * W] == d[u - W:u], k
    print(f"zlib from the checkpoint: {whole} to the stream's end, {bounded} up to a stored block, of {ix.count - 1}")
    assert kind != "text" or whole == ix.count - 1
    assert whole + bounded >= 1  # (the zlib check ran, also where stored blocks bound it)


def random_chunk(d, offset=99):
    """A 64 KiB piece of the mixed corpus that is random bytes (the corpus changes kind at
    multiples of 64 KiB of its own offsets) -> its first byte in d."""
    for k in range(1, len(d) // 65536 - 1):
        a = k * 65536 - offset
        if len(zlib.compress(d[a:a + 65536], 1)) > 65536:
            return a
    raise AssertionError("no random piece")


@pytest.mark.parametrize("kind,lvl", FOREIGN)
def test_foreign_stream_ranges(ctx, kind, lvl):
    ix = foreign(ctx, kind, lvl)
    e, total = ix.entries, len(ix.data)
    k = ix.count // 2
    uk, un = int(e[k, 1]), int(e[k + 1, 1])
    ranges = [(0, 1), (0, 100), (0, total), (uk, un - uk), (uk - 1, 2), (uk + 1, 1), (total - 1, 1),
              (1234567, 1 << 20), (0, 0), (uk, 0), (total, 0)]
    if kind == "mixed":  # zlib stores the random pieces: a range that ends inside a stored block
        a = random_chunk(ix.data)
        ranges += [(a - 5000, 5000 + 30000), (a + 100, 70), (a + 65536 - 10, 20)]
    check_ranges(ctx, ix, ranges)


# ---- libdmx's own streams: path 4 ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def c16():
    c = dmx.Context(segment_bytes=16384)
    yield c
    c.close()


def own(c, seg, level):
    if ("own", seg, level) not in _cache:
        d = dmx.corpus("mixed", 1 << 20)
        _cache[("own", seg, level)] = Indexed(c, c.compress(d, level), d, 65536, mod=7)
    return _cache[("own", seg, level)]


@pytest.mark.parametrize("seg", [32768, 16384])
@pytest.mark.parametrize("level", [2, 0])
def test_own_stream_index_and_ranges(ctx, c16, seg, level):
    """libdmx's streams: the checkpoints are segment starts -- byte aligned, behind a 00 00 FF FF
    marker, nothing before them referenced -- one per 64 KiB at this spacing (every second segment
    of 32 KiB, every fourth of 16 KiB)."""
    ctx = ctx if seg == 32768 else c16
    ix = own(ctx, seg, level)
    d, s, e = ix.data, ix.stream, ix.entries
    got, outside_ok = ix.decoded()
    assert ix.out_len == len(d) and got == d and outside_ok
    assert ix.path == 4
    assert ix.count == len(d) // 65536
    assert list(e[:ix.count, 1]) == [65536 * k for k in range(ix.count)]
    assert np.all(e[:ix.count, 2] == 0) and np.all(e[:ix.count, 3] == NOWINDOW)
    assert tuple(e[-1]) == (8 * len(s), len(d), 0, 0)
    for k in range(1, ix.count):
        bit, u = int(e[k, 0]), int(e[k, 1])
        assert bit % 8 == 0 and s[bit // 8 - 4:bit // 8] == b"\x00\x00\xff\xff", k
        assert zlib.decompressobj(-15).decompress(s[bit // 8:]) == d[u:], k
    # (40000, 1000): inside a stored block at level 0; then across three segments, entry edges, the file
    check_ranges(ctx, ix, [(40000, 1000), (65536 - 100, 32768 + 200), (3 * 65536 - 1, 65536 + 2), (0, len(d)),
                           (len(d) - 1, 1), (0, 1), (500000, 0)])
    # the windows are not needed: none of the entries has one
    area = torch.full((1000 + 16,), FILL, dtype=torch.uint8, device="cuda")
    ctx.inflate_range_device(ix.d_in, len(s), e, None, 70000, 1000, area.data_ptr() + 3)
    torch.cuda.synchronize()
    assert host_of(area)[3:1003] == d[70000:71000]


# ---- one huge block ---------------------------------------------------------------------------------
def test_one_huge_block(ctx):
    """One fixed-code block of 256 KiB: no checkpoint but entry 0, and a ranged read decodes from
    the stream's start (205000 bytes behind no window on one wavefront)."""
    d = dmx.corpus("text", 256 << 10)
    ix = Indexed(ctx, streams.single_fixed_block(d), d, 32768)
    got, outside_ok = ix.decoded()
    assert got == d and outside_ok
    assert ix.count == 1
    assert tuple(ix.entries[0]) == (0, 0, 0, NOWINDOW) and tuple(ix.entries[1]) == (8 * len(ix.stream), len(d), 0, 0)
    check_ranges(ctx, ix, [(200000, 5000)])


# ---- errors -----------------------------------------------------------------------------------------
def index_raw(ctx, ix, spacing, entry_cap, windows_cap, cap=None, n=None):
    """dmx_inflate_index_device with the caller's capacities -> (rc, count, out_len, output bytes,
    nothing outside the output touched)."""
    cap = len(ix.data) if cap is None else cap
    out, ooff = dev(bytes([FILL]) * cap, 9)
    ent = (dmx.SeekEntry * max(entry_cap, 1))()
    win = torch.full((max(windows_cap, 1),), FILL, dtype=torch.uint8, device="cuda")
    count, out_len = ctypes.c_size_t(12345), ctypes.c_size_t()
    rc = dmx.lib().dmx_inflate_index_device(ctx.h, ctypes.c_void_p(ix.d_in), len(ix.stream) if n is None else n,
                                            ctypes.c_void_p(out.data_ptr() + ooff), cap, spacing, ent, entry_cap,
                                            ctypes.c_void_p(win.data_ptr()), windows_cap, ctypes.byref(count),
                                            ctypes.byref(out_len), None)
    torch.cuda.synchronize()
    h = host_of(out)
    outside = h[:ooff] + h[ooff + cap:]
    return rc, count.value, out_len.value, h[ooff:ooff + cap], outside == bytes([FILL]) * len(outside)


def test_index_capacities_and_arguments(ctx):
    ix = foreign(ctx, "text", 1)
    c, d = ix.count, ix.data
    # one entry short (the sentinel does not fit), one window slot short: the count comes back
    # and the decoded bytes stand
    for ecap, wcap in ((c, c * W), (c + 1, c * W - 1), (0, 0)):
        rc, count, out_len, got, outside_ok = index_raw(ctx, ix, ix.spacing, ecap, wcap)
        assert rc == dmx.DMX_ERR_CAPACITY and count == c, (ecap, wcap, rc, count)
        assert out_len == len(d) and got == d and outside_ok
    rc, count, out_len, got, outside_ok = index_raw(ctx, ix, ix.spacing, c + 1, c * W)
    assert rc == dmx.DMX_OK and count == c and got == d and outside_ok
    # an output buffer one byte short: dmx_inflate_device's behaviour
    out, ooff = dev(bytes([FILL]) * (len(d) - 1), 9)
    st, err = status_of(ctx.inflate_device, ix.d_in, len(ix.stream), out.data_ptr() + ooff, len(d) - 1)
    assert st == dmx.DMX_ERR_CAPACITY
    rc, count, out_len, got, outside_ok = index_raw(ctx, ix, ix.spacing, c + 1, c * W, cap=len(d) - 1)
    assert rc == dmx.DMX_ERR_CAPACITY and out_len == len(d) and outside_ok
    # a spacing below the window
    rc, _, _, got, outside_ok = index_raw(ctx, ix, 1000, c + 1, c * W)
    assert rc == dmx.DMX_ERR_ARG and got == bytes([FILL]) * len(d) and outside_ok
    # a truncated stream: dmx_inflate_device's error
    cut = len(ix.stream) * 2 // 3
    out, ooff = dev(bytes([FILL]) * len(d), 9)
    st, _ = status_of(ctx.inflate_device, ix.d_in, cut, out.data_ptr() + ooff, len(d))
    assert st in (dmx.DMX_ERR_OVERREAD, dmx.DMX_ERR_DATA)
    rc, _, _, _, outside_ok = index_raw(ctx, ix, ix.spacing, c + 1, c * W, n=cut)
    assert rc == st and outside_ok


def test_range_errors(ctx):
    ix = foreign(ctx, "text", 1)
    e, total, n = ix.entries, len(ix.data), len(ix.stream)

    def arg_error(u, ln, entries=None, n=None):
        st, got, guard_ok = read(ctx, ix, u, ln, entries, n)
        return st == dmx.DMX_ERR_ARG and guard_ok and got == bytes([FILL]) * ln

    assert arg_error(total, 1) and arg_error(total - 1, 2) and arg_error(total + 1, 0) and arg_error(0, total + 1)
    # n cut to half the stream: the sentinel's bit lies beyond 8 n, whatever the range
    assert arg_error(total - 1000, 1000, n=n // 2) and arg_error(0, 10, n=n // 2)
    assert arg_error(0, 10, n=n - 1)
    bad = e.copy()
    bad[2, 1] = bad[1, 1]  # not strictly increasing
    assert arg_error(0, 10, bad)
    bad = e.copy()
    bad[3, 1] = bad[4, 1] + 1
    assert arg_error(0, 10, bad)
    bad = e.copy()
    bad[-1, 1] = bad[-2, 1] - 1  # the sentinel before the last entry
    assert arg_error(0, 10, bad)
    bad = e.copy()
    bad[2, 2] = 32767  # no NOWINDOW and not a whole window
    assert arg_error(0, 10, bad)
    bad[2, 2] = 0
    assert arg_error(0, 10, bad)
    # the sentinel claims 100 plain bytes more than the stream holds: the final block ends before
    # the last span's byte count
    lie = e.copy()
    lie[-1, 1] += 100
    st, _, guard_ok = read(ctx, ix, total - 100, 200, lie)
    assert st == dmx.DMX_ERR_DATA and guard_ok
    # ... and the bytes the stream does hold are still read correctly through that index
    st, got, guard_ok = read(ctx, ix, total - 100, 100, lie)
    assert st == dmx.DMX_OK and got == ix.data[-100:] and guard_ok


# ---- existing behaviour --------------------------------------------------------------------------------
def test_decompress_is_unchanged_around_an_index_call(ctx):
    cases = [(zraw(dmx.corpus(kind, 4 << 20, offset=99), lvl), dmx.corpus(kind, 4 << 20, offset=99), 5, 262144)
             for kind, lvl in FOREIGN]
    d = dmx.corpus("mixed", 1 << 20)
    cases += [(ctx.compress(d, 2), d, 4, 65536), (ctx.compress(d, 0), d, 4, 65536)]
    for s, d, path, spacing in cases:
        before = ctx.decompress(s)
        path_before = ctx.stats().path
        ix = Indexed(ctx, s, d, spacing)
        after = ctx.decompress(s)
        assert before == after == d
        assert path_before == ctx.stats().path == path == ix.path
