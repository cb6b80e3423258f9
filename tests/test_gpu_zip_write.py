"""GPU: writing ZIP archives -- dmx_zip_write_device, dmx_zip_write, dmx_zip_bound, Context.zip
(csrc/zip_write.hip, csrc/host_zip_write.cpp).

The oracle is Python's zipfile on the written archive, the project's own reader (Context.unzip,
zip_index_device) and, for a deflated payload, the batch deflate of the same bytes.  Inputs and
output sit at offsets 0, 1 and 7 mod 16 inside canary-filled tensors: the inputs are unchanged
after every call and the canaries intact."""
import ctypes
import functools
import io
import zipfile

import numpy as np
import pytest
import torch

import dmx
import zip_cases as zc
import zip_write_cases as zw

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
MODS = [(0, 0), (1, 7), (7, 1)]
FIELDS = [f for f, _ in dmx.ZipEntry._fields_]


def dev_inputs(datas, mod):
    """every buffer inside one FILL-filled device tensor, buffer k at an offset that is mod + 5 k
    modulo 16 (mod 0: every buffer aligned), 16 bytes of canary at least between two -> (tensor,
    offsets)"""
    host, offs = bytearray([FILL]) * PAD, []
    for k, d in enumerate(datas):
        host += bytes([FILL]) * (-len(host) % 16 + ((mod + 5 * k) % 16 if mod else 0))
        offs.append(len(host))
        host += d
        host += bytes([FILL]) * 16
    host += bytes([FILL]) * PAD
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, offs


def host_of(t):
    return t.cpu().numpy().tobytes()


def status_of(fn, *a, **k):
    try:
        return dmx.DMX_OK, fn(*a, **k)
    except dmx.DmxError as e:
        return e.code, e


def bound_of(members, comment=b"", force64=False):
    return dmx.zip_bound([len(d) for _, d, _, _ in members], [n for n, *_ in members], [m for _, _, m, _ in members],
                         comment=comment, force64=force64)


def write(ctx, members, level=2, force64=False, mods=(1, 7), cap=None, comment=b"", c=None):
    """dmx_zip_write_device with canaries around the inputs and the output -> (status, (bytes,
    entries) or the error, the output area's cap bytes)"""
    t, offs = dev_inputs([d for _, d, _, _ in members], mods[0])
    before = host_of(t)
    cap = bound_of(members, comment, force64) if cap is None else cap
    ooff = PAD + mods[1]
    out = torch.full((ooff + cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    st, val = status_of((c or ctx).zip_write_device, [t.data_ptr() + o for o in offs], [len(d) for _, d, _, _ in members],
                        [n for n, *_ in members], out.data_ptr() + ooff, cap, level=level,
                        methods=[m for _, _, m, _ in members], dostimes=[ts for *_, ts in members], comment=comment,
                        force64=force64)
    torch.cuda.synchronize()
    assert host_of(t) == before  # the inputs are only read
    h = host_of(out)
    used = val[0] if st == dmx.DMX_OK else 0
    assert h[:ooff] == bytes([FILL]) * ooff and h[ooff + used:] == bytes([FILL]) * (len(h) - ooff - used), \
        "a write outside the archive"
    return st, val, h[ooff:ooff + cap]


def index_of(ctx, archive):
    t = torch.frombuffer(bytearray(archive), dtype=torch.uint8).cuda()
    return ctx.zip_index_device(t.data_ptr(), len(archive))[0]


def rows_equal(a, b):
    return len(a) == len(b) and all([getattr(x, f) for f in FIELDS] == [getattr(y, f) for f in FIELDS] for x, y in zip(a, b))


def round_trip_members():
    return zw.mixed() + zw.non_ascii()


@pytest.mark.parametrize("force64", [False, True], ids=["classic", "force64"])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_round_trip(ctx, level, force64):
    members = round_trip_members()
    want = {n.decode("utf-8"): d for n, d, _, _ in members}
    comment = b"written on the device"
    for mods in MODS:
        st, val, area = write(ctx, members, level=level, force64=force64, mods=mods, comment=comment)
        assert st == dmx.DMX_OK, val
        n, entries = val
        assert n <= bound_of(members, comment, force64)
        archive = area[:n]
        zw.check_with_zipfile(archive, members, comment)
        assert ctx.unzip(archive) == want
        assert rows_equal(index_of(ctx, archive), entries), mods
        assert (archive[-22 - len(comment) - 20:][:4] == b"PK\x06\x07") == force64
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        assert np.load(io.BytesIO(z.read("array.npy")))[29, 99] == 2999.0


def test_empty_and_one_entry(ctx):
    st, val, area = write(ctx, [], cap=64)
    assert st == dmx.DMX_OK and val[0] == 22 and len(val[1]) == 0 and area[:22] == zc.write_zip([])
    st, val, area = write(ctx, [], cap=128, comment=b"only a comment", force64=True)
    assert st == dmx.DMX_OK and val[0] == 76 + 22 + 14
    with zipfile.ZipFile(io.BytesIO(area[:val[0]])) as z:
        assert z.namelist() == [] and z.comment == b"only a comment"
    for mods in MODS:
        st, val, area = write(ctx, zw.one(), mods=mods)
        assert st == dmx.DMX_OK
        zw.check_with_zipfile(area[:val[0]], zw.one())
        assert ctx.unzip(area[:val[0]]) == {"hello.txt": zc._text(5000)}


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_deterministic_and_the_batch_deflate_payload(ctx, level):
    members = round_trip_members()
    st, val, area = write(ctx, members, level=level, mods=(7, 1))
    assert st == dmx.DMX_OK
    st2, val2, area2 = write(ctx, members, level=level, mods=(0, 0))
    assert st2 == dmx.DMX_OK and val2[0] == val[0] and area2[:val[0]] == area[:val[0]]
    for (name, data, method, _), e in zip(members, val[1]):
        payload = area[e.data_off:e.data_off + e.csize]
        assert payload == (ctx.compress_batch([data], level)[0] if method == 8 else data), name


@functools.lru_cache(maxsize=None)
def large_members():
    return [(b"big/text.txt", dmx.corpus("text", 3 << 20), 8, zw.DOSTIME), (b"big/random.bin", zc._rand((1 << 20) + 5, 16), 0, 0),
            (b"small", zc._text(100, 17), 8, 0)]


@pytest.mark.parametrize("mods", MODS, ids=lambda m: f"in{m[0]}_out{m[1]}")
def test_large_entries(ctx, mods):
    """many chunks per entry: a deflated entry of 3 MiB, a stored one of 1 MiB + 5 bytes"""
    members = large_members()
    st, val, area = write(ctx, members, mods=mods)
    assert st == dmx.DMX_OK, val
    n, entries = val
    assert entries[0].csize > 4 * 65536 and entries[1].csize == (1 << 20) + 5
    zw.check_with_zipfile(area[:n], members)
    assert rows_equal(index_of(ctx, area[:n]), entries)


def test_65536_tiny_entries(ctx):
    members = zw.tiny(65536)
    st, val, area = write(ctx, members)
    assert st == dmx.DMX_OK, val
    n, entries = val
    archive = area[:n]
    assert archive[-42:-38] == b"PK\x06\x07" and len(entries) == 65536  # the ZIP64 end record came by itself
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        assert [x.encode() for x in z.namelist()] == [m[0] for m in members]
        for k in (0, 1, 4097, 65535):
            assert z.read(z.infolist()[k]) == members[k][1]
    assert ctx.unzip(archive) == {m[0].decode(): m[1] for m in members}
    assert rows_equal(index_of(ctx, archive), entries)


def test_capacity(ctx):
    members = zw.mixed()
    st, val, area = write(ctx, members)
    assert st == dmx.DMX_OK
    needed = val[0]
    for mods in MODS:
        st, err, area = write(ctx, members, cap=needed - 1, mods=mods)
        assert st == dmx.DMX_ERR_CAPACITY and err.needed == needed
        assert area == bytes([FILL]) * (needed - 1)  # nothing was written
    st, val, area = write(ctx, members, cap=needed)
    assert st == dmx.DMX_OK and val[0] == needed
    zw.check_with_zipfile(area, members)
    st, err, area = write(ctx, [], cap=21)
    assert st == dmx.DMX_ERR_CAPACITY and err.needed == 22 and area == bytes([FILL]) * 21


def test_argument_errors_leave_the_output_untouched(ctx):
    good = zw.one()[0]
    cap = 8192
    bad = {"method 1": [(b"a", b"abc", 1, 0)], "method 12": [good, (b"a", b"abc", 12, 0)],
           "empty name": [(b"", b"abc", 8, 0)], "name of 65536 bytes": [(b"n" * 65536, b"abc", 0, 0)]}
    for what, members in bad.items():
        st, err, area = write(ctx, members, cap=cap)
        assert st == dmx.DMX_ERR_ARG and area == bytes([FILL]) * cap, what
    st, err, area = write(ctx, [good], cap=cap, comment=b"c" * 65536)
    assert st == dmx.DMX_ERR_ARG and area == bytes([FILL]) * cap
    st, val, area = write(ctx, [good], cap=cap + 70000, comment=b"c" * 65535)
    assert st == dmx.DMX_OK and area[:val[0]].endswith(b"c" * 65535)
    # raw calls: a null data pointer with n > 0, unknown flags, a null context, a 64 KiB context
    out = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    t, offs = dev_inputs([good[1]], 1)
    n = ctypes.c_size_t(5)
    lib = dmx.lib()

    def raw(h, src, flags):
        rc = lib.dmx_zip_write_device(h, src, 1, 2, flags, None, 0, ctypes.c_void_p(out.data_ptr()), cap, None,
                                      ctypes.byref(n), None)
        torch.cuda.synchronize()
        assert host_of(out) == bytes([FILL]) * cap
        return rc

    ok = dmx.zip_sources([t.data_ptr() + offs[0]], [len(good[1])], [good[0]])
    assert raw(ctx.h, dmx.zip_sources([0], [3], [b"a"]), 0) == dmx.DMX_ERR_ARG
    assert raw(ctx.h, ok, 2) == dmx.DMX_ERR_ARG
    assert raw(None, ok, 0) == dmx.DMX_ERR_ARG
    c64 = dmx.Context(segment_bytes=65536)
    try:
        assert raw(c64.h, ok, 0) == dmx.DMX_ERR_ARG
        st, err, area = write(ctx, [good], cap=cap, c=c64)
        assert st == dmx.DMX_ERR_ARG and area == bytes([FILL]) * cap
    finally:
        c64.close()
    assert n.value == 5  # no call got as far as the size


def test_host_forms(ctx):
    members = {n.decode("utf-8"): d for n, d, _, _ in round_trip_members()}
    archive = ctx.zip(members, stored=("stored_17.bin", "dir/"), comment=b"host form")
    assert ctx.unzip(archive) == members
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        assert z.testzip() is None and z.comment == b"host form"
        assert {zi.filename: zi.compress_type for zi in z.infolist()} == \
            {k: (0 if k in ("stored_17.bin", "dir/") else 8) for k in members}
    assert ctx.unzip(ctx.zip(list(members.items()), level=0, force64=True)) == members
    assert ctx.zip({}) == zc.write_zip([])
    # an .npz made on the GPU
    arrays = {"a": np.arange(10000, dtype=np.float32).reshape(100, 100), "b": np.zeros(7, dtype=np.int64)}
    files = {}
    for k, v in arrays.items():
        buf = io.BytesIO()
        np.save(buf, v)
        files[k + ".npy"] = buf.getvalue()
    npz = np.load(io.BytesIO(ctx.zip(files)))
    assert sorted(npz.files) == ["a", "b"] and all(np.array_equal(npz[k], v) for k, v in arrays.items())
    # dmx_zip_write with a host buffer one byte short
    data = zc._text(5000)
    buf = ctypes.create_string_buffer(data, len(data))
    src = dmx.zip_sources([ctypes.addressof(buf)], [len(data)], [b"hello.txt"])
    n = ctypes.c_size_t()
    out = ctypes.create_string_buffer(bytes([FILL]) * 8192, 8192)
    lib = dmx.lib()
    assert lib.dmx_zip_write(ctx.h, src, 1, 2, 0, None, 0, out, 8192, None, ctypes.byref(n)) == dmx.DMX_OK
    needed = n.value
    assert out.raw[needed:] == bytes([FILL]) * (8192 - needed)
    zw.check_with_zipfile(out.raw[:needed], [(b"hello.txt", data, 8, 0)])
    short = ctypes.create_string_buffer(bytes([FILL]) * 8192, 8192)
    ent = (dmx.ZipEntry * 1)()
    assert lib.dmx_zip_write(ctx.h, src, 1, 2, 0, None, 0, short, needed - 1, ent, ctypes.byref(n)) == dmx.DMX_ERR_CAPACITY
    assert n.value == needed and short.raw == bytes([FILL]) * 8192
    assert lib.dmx_zip_write(ctx.h, src, 1, 2, 0, None, 0, short, needed, ent, ctypes.byref(n)) == dmx.DMX_OK
    assert short.raw[:needed] == out.raw[:needed] and ent[0].usize == 5000 and ent[0].status == 0
