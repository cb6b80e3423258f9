"""GPU: ZIP archives -- dmx_zip_index_device, dmx_zip_extract_device, dmx_inflate_zip_device, the host
forms dmx_zip_index / dmx_inflate_zip and Context.unzip (csrc/zip_dir.hip, csrc/host_zip.cpp).

The oracle is Python's zipfile (ZipFile.read, infolist).  The archive and the output sit at offsets
0, 1 and 7 mod 16 inside canary-filled tensors, checked after every call.  Every archive is built
once (tests/zip_cases.py caches them)."""
import ctypes
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest
import torch

import dmx
import zip_cases as zc

pytestmark = pytest.mark.gpu

FILL = 0xA5
PAD = 64
MODS = [(0, 0), (1, 7), (7, 1)]


def dev(data, mod=0, extra=0):
    """`data` at an offset that is `mod` modulo 16 inside a FILL-filled device tensor, PAD bytes of
    canary before it and PAD + extra behind -> (tensor, offset)."""
    off = PAD + mod
    host = bytearray([FILL]) * (off + len(data) + extra + PAD)
    host[off:off + len(data)] = data
    t = torch.frombuffer(host, dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t, off


def host_of(t):
    return t.cpu().numpy().tobytes()


def canaries_ok(h, off, used):
    return h[:off] == bytes([FILL]) * off and h[off + used:] == bytes([FILL]) * (len(h) - off - used)


def status_of(fn, *a, **k):
    try:
        return dmx.DMX_OK, fn(*a, **k)
    except dmx.DmxError as e:
        return e.code, e


def plain_size(archive):
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        return sum(zi.file_size for zi in z.infolist())


def inflate_zip(ctx, archive, verify=True, mod=1, omod=7, cap=None):
    """dmx_inflate_zip_device with canaries around the archive and the output -> (status, entries or
    the error, the output bytes)"""
    t, off = dev(archive, mod)
    before = host_of(t)
    cap = plain_size(archive) if cap is None else cap
    out, ooff = dev(bytes([FILL]) * cap, omod)
    st, val = status_of(ctx.inflate_zip_device, t.data_ptr() + off, len(archive), out.data_ptr() + ooff, cap,
                        verify=verify)
    torch.cuda.synchronize()
    assert host_of(t) == before  # the archive is only read
    h = host_of(out)
    used = val[0] if st == dmx.DMX_OK else 0
    assert canaries_ok(h, ooff, used if st == dmx.DMX_OK else cap), "a write outside the output"
    if st != dmx.DMX_OK:
        return st, val, h[ooff:ooff + cap]
    return st, val[1], h[ooff:ooff + used]


def check_against_zipfile(archive, entries, out, payloads=None):
    """every entry's fields against ZipInfo, its bytes against ZipFile.read (payloads: the bytes
    by entry index, where they are known without reading)"""
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        infos = z.infolist()
        assert len(entries) == len(infos)
        at = 0
        for k, (e, zi) in enumerate(zip(entries, infos)):
            h = zi.header_offset
            nl, el = struct.unpack("<HH", archive[h + 26:h + 30])
            assert (e.csize, e.usize, e.crc, e.method, e.gpflags) == (zi.compress_size, zi.file_size, zi.CRC,
                                                                       zi.compress_type, zi.flag_bits), k
            assert e.data_off == h + 30 + nl + el and e.uoffset == at and e.status == dmx.DMX_OK, k
            assert archive[e.name_off:e.name_off + e.name_len] == zi.orig_filename.encode(
                "utf-8" if zi.flag_bits & 0x800 else "cp437"), k
            d, t = zi.date_time, e.dostime
            assert ((t >> 25) + 1980, (t >> 21) & 15, (t >> 16) & 31, (t >> 11) & 31, (t >> 5) & 63,
                    (t & 31) * 2) == d, k
            if out is not None:
                want = payloads[k] if payloads is not None else z.read(zi)
                assert out[at:at + zi.file_size] == want, k
            at += zi.file_size
        assert out is None or len(out) == at


SMALL = {"empty": zc.empty, "one": zc.one_entry, "mixed": zc.mixed, "descriptors": zc.data_descriptors,
         "false_signatures": zc.false_signatures, "prepended": zc.prepended, "hand_zip64": zc.hand_zip64}


@pytest.mark.parametrize("mods", MODS, ids=lambda m: f"in{m[0]}_out{m[1]}")
@pytest.mark.parametrize("name", list(SMALL))
def test_extract_all(ctx, name, mods):
    archive = SMALL[name]()
    st, entries, out = inflate_zip(ctx, archive, mod=mods[0], omod=mods[1])
    assert st == dmx.DMX_OK, entries
    check_against_zipfile(archive, entries, out)
    for e in entries:
        assert e.path == (dmx.BATCH_PATH if e.method == 8 else 0)


@pytest.mark.parametrize("name", list(SMALL))
def test_index_alone(ctx, name):
    archive = SMALL[name]()
    t, off = dev(archive, 7)
    entries, plain = ctx.zip_index_device(t.data_ptr() + off, len(archive))
    assert host_of(t) == host_of(dev(archive, 7)[0])
    check_against_zipfile(archive, entries, None)
    assert plain == plain_size(archive)


TILE = 4096  # the candidate scan's tile (csrc/cand_scan.h)


def test_tile_edge_records(ctx):
    """A central record's signature starts 0-3 bytes before and behind a multiple of the scan's tile
    in the 16-byte aligned view of the directory region.  160 stored entries with 10-byte names give
    a directory of two tiles and a bit; the first entry's name length picks the record that lands
    there and its payload's length the region's place in the view."""
    count = 160
    for mod in (0, 5):
        for edge in (TILE, 2 * TILE):
            for delta in range(-3, 4):
                target = edge + delta
                # local entry: 30 + name + payload; central record: 46 + name
                pick = [(nl, pl) for nl in range(1, 57) for pl in range(1, 17)
                        if (target - (mod + 30 + nl + pl + (count - 1) * 41) % 16 - 46 - nl) % 56 == 0]
                nl, pl = pick[0]
                archive = zc.write_zip([("n" * nl, b"p" * pl, 0)] +
                                       [("e%09d" % k, b"x", 0) for k in range(1, count)])
                with zipfile.ZipFile(io.BytesIO(archive)) as z:
                    sizes = [46 + len(zi.orig_filename.encode()) + len(zi.extra) + len(zi.comment)
                             for zi in z.infolist()]
                    at = (mod + z.start_dir) % 16  # the region's first byte in its aligned view
                    starts = [at + sum(sizes[:k]) for k in range(count)]
                assert target in starts[1:] and starts[-1] + sizes[-1] > 2 * TILE, (mod, edge, delta)
                t, off = dev(archive, mod)
                entries, plain = ctx.zip_index_device(t.data_ptr() + off, len(archive))
                assert host_of(t) == host_of(dev(archive, mod)[0])
                check_against_zipfile(archive, entries, None)
                assert plain == plain_size(archive)


def test_mixed_archive_has_the_shapes():
    """stored entries of 0, 1, 15, 16, 17 and 4097 bytes, a deflated empty entry (03 00), a directory"""
    archive = zc.mixed()
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        infos = {zi.filename: zi for zi in z.infolist()}
    assert sorted(zi.file_size for zi in infos.values() if zi.compress_type == 0 and not zi.is_dir()) == \
        [0, 1, 15, 16, 17, 4097]
    e = infos["empty_deflated"]
    assert e.compress_type == 8 and e.compress_size == 2
    assert infos["dir/"].is_dir()
    assert all(zi.flag_bits & 8 for zi in zipfile.ZipFile(io.BytesIO(zc.data_descriptors())).infolist())


def test_3000_entries_with_name_lengths_1_to_200(ctx):
    archive = zc.many(3000, True)
    st, entries, out = inflate_zip(ctx, archive, mod=7, omod=1)
    assert st == dmx.DMX_OK
    assert sorted({e.name_len for e in entries}) == list(range(1, 201))
    check_against_zipfile(archive, entries, out)


def test_65536_tiny_entries(ctx):
    archive = zc.many(65536)
    assert archive[-42:-38] == b"PK\x06\x07"  # zipfile wrote the ZIP64 end record and its locator
    st, entries, out = inflate_zip(ctx, archive, mod=1, omod=7)
    assert st == dmx.DMX_OK and len(entries) == 65536
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        infos = z.infolist()
        assert z.read(infos[4097]) == out[entries[4097].uoffset:entries[4097].uoffset + entries[4097].usize]
    at = 0
    for e, zi in zip(entries, infos):  # (the payloads' CRCs stand in for 65536 ZipFile.read calls)
        assert (e.csize, e.usize, e.crc, e.method, e.uoffset, e.status) == \
            (zi.compress_size, zi.file_size, zi.CRC, zi.compress_type, at, 0)
        at += zi.file_size
    assert at == len(out)
    crcs = [zlib.crc32(out[e.uoffset:e.uoffset + e.usize]) for e in entries]
    assert crcs == [zi.CRC for zi in infos]


def test_deflated_entry_above_the_routing_threshold(ctx):
    archive = zc.big_deflated()
    st, entries, out = inflate_zip(ctx, archive, mod=7, omod=7)
    assert st == dmx.DMX_OK
    assert entries[1].csize > (1 << 20) and entries[1].path != dmx.BATCH_PATH and entries[1].path != 0
    assert entries[0].path == dmx.BATCH_PATH
    check_against_zipfile(archive, entries, out)


def test_stored_entry_above_the_routing_threshold(ctx):
    archive = zc.big_stored()
    for verify in (True, False):
        st, entries, out = inflate_zip(ctx, archive, verify=verify, mod=1, omod=1)
        assert st == dmx.DMX_OK
        assert entries[0].csize > (1 << 20) and entries[0].path == 0
        check_against_zipfile(archive, entries, out)


def test_npz_through_unzip(ctx):
    arrays = {"a": np.arange(10000, dtype=np.float32).reshape(100, 100), "b": np.zeros(7, dtype=np.int64),
              "c": np.random.default_rng(1).integers(0, 9, (33, 5)).astype(np.uint8)}
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    files = ctx.unzip(buf.getvalue())
    assert sorted(files) == ["a.npy", "b.npy", "c.npy"]
    for k, v in arrays.items():
        got = np.load(io.BytesIO(files[k + ".npy"]))
        assert got.dtype == v.dtype and np.array_equal(got, v)
    only = ctx.unzip(buf.getvalue(), names=["c.npy"])
    assert list(only) == ["c.npy"] and only["c.npy"] == files["c.npy"]


# ---- selections -----------------------------------------------------------------------------------
def extract(ctx, archive, entries, sel, verify=True, mod=7, omod=1, cap=None):
    t, off = dev(archive, mod)
    if cap is None:
        cap = sum(entries[k].usize for k in (range(len(entries)) if sel is None else sel))
    out, ooff = dev(bytes([FILL]) * cap, omod)
    st, val = status_of(ctx.zip_extract_device, t.data_ptr() + off, len(archive), entries, out.data_ptr() + ooff, cap,
                        sel=sel, verify=verify)
    torch.cuda.synchronize()
    h = host_of(out)
    assert canaries_ok(h, ooff, cap)
    return st, val, h[ooff:ooff + cap]


def test_selections(ctx):
    archive = zc.mixed()
    t, off = dev(archive, 0)
    entries, _ = ctx.zip_index_device(t.data_ptr() + off, len(archive))
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        want = [z.read(zi) for zi in z.infolist()]
    n = len(entries)
    for sel in ([n - 1, 7, 4, 0], [2, 0, 2, 10, 2], list(range(n))[::-1], []):
        st, val, out = extract(ctx, archive, entries, sel)
        assert st == dmx.DMX_OK, sel
        out_len, res = val
        assert out_len == sum(len(want[k]) for k in sel) and len(res) == len(sel)
        at = 0
        for k, r in zip(sel, res):  # the layout: the prefix sum of usize in selection order
            assert (r.status, r.bytes) == (dmx.DMX_OK, len(want[k])), (sel, k)
            assert out[at:at + len(want[k])] == want[k], (sel, k)
            at += len(want[k])
    st, val, out = extract(ctx, archive, entries, None)
    assert st == dmx.DMX_OK and out == b"".join(want)
    st, err, out = extract(ctx, archive, entries, [0, n], cap=100000)
    assert st == dmx.DMX_ERR_ARG and out == bytes([FILL]) * 100000


def test_stored_copy_at_every_alignment(ctx):
    """the copy kernel's paths: source and destination at every distance mod 16, entries shorter
    than the destination's lead-in, bodies with and without a tail"""
    data = [zc._rand(n, 40 + n) for n in (4097, 3, 16, 31, 64)]
    archive = zc.write_zip([(f"s{k}", d, zipfile.ZIP_STORED) for k, d in enumerate(data)])
    t0, off0 = dev(archive, 0)
    entries, _ = ctx.zip_index_device(t0.data_ptr() + off0, len(archive))
    assert all(e.method == 0 for e in entries)
    want = b"".join(data)
    for mod in range(16):
        for omod in (0, 1, 6, 11, 15):
            st, val, out = extract(ctx, archive, entries, None, mod=mod, omod=omod)
            assert st == dmx.DMX_OK and out == want, (mod, omod)
            assert all(r.status == dmx.DMX_OK and r.path == 0 for r in val[1])


# ---- failures, each with intact neighbours ------------------------------------------------------------
PAYLOADS = [zc._text(30000, 21), zc._rand(5000, 22), zc._rand(333, 23), zc._text(777, 24), zc._rand(4097, 25)]
METHODS = [8, 8, 0, 8, 0]  # (entry 1: random bytes deflated -- zlib keeps them in stored blocks)


def victims():
    return zc.write_zip([(f"v{k}", PAYLOADS[k], METHODS[k]) for k in range(5)])


def central_records(archive):
    """offsets of the central records, in order"""
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        at, out = z.start_dir, []
        for _ in z.infolist():
            assert archive[at:at + 4] == b"PK\x01\x02"
            out.append(at)
            nl, el, cl = struct.unpack("<HHH", archive[at + 28:at + 34])
            at += 46 + nl + el + cl
    return out


def local_data(archive, k):
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        h = z.infolist()[k].header_offset
    nl, el = struct.unpack("<HH", archive[h + 26:h + 30])
    return h, h + 30 + nl + el


def patched(archive, at, new):
    b = bytearray(archive)
    b[at:at + len(new)] = new
    return bytes(b)


def neighbours_intact(entries, out, bad):
    at = 0
    for k, e in enumerate(entries):
        if k != bad:
            assert e.status == dmx.DMX_OK, k
            assert out[at:at + e.usize] == PAYLOADS[k], k
        at += e.usize
    assert at == len(out)


@pytest.mark.parametrize("verify", [True, False])
def test_flipped_payload_byte(ctx, verify):
    good = victims()
    for k in (1, 2):  # a deflated entry (inside a stored block of its stream) and a stored entry
        _, d0 = local_data(good, k)
        at = d0 + 100
        archive = patched(good, at, bytes([good[at] ^ 0x40]))
        st, entries, out = inflate_zip(ctx, archive, verify=verify, cap=sum(map(len, PAYLOADS)))
        assert st == dmx.DMX_OK
        if verify:
            assert entries[k].status in (dmx.DMX_ERR_DATA, dmx.DMX_ERR_CHECKSUM)
        else:
            assert entries[k].status in (dmx.DMX_OK, dmx.DMX_ERR_DATA, dmx.DMX_ERR_CHECKSUM)
        neighbours_intact(entries, out, k)


@pytest.mark.parametrize("verify", [True, False])
def test_directory_crc_altered(ctx, verify):
    good = victims()
    for k in (0, 4):
        rec = central_records(good)[k]
        archive = patched(good, rec + 16, struct.pack("<I", zlib.crc32(PAYLOADS[k]) ^ 1))
        st, entries, out = inflate_zip(ctx, archive, verify=verify, cap=sum(map(len, PAYLOADS)))
        assert st == dmx.DMX_OK
        assert entries[k].status == (dmx.DMX_ERR_CHECKSUM if verify else dmx.DMX_OK)
        neighbours_intact(entries, out, k if verify else -1)


@pytest.mark.parametrize("verify", [True, False])
@pytest.mark.parametrize("delta", [-1, 1])
def test_directory_usize_off_by_one(ctx, verify, delta):
    good = victims()
    for k in (0, 3):
        rec = central_records(good)[k]
        archive = patched(good, rec + 24, struct.pack("<I", len(PAYLOADS[k]) + delta))
        st, entries, out = inflate_zip(ctx, archive, verify=verify, cap=sum(map(len, PAYLOADS)) + delta)
        assert st == dmx.DMX_OK
        assert entries[k].status == dmx.DMX_ERR_CHECKSUM and entries[k].usize == len(PAYLOADS[k]) + delta
        neighbours_intact(entries, out, k)


def test_unsupported_entries(ctx):
    good = victims()
    # flag bit 0 patched in (central record)
    rec = central_records(good)[3]
    archive = patched(good, rec + 8, struct.pack("<H", 1))
    st, entries, out = inflate_zip(ctx, archive, cap=sum(map(len, PAYLOADS)))
    assert st == dmx.DMX_OK and entries[3].status == dmx.DMX_ERR_ARG
    neighbours_intact(entries, out, 3)
    # a bzip2 entry between two others
    data = [zc._text(2000, 31), zc._text(5000, 32), zc._rand(100, 33)]
    archive = zc.write_zip([("a", data[0], zipfile.ZIP_DEFLATED), ("b", data[1], zipfile.ZIP_BZIP2),
                            ("c", data[2], zipfile.ZIP_STORED)])
    st, entries, out = inflate_zip(ctx, archive)
    assert st == dmx.DMX_OK
    assert [e.status for e in entries] == [dmx.DMX_OK, dmx.DMX_ERR_ARG, dmx.DMX_OK] and entries[1].method == 12
    assert out[:2000] == data[0] and out[7000:] == data[2]
    with pytest.raises(dmx.DmxError, match="'b'"):
        ctx.unzip(archive)
    assert ctx.unzip(archive, names=["c", "a"]) == {"c": data[2], "a": data[0]}


def test_destroyed_local_signature(ctx):
    good = victims()
    h, _ = local_data(good, 2)
    archive = patched(good, h, b"PK\x03\x05")
    st, entries, out = inflate_zip(ctx, archive, cap=sum(map(len, PAYLOADS)))
    assert st == dmx.DMX_OK and entries[2].status == dmx.DMX_ERR_DATA
    neighbours_intact(entries, out, 2)


def test_caller_edited_entry_overreads(ctx):
    archive = victims()
    t, off = dev(archive, 1)
    entries, _ = ctx.zip_index_device(t.data_ptr() + off, len(archive))
    for k, field, value in ((0, "csize", len(archive)), (2, "data_off", len(archive) - 100), (4, "data_off", 1 << 62)):
        edited = (dmx.ZipEntry * 5).from_buffer_copy(entries)
        setattr(edited[k], field, value)
        if METHODS[k] == 0 and field == "csize":
            edited[k].usize = value
        st, val, out = extract(ctx, archive, edited, None)
        assert st == dmx.DMX_OK
        res = val[1]
        assert res[k].status == dmx.DMX_ERR_OVERREAD
        at = 0
        for j in range(5):
            if j != k:
                assert res[j].status == dmx.DMX_OK and out[at:at + len(PAYLOADS[j])] == PAYLOADS[j], (k, j)
            at += len(PAYLOADS[j])


def test_broken_archives(ctx):
    good = victims()
    plain = sum(map(len, PAYLOADS))
    eocd = good.rfind(b"PK\x05\x06")
    # no end record
    st, err, out = inflate_zip(ctx, patched(good, eocd, b"PK\x05\x07"), cap=plain)
    assert st == dmx.DMX_ERR_DATA and out == bytes([FILL]) * plain
    # a directory cut short: one byte of it is gone, the end record states the old size
    rec = central_records(good)[-1]
    assert good[rec + 46:rec + 48] == b"v4"
    st, err, out = inflate_zip(ctx, good[:rec + 47] + good[rec + 48:], cap=plain)
    assert st == dmx.DMX_ERR_DATA and out == bytes([FILL]) * plain
    # a count that is off by one
    st, err, out = inflate_zip(ctx, patched(good, eocd + 8, struct.pack("<HH", 6, 6)), cap=plain)
    assert st == dmx.DMX_ERR_DATA
    # fewer than 22 bytes
    for n in (0, 21):
        t, off = dev(good[:n], 1)
        with pytest.raises(dmx.DmxError) as e:
            ctx.zip_index_device(t.data_ptr() + off, n)
        assert e.value.code == dmx.DMX_ERR_DATA


def test_capacity_one_byte_short(ctx):
    archive = victims()
    plain = sum(map(len, PAYLOADS))
    st, err, out = inflate_zip(ctx, archive, cap=plain - 1)
    assert st == dmx.DMX_ERR_CAPACITY and err.needed == plain
    assert out == bytes([FILL]) * (plain - 1)  # nothing was written
    t, off = dev(archive, 0)
    entries, _ = ctx.zip_index_device(t.data_ptr() + off, len(archive))
    st, err, out = extract(ctx, archive, entries, [4, 0], cap=len(PAYLOADS[4]) + len(PAYLOADS[0]) - 1)
    assert st == dmx.DMX_ERR_CAPACITY and err.needed == len(PAYLOADS[4]) + len(PAYLOADS[0])
    assert out == bytes([FILL]) * (len(PAYLOADS[4]) + len(PAYLOADS[0]) - 1)


# ---- host forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "prepended", "hand_zip64"])
def test_host_forms_match_the_device_forms(ctx, name):
    archive = SMALL[name]()
    st, dev_entries, dev_out = inflate_zip(ctx, archive)
    assert st == dmx.DMX_OK
    lib = dmx.lib()
    n = len(dev_entries)
    count, plain, out_len = ctypes.c_size_t(), ctypes.c_uint64(), ctypes.c_size_t()
    ent = (dmx.ZipEntry * n)()
    assert lib.dmx_zip_index(ctx.h, archive, len(archive), ent, n, ctypes.byref(count),
                             ctypes.byref(plain)) == dmx.DMX_OK
    assert count.value == n and plain.value == len(dev_out)
    fields = [f for f, _ in dmx.ZipEntry._fields_]
    for a, b in zip(ent, dev_entries):
        assert [getattr(a, f) for f in fields if f != "path"] == [getattr(b, f) for f in fields if f != "path"]
    ent2 = (dmx.ZipEntry * n)()
    out = ctypes.create_string_buffer(len(dev_out) + 16)
    assert lib.dmx_inflate_zip(ctx.h, archive, len(archive), dmx.DMX_VERIFY, out, len(dev_out), ent2, n,
                               ctypes.byref(count), ctypes.byref(out_len)) == dmx.DMX_OK
    assert count.value == n and out_len.value == len(dev_out) and out.raw[:out_len.value] == dev_out
    assert out.raw[out_len.value:] == bytes(16)
    for a, b in zip(ent2, dev_entries):
        assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields]
    assert lib.dmx_inflate_zip(ctx.h, archive, len(archive), 0, out, len(dev_out) - 1, ent2, n, ctypes.byref(count),
                               ctypes.byref(out_len)) == dmx.DMX_ERR_CAPACITY
    assert out_len.value == len(dev_out)
