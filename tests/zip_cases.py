"""ZIP archives for tests/test_zip_dir.py (CPU) and tests/test_gpu_zip.py: written with Python's
zipfile, which is also the oracle, plus one hand-packed archive whose central record carries
0xFFFFFFFF size and offset fields and a ZIP64 extra 0x0001."""
import functools
import io
import struct
import zipfile
import zlib

SIG_CENTRAL = b"PK\x01\x02"


def _rand(n, seed):
    """n reproducible bytes that do not compress"""
    import numpy as np
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _text(n, seed=0):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta"]
    out, k = bytearray(), seed
    while len(out) < n:
        k = (k * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[k % len(words)] + b" "
    return bytes(out[:n])


def write_zip(members, comment=b""):
    """members: (name, data, method) or (name, data, method, entry comment) -> archive bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for m in members:
            zi = zipfile.ZipInfo(m[0], date_time=(2024, 2, 29, 12, 34, 56))
            zi.compress_type = m[2]
            if len(m) > 3:
                zi.comment = m[3]
            if m[0].endswith("/"):
                zi.external_attr = 0x10
            z.writestr(zi, m[1])
        z.comment = comment
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def empty():
    return write_zip([])


@functools.lru_cache(maxsize=None)
def one_entry():
    return write_zip([("hello.txt", _text(5000), zipfile.ZIP_DEFLATED)])


@functools.lru_cache(maxsize=None)
def mixed():
    """deflated, stored (0, 1, 15, 16, 17, 4097 bytes), a deflated empty entry and a directory"""
    m = [("text.txt", _text(70000, 1), zipfile.ZIP_DEFLATED), ("dir/", b"", zipfile.ZIP_STORED)]
    for n in (0, 1, 15, 16, 17, 4097):
        m.append((f"stored_{n}.bin", _rand(n, n), zipfile.ZIP_STORED))
    m.append(("empty_deflated", b"", zipfile.ZIP_DEFLATED))
    m.append(("dir/random.bin", _rand(3000, 7), zipfile.ZIP_DEFLATED))
    m.append(("zeros", bytes(100000), zipfile.ZIP_DEFLATED))
    return write_zip(m)


class _Unseekable(io.RawIOBase):
    def __init__(self):
        self.buf = bytearray()

    def writable(self):
        return True

    def write(self, b):
        self.buf += b
        return len(b)


@functools.lru_cache(maxsize=None)
def data_descriptors():
    """written to an unseekable stream: flag bit 3, sizes and CRC behind the data"""
    raw = _Unseekable()
    with zipfile.ZipFile(raw, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("a.txt", _text(20000, 3))
        z.writestr("b.bin", _rand(1000, 4), compress_type=zipfile.ZIP_STORED)
        z.writestr("c.txt", _text(333, 5))
    return bytes(raw.buf)


@functools.lru_cache(maxsize=None)
def false_signatures():
    """names, entry comments and the archive comment hold 50 4b 01 02 with plausible lengths"""
    def fake(nl, el, cl):
        return SIG_CENTRAL + bytes(24) + struct.pack("<HHH", nl, el, cl) + bytes(12)
    name = "PK\x01\x02" + "A" * 24 + "\x01\x01" * 3 + "B" * 12  # (zipfile cuts a name at a NUL)
    members = [("first.txt", _text(900, 6), zipfile.ZIP_DEFLATED, fake(4, 0, 0) + b"tail"),
               (name, _text(100, 7), zipfile.ZIP_DEFLATED, fake(0, 0, 0)),
               ("third", _rand(64, 8), zipfile.ZIP_STORED, fake(10, 0, 36) + fake(0, 0, 0))]
    return write_zip(members, comment=fake(0, 0, 0) + b"between" + fake(1, 1, 1))


@functools.lru_cache(maxsize=None)
def prepended():
    """1 KiB in front of a finished archive (a self-extractor's stub): every stated offset is 1024 short"""
    return _rand(1024, 11) + write_zip([("x.txt", _text(3000, 9), zipfile.ZIP_DEFLATED),
                                        ("y.bin", _rand(50, 10), zipfile.ZIP_STORED)])


@functools.lru_cache(maxsize=None)
def many(count, name_lengths=False):
    """count tiny entries; name_lengths: names of 1..200 bytes"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:
        for k in range(count):
            # (name_lengths: one letter per round of 200, so no two names are equal)
            name = chr(97 + k // 200) * (1 + k % 200) if name_lengths else f"{k:x}"
            z.writestr(name, b"%d\n" % k if k % 3 else _text(40 + k % 50, k),
                       compress_type=zipfile.ZIP_DEFLATED if k % 3 == 0 else zipfile.ZIP_STORED)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def hand_zip64():
    """one deflated and one stored entry; the first central record reads 0xFFFFFFFF for csize, usize
    and the local header offset and carries them in a 0x0001 extra, the second only for usize"""
    plain = [_text(4000, 12), _rand(77, 13)]
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = [comp.compress(plain[0]) + comp.flush(), plain[1]]
    method = [8, 0]
    names = [b"big64.txt", b"small.bin"]
    out, offs = bytearray(b"junk"), []  # (the local headers do not start at 0)
    for k in range(2):
        offs.append(len(out))
        out += struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", 45, 0, method[k], 0, 0x5841, zlib.crc32(plain[k]),
                           len(raw[k]), len(plain[k]), len(names[k]), 0) + names[k] + raw[k]
    cd = len(out)
    x0 = struct.pack("<HHQQQ", 1, 24, len(plain[0]), len(raw[0]), offs[0])
    x0 = struct.pack("<HH", 0x7075, 3) + b"abc" + x0  # another subfield in front
    out += struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 45, 45, 0, 8, 0, 0x5841, zlib.crc32(plain[0]),
                       0xFFFFFFFF, 0xFFFFFFFF, len(names[0]), len(x0), 0, 0, 0, 0, 0xFFFFFFFF) + names[0] + x0
    x1 = struct.pack("<HHQ", 1, 8, len(plain[1]))
    out += struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\x01\x02", 45, 45, 0, 0, 0, 0x5841, zlib.crc32(plain[1]),
                       len(raw[1]), 0xFFFFFFFF, len(names[1]), len(x1), 0, 0, 0, 0, offs[1]) + names[1] + x1
    size = len(out) - cd
    out += struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, 2, 2, size, cd, 0)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def big_deflated():
    """one deflated entry just above 1 MiB compressed"""
    data = _rand((1 << 20) + 4096, 14)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=1) as z:
        z.writestr("small.txt", _text(100, 15))
        z.writestr("big.bin", data)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def big_stored():
    return write_zip([("big.bin", _rand((1 << 20) + 5, 16), zipfile.ZIP_STORED),
                      ("after.txt", _text(100, 17), zipfile.ZIP_DEFLATED)])


def table(archive):
    """what zipfile states about every entry: (header_offset, compress_size, file_size, CRC, method,
    data offset, flags)"""
    rows = []
    with zipfile.ZipFile(io.BytesIO(archive)) as z:
        for zi in z.infolist():
            h = zi.header_offset
            nl, el = struct.unpack("<HH", archive[h + 26:h + 30])
            rows.append((h, zi.compress_size, zi.file_size, zi.CRC, zi.compress_type, h + 30 + nl + el, zi.flag_bits))
    return rows


def table_text(archive):
    rows = table(archive)
    return "".join(f"{len(rows)}\n") + "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
