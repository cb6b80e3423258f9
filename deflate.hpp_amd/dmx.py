"""Python binding of libdmx's C-ABI (include/dmx.h) via ctypes.

Mirrors the reference's public API names (deflate::compress / inflate::decompress /
inflate::decompressZlib, /root/reference/include/deflate.hpp:755-815, inflate.hpp:326-408)
so tests read like the reference's own; errors raise ``DmxError`` (a ``RuntimeError``, as the
reference throws ``std::runtime_error``).  The HIP library is mandatory: there is no CPU
fallback, an import without ``lib/libdmx.so`` fails loudly.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# DMX_LIB: developer override (A/B runs of two builds); the default is the in-tree build
LIB_PATH = os.environ.get("DMX_LIB") or os.path.join(HERE, "lib", "libdmx.so")

DMX_OK = 0
DMX_ERR_ARG = -1
DMX_ERR_NOMEM = -2
DMX_ERR_DEVICE = -3
DMX_ERR_DATA = -4
DMX_ERR_OVERREAD = -5
DMX_ERR_CAPACITY = -6
DMX_ERR_CHECKSUM = -8
DMX_CFG_RFC_STRICT = 1
DMX_CFG_FB_SERIAL = 2
DMX_VERIFY = 1
DMX_DEFLATE_NOT_FINAL = 1
DMX_BATCH_NO_ROUTE = 1
DMX_BATCH_VERIFY = 2
DMX_BATCH_DEFERRED = 1  # per-buffer status of inflate_batch_async: decode it with inflate_device
DMX_FRAME_ZLIB = 1
DMX_FRAME_GZIP = 2
DMX_FRAME_BGZF = 3
FRAME = {"zlib": DMX_FRAME_ZLIB, "gzip": DMX_FRAME_GZIP, "bgzf": DMX_FRAME_BGZF}
DMX_ZIP_FORCE64 = 1
DMX_SEEK_WINDOW = 32768
DMX_SEEK_NOWINDOW = 1  # dmx_seek_entry.flags: nothing before the entry is referenced
BATCH_PATH = 6  # dmx_batch_result.path of a stream the batch decoder took

CORPUS = {"zeros": 0, "repeat": 1, "random": 2, "text": 3, "mixed": 4, "bmp": 5}

# every symbol include/dmx.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "dmx_config_default", "dmx_create", "dmx_destroy", "dmx_default_ctx", "dmx_deflate_bound",
    "dmx_deflate", "dmx_inflate", "dmx_inflate_alloc", "dmx_free", "dmx_strerror",
    "dmx_deflate_device", "dmx_inflate_device", "dmx_set_timing", "dmx_last_stats",
    "dmx_corpus_generate", "dmx_adler32_device", "dmx_crc32_device", "dmx_adler32", "dmx_crc32",
    "dmx_framed_bound", "dmx_deflate_zlib", "dmx_deflate_gzip", "dmx_inflate_zlib", "dmx_inflate_gzip",
    "dmx_deflate_file", "dmx_inflate_file", "dmx_segment_starts_device", "dmx_inflate_piece_device",
    "dmx_segment_check_device", "dmx_set_default_config", "dmx_deflate_device_async",
    "dmx_inflate_device_async", "dmx_deflate_batch_device", "dmx_inflate_batch_device",
    "dmx_deflate_batch", "dmx_inflate_batch", "dmx_deflate_batch_dict_device",
    "dmx_inflate_batch_dict_device", "dmx_deflate_batch_dict", "dmx_inflate_batch_dict",
    "dmx_batch_framed_bound", "dmx_deflate_batch_framed_device", "dmx_inflate_batch_framed_device",
    "dmx_deflate_batch_framed", "dmx_inflate_batch_framed", "dmx_bgzf_bound", "dmx_deflate_bgzf",
    "dmx_inflate_bgzf", "dmx_deflate_bgzf_device", "dmx_bgzf_index_device", "dmx_inflate_bgzf_device",
    "dmx_inflate_bgzf_range_device", "dmx_batch_reserve", "dmx_deflate_batch_async", "dmx_inflate_batch_async",
    "dmx_seek_windows_bound", "dmx_inflate_index_device", "dmx_inflate_range_device",
    "dmx_inflate_gzip_members_device", "dmx_inflate_gzip_members",
    "dmx_zip_index_device", "dmx_zip_extract_device", "dmx_inflate_zip_device", "dmx_zip_index", "dmx_inflate_zip",
    "dmx_zip_bound", "dmx_zip_write_device", "dmx_zip_write",
]


class DmxError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"{what}: {strerror(code)} ({code})" if what else f"{strerror(code)} ({code})")


class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("segment_bytes", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("n_gpus", ctypes.c_uint32), ("dev_inflate_pass", ctypes.c_uint32),
                ("dev_heavy_bytes", ctypes.c_uint32)]


class Stats(ctypes.Structure):
    _fields_ = [("ms_main_kernel", ctypes.c_double), ("ms_device_total", ctypes.c_double),
                ("segments", ctypes.c_uint64), ("in_bytes", ctypes.c_uint64),
                ("out_bytes", ctypes.c_uint64), ("path", ctypes.c_uint32), ("shards", ctypes.c_uint32)]


class BatchResult(ctypes.Structure):
    """dmx_batch_result: one buffer's outcome of a batch call."""
    _fields_ = [("bytes", ctypes.c_uint64), ("status", ctypes.c_int32), ("path", ctypes.c_uint32)]


class BgzfEntry(ctypes.Structure):
    """dmx_bgzf_entry: a member's start in the BGZF file and in the plain bytes."""
    _fields_ = [("coffset", ctypes.c_uint64), ("uoffset", ctypes.c_uint64)]


class ZipEntry(ctypes.Structure):
    """dmx_zip_entry: one entry of a ZIP archive's central directory, 64 bytes."""
    _fields_ = [("name_off", ctypes.c_uint64), ("data_off", ctypes.c_uint64), ("csize", ctypes.c_uint64),
                ("usize", ctypes.c_uint64), ("uoffset", ctypes.c_uint64), ("crc", ctypes.c_uint32),
                ("dostime", ctypes.c_uint32), ("name_len", ctypes.c_uint16), ("method", ctypes.c_uint16),
                ("gpflags", ctypes.c_uint16), ("reserved", ctypes.c_uint16), ("status", ctypes.c_int32),
                ("path", ctypes.c_uint32)]


class ZipSource(ctypes.Structure):
    """dmx_zip_source: one entry to write -- its plain bytes (a device pointer for the device form), its
    name (host bytes), the method (0 stored, 8 deflated) and the DOS time (0: 1980-01-01), 40 bytes."""
    _fields_ = [("data", ctypes.c_void_p), ("n", ctypes.c_uint64), ("name", ctypes.c_char_p),
                ("name_len", ctypes.c_uint32), ("method", ctypes.c_uint16), ("reserved", ctypes.c_uint16),
                ("dostime", ctypes.c_uint32)]


class SeekEntry(ctypes.Structure):
    """dmx_seek_entry: a checkpoint of the seek index -- a block header's stream bit, the plain
    bytes before it, the valid bytes of its window slot (0 or 32768) and DMX_SEEK_* flags."""
    _fields_ = [("bit", ctypes.c_uint64), ("uoffset", ctypes.c_uint64), ("window", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


_lib = None


def lib():
    """Load libdmx.so (raises OSError when the HIP library has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    try:  # share torch's HIP runtime (same SONAME libamdhip64.so.7) instead of loading a second
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise OSError(f"{LIB_PATH} missing: build it with `make -C deflate.hpp_amd` "
                      "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    sz = ctypes.c_size_t
    vp = ctypes.c_void_p
    u8p = ctypes.POINTER(ctypes.c_uint8)
    L.dmx_config_default.argtypes = [ctypes.POINTER(Config)]
    L.dmx_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(Config)]
    L.dmx_destroy.argtypes = [vp]
    L.dmx_default_ctx.restype = vp
    L.dmx_deflate_bound.argtypes = [sz]
    L.dmx_deflate_bound.restype = sz
    L.dmx_deflate.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(sz)]
    L.dmx_inflate.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    L.dmx_inflate_alloc.argtypes = [vp, vp, sz, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
    L.dmx_free.argtypes = [vp]
    L.dmx_strerror.argtypes = [ctypes.c_int]
    L.dmx_strerror.restype = ctypes.c_char_p
    L.dmx_deflate_device.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_uint32, vp, sz, ctypes.POINTER(sz), vp]
    L.dmx_deflate_device_async.argtypes = [vp, vp, sz, ctypes.c_int, ctypes.c_uint32, vp, sz, vp, vp]
    L.dmx_set_default_config.argtypes = [ctypes.POINTER(Config)]
    L.dmx_inflate_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
    L.dmx_inflate_device_async.argtypes = [vp, vp, sz, vp, sz, vp, ctypes.c_uint32, vp]
    L.dmx_set_timing.argtypes = [vp, ctypes.c_int]
    L.dmx_last_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.dmx_corpus_generate.argtypes = [ctypes.c_int, ctypes.c_uint64, sz, vp]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for f in ("dmx_adler32_device", "dmx_crc32_device"):
        getattr(L, f).argtypes = [vp, vp, sz, ctypes.c_uint32, u32p, vp]
    for f in ("dmx_adler32", "dmx_crc32"):
        getattr(L, f).argtypes = [vp, vp, sz, ctypes.c_uint32, u32p]
    L.dmx_deflate_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(sz),
                                   ctypes.POINTER(sz)]
    L.dmx_inflate_file.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(sz)]
    L.dmx_segment_starts_device.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(sz), vp]
    L.dmx_inflate_piece_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
    L.dmx_segment_check_device.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_uint64), sz,
                                           ctypes.POINTER(ctypes.c_uint64), vp]
    L.dmx_framed_bound.argtypes = [sz]
    L.dmx_framed_bound.restype = sz
    for f in ("dmx_deflate_zlib", "dmx_deflate_gzip"):
        getattr(L, f).argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(sz)]
    for f in ("dmx_inflate_zlib", "dmx_inflate_gzip"):
        getattr(L, f).argtypes = [vp, vp, sz, ctypes.c_uint32, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
    brp = ctypes.POINTER(BatchResult)
    L.dmx_deflate_batch_device.argtypes = [vp, vp, vp, sz, ctypes.c_int, vp, vp, brp, vp]
    L.dmx_inflate_batch_device.argtypes = [vp, vp, vp, sz, vp, vp, brp, ctypes.c_uint32, vp]
    L.dmx_deflate_batch.argtypes = [vp, vp, vp, sz, ctypes.c_int, vp, vp, brp]
    L.dmx_inflate_batch.argtypes = [vp, vp, vp, sz, vp, vp, brp, ctypes.c_uint32]
    L.dmx_deflate_batch_dict_device.argtypes = [vp, vp, vp, sz, ctypes.c_int, vp, sz, vp, vp, brp, vp]
    L.dmx_inflate_batch_dict_device.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, brp, ctypes.c_uint32, vp]
    L.dmx_deflate_batch_dict.argtypes = [vp, vp, vp, sz, ctypes.c_int, vp, sz, vp, vp, brp]
    L.dmx_inflate_batch_dict.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, brp, ctypes.c_uint32]
    u32 = ctypes.c_uint32
    L.dmx_batch_framed_bound.argtypes = [u32, sz]
    L.dmx_batch_framed_bound.restype = sz
    L.dmx_deflate_batch_framed_device.argtypes = [vp, vp, vp, sz, ctypes.c_int, u32, vp, vp, brp, vp]
    L.dmx_inflate_batch_framed_device.argtypes = [vp, vp, vp, sz, u32, vp, vp, brp, u32, vp]
    L.dmx_deflate_batch_framed.argtypes = [vp, vp, vp, sz, ctypes.c_int, u32, vp, vp, brp]
    L.dmx_inflate_batch_framed.argtypes = [vp, vp, vp, sz, u32, vp, vp, brp, u32]
    L.dmx_batch_reserve.argtypes = [vp, sz, sz, sz, sz]
    L.dmx_deflate_batch_async.argtypes = [vp, vp, vp, sz, sz, sz, ctypes.c_int, vp, sz, vp, vp, vp, vp]
    L.dmx_inflate_batch_async.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, u32, vp]
    L.dmx_bgzf_bound.argtypes = [sz]
    L.dmx_bgzf_bound.restype = sz
    L.dmx_deflate_bgzf.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(sz)]
    L.dmx_inflate_bgzf.argtypes = [vp, vp, sz, u32, ctypes.POINTER(u8p), ctypes.POINTER(sz)]
    u64 = ctypes.c_uint64
    bep = ctypes.POINTER(BgzfEntry)
    L.dmx_deflate_bgzf_device.argtypes = [vp, vp, sz, ctypes.c_int, vp, sz, ctypes.POINTER(sz), vp]
    L.dmx_bgzf_index_device.argtypes = [vp, vp, sz, bep, sz, ctypes.POINTER(sz), ctypes.POINTER(u64), vp]
    L.dmx_inflate_bgzf_device.argtypes = [vp, vp, sz, u32, vp, sz, ctypes.POINTER(sz), vp]
    L.dmx_inflate_bgzf_range_device.argtypes = [vp, vp, sz, bep, sz, u64, sz, u32, vp, vp]
    L.dmx_inflate_gzip_members_device.argtypes = [vp, vp, sz, u32, vp, sz, bep, sz, ctypes.POINTER(sz),
                                                  ctypes.POINTER(sz), vp]
    L.dmx_inflate_gzip_members.argtypes = [vp, vp, sz, u32, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    zep = ctypes.POINTER(ZipEntry)
    L.dmx_zip_index_device.argtypes = [vp, vp, sz, zep, sz, ctypes.POINTER(sz), ctypes.POINTER(u64), vp]
    L.dmx_zip_extract_device.argtypes = [vp, vp, sz, zep, sz, ctypes.POINTER(sz), sz, u32, vp, sz, brp,
                                         ctypes.POINTER(sz), vp]
    L.dmx_inflate_zip_device.argtypes = [vp, vp, sz, u32, vp, sz, zep, sz, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
    L.dmx_zip_index.argtypes = [vp, vp, sz, zep, sz, ctypes.POINTER(sz), ctypes.POINTER(u64)]
    L.dmx_inflate_zip.argtypes = [vp, vp, sz, u32, vp, sz, zep, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    zsp = ctypes.POINTER(ZipSource)
    L.dmx_zip_bound.argtypes = [zsp, sz, sz, u32]
    L.dmx_zip_bound.restype = sz
    L.dmx_zip_write_device.argtypes = [vp, zsp, sz, ctypes.c_int, u32, vp, sz, vp, sz, zep, ctypes.POINTER(sz), vp]
    L.dmx_zip_write.argtypes = [vp, zsp, sz, ctypes.c_int, u32, vp, sz, vp, sz, zep, ctypes.POINTER(sz)]
    sep = ctypes.POINTER(SeekEntry)
    L.dmx_seek_windows_bound.argtypes = [sz, sz]
    L.dmx_seek_windows_bound.restype = sz
    L.dmx_inflate_index_device.argtypes = [vp, vp, sz, vp, sz, sz, sep, sz, vp, sz, ctypes.POINTER(sz),
                                           ctypes.POINTER(sz), vp]
    L.dmx_inflate_range_device.argtypes = [vp, vp, sz, sep, sz, vp, u64, sz, vp, vp]
    _lib = L
    return L


def strerror(code):
    try:
        return lib().dmx_strerror(code).decode()
    except OSError:
        return f"error {code}"


def _check(rc, what):
    if rc != DMX_OK:
        raise DmxError(rc, what)


def deflate_bound(n):
    return lib().dmx_deflate_bound(n)


def zip_sources(ptrs, sizes, names, methods=None, dostimes=None):
    """The ZipSource array of a write call: names are bytes (str: encoded as UTF-8), methods default
    to 8 (deflated), dostimes to 0 (1980-01-01 00:00:00).  The array keeps the names alive."""
    k = len(ptrs)
    names = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
    arr = (ZipSource * max(k, 1))()
    for i in range(k):
        arr[i].data = ptrs[i] or None
        arr[i].n = sizes[i]
        arr[i].name = names[i]
        arr[i].name_len = len(names[i])
        arr[i].method = 8 if methods is None else methods[i]
        arr[i].dostime = 0 if dostimes is None else dostimes[i]
    arr._names = names
    return arr


def zip_bound(sizes, names, methods=None, comment=b"", force64=False):
    """dmx_zip_bound: no archive written from these entries is longer."""
    src = zip_sources([0] * len(sizes), sizes, names, methods)
    return lib().dmx_zip_bound(src, len(sizes), len(comment), DMX_ZIP_FORCE64 if force64 else 0)


def seek_windows_bound(cap, spacing=262144):
    """Bytes of window slots that hold the seek index of any stream of at most cap plain bytes."""
    return lib().dmx_seek_windows_bound(cap, spacing)


def corpus(kind, n, offset=0):
    """Synthetic corpus bytes [offset, offset+n)."""
    buf = ctypes.create_string_buffer(max(1, n))
    _check(lib().dmx_corpus_generate(CORPUS[kind], offset, n, buf), "corpus")
    return buf.raw[:n]


def corpus_into(kind, n, ptr, offset=0):
    _check(lib().dmx_corpus_generate(CORPUS[kind], offset, n, ctypes.c_void_p(ptr)), "corpus")


class Context:
    """A libdmx context bound to one HIP device (dmx_create / dmx_destroy)."""

    def __init__(self, device=-1, segment_bytes=32768, rfc_strict=False, n_gpus=1, **dev):
        """dev: developer A/B controls -- inflate_pass=k forces pass k of the segmented inflate
        plan, heavy_bytes=b sets the lane decoder's heavy-candidate threshold, fb_serial=True
        makes the block-parallel path decode every unit with one wavefront."""
        cfg = Config()
        lib().dmx_config_default(ctypes.byref(cfg))
        cfg.device = device
        cfg.segment_bytes = segment_bytes
        cfg.flags = DMX_CFG_RFC_STRICT if rfc_strict else 0
        cfg.n_gpus = n_gpus
        if dev.get("fb_serial"):
            cfg.flags |= DMX_CFG_FB_SERIAL
        if dev.get("inflate_pass") is not None:
            cfg.dev_inflate_pass = int(dev["inflate_pass"]) + 1
        cfg.dev_heavy_bytes = int(dev.get("heavy_bytes") or 0)
        h = ctypes.c_void_p()
        _check(lib().dmx_create(ctypes.byref(h), ctypes.byref(cfg)), "dmx_create")
        self.h = h

    def close(self):
        if self.h:
            lib().dmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer API: the reference's signatures -------------------------------------
    def compress(self, data, level=2):
        """deflate::compress(char*, size_t, int) -> raw DEFLATE bytes."""
        data = bytes(data)
        cap = deflate_bound(len(data))
        out = ctypes.create_string_buffer(max(1, cap))
        n = ctypes.c_size_t()
        _check(lib().dmx_deflate(self.h, data, len(data), level, out, cap, ctypes.byref(n)), "deflate")
        return out.raw[: n.value]

    def compress_raw_not_final(self, data, level=2):
        """One shard of a larger stream (DMX_DEFLATE_NOT_FINAL: no BFINAL, ends byte-aligned on
        an empty stored block), through the device API."""
        import torch
        data = bytes(data)
        d_in = torch.frombuffer(bytearray(data or b"\0"), dtype=torch.uint8).cuda()
        cap = deflate_bound(len(data)) + 64
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        n = self.deflate_device(d_in.data_ptr(), len(data), level, d_out.data_ptr(), cap, not_final=True)
        torch.cuda.synchronize()
        return d_out[:n].cpu().numpy().tobytes()

    def decompress(self, data, cap=None):
        """inflate::decompress(void*, size_t) -> bytes; with cap: the (void*,size_t,void*,size_t)
        overload (returns at most cap bytes)."""
        data = bytes(data)
        if cap is None:
            p = ctypes.POINTER(ctypes.c_uint8)()
            n = ctypes.c_size_t()
            _check(lib().dmx_inflate_alloc(self.h, data, len(data), ctypes.byref(p), ctypes.byref(n)), "inflate")
            try:
                return ctypes.string_at(p, n.value)
            finally:
                lib().dmx_free(p)
        out = ctypes.create_string_buffer(max(1, cap))
        w = ctypes.c_size_t()
        tot = ctypes.c_size_t()
        _check(lib().dmx_inflate(self.h, data, len(data), out, cap, ctypes.byref(w), ctypes.byref(tot)), "inflate")
        return out.raw[: w.value]

    def decompress_zlib(self, data):
        """inflate::decompressZlib(void*, size_t): skips the 2-byte zlib header (the reference's
        FDICT test never fires, inflate.hpp:355, SURVEY A-9) and ignores the Adler-32."""
        data = bytes(data)
        if len(data) < 2:
            raise DmxError(DMX_ERR_OVERREAD, "inflate_zlib")
        return self.decompress(data[2:])

    # ---- file-path overloads (streaming, deflate.hpp:755-777 / inflate.hpp:390-408) ------
    def compress_file(self, in_path, out_path, level=2):
        """deflate::compress(std::string, std::string, int); returns (input, output) sizes."""
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().dmx_deflate_file(self.h, os.fsencode(in_path), os.fsencode(out_path), level,
                                      ctypes.byref(a), ctypes.byref(b)), "deflate_file")
        return a.value, b.value

    def decompress_file(self, in_path, out_path):
        """inflate::decompress(std::string, std::string); returns the decoded size."""
        n = ctypes.c_size_t()
        _check(lib().dmx_inflate_file(self.h, os.fsencode(in_path), os.fsencode(out_path), ctypes.byref(n)),
               "inflate_file")
        return n.value

    # ---- containers and checksums (extensions, not in the reference) -----
    def _framed(self, fn, data, level):
        data = bytes(data)
        cap = lib().dmx_framed_bound(len(data))
        out = ctypes.create_string_buffer(max(1, cap))
        n = ctypes.c_size_t()
        _check(getattr(lib(), fn)(self.h, data, len(data), level, out, cap, ctypes.byref(n)), fn)
        return out.raw[: n.value]

    def compress_zlib(self, data, level=2):
        """RFC 1950 zlib stream (Adler-32 computed on the GPU)."""
        return self._framed("dmx_deflate_zlib", data, level)

    def compress_gzip(self, data, level=2):
        """RFC 1952 gzip member (CRC-32 computed on the GPU)."""
        return self._framed("dmx_deflate_gzip", data, level)

    def _unframed(self, fn, data, verify):
        data = bytes(data)
        p = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t()
        _check(getattr(lib(), fn)(self.h, data, len(data), DMX_VERIFY if verify else 0, ctypes.byref(p),
                                  ctypes.byref(n)), fn)
        try:
            return ctypes.string_at(p, n.value)
        finally:
            lib().dmx_free(p)

    def inflate_zlib(self, data, verify=True):
        """zlib stream -> bytes; header checked, Adler-32 verified on the GPU (DMX_ERR_CHECKSUM)."""
        return self._unframed("dmx_inflate_zlib", data, verify)

    def inflate_gzip(self, data, verify=True):
        """gzip member -> bytes; CRC-32 and ISIZE verified on the GPU."""
        return self._unframed("dmx_inflate_gzip", data, verify)

    def _ck(self, fn, data, init):
        data = bytes(data)
        v = ctypes.c_uint32()
        _check(getattr(lib(), fn)(self.h, data, len(data), init, ctypes.byref(v)), fn)
        return v.value

    def adler32(self, data, init=1):
        return self._ck("dmx_adler32", data, init)

    def crc32(self, data, init=0):
        return self._ck("dmx_crc32", data, init)

    def adler32_device(self, d, n, init=1, stream=None):
        v = ctypes.c_uint32()
        _check(lib().dmx_adler32_device(self.h, ctypes.c_void_p(d), n, init, ctypes.byref(v),
                                        ctypes.c_void_p(stream) if stream else None), "adler32_device")
        return v.value

    def crc32_device(self, d, n, init=0, stream=None):
        v = ctypes.c_uint32()
        _check(lib().dmx_crc32_device(self.h, ctypes.c_void_p(d), n, init, ctypes.byref(v),
                                      ctypes.c_void_p(stream) if stream else None), "crc32_device")
        return v.value

    # ---- device-resident API --------------------------------------------------------------
    def deflate_device(self, d_in, n, level, d_out, cap, stream=None, not_final=False):
        out_len = ctypes.c_size_t()
        rc = lib().dmx_deflate_device(self.h, ctypes.c_void_p(d_in), n, level,
                                      DMX_DEFLATE_NOT_FINAL if not_final else 0,
                                      ctypes.c_void_p(d_out), cap, ctypes.byref(out_len),
                                      ctypes.c_void_p(stream) if stream else None)
        _check(rc, "deflate_device")
        return out_len.value

    def deflate_device_async(self, d_in, n, level, d_out, cap, d_len, stream=None, not_final=False):
        """Enqueue a device deflate; the stream length lands in the 8-byte device buffer d_len."""
        rc = lib().dmx_deflate_device_async(self.h, ctypes.c_void_p(d_in), n, level,
                                            DMX_DEFLATE_NOT_FINAL if not_final else 0,
                                            ctypes.c_void_p(d_out), cap, ctypes.c_void_p(d_len),
                                            ctypes.c_void_p(stream) if stream else None)
        _check(rc, "deflate_device_async")

    def inflate_device(self, d_in, n, d_out, cap, stream=None):
        out_len = ctypes.c_size_t()
        rc = lib().dmx_inflate_device(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                      ctypes.byref(out_len), ctypes.c_void_p(stream) if stream else None)
        _check(rc, "inflate_device")
        return out_len.value

    def inflate_device_async(self, d_in, n, d_out, cap, d_result, stream=None, piece=False):
        """Enqueue the lane-path inflate of a libdmx-layout stream; d_result (16 device bytes)
        receives {decoded bytes, status}; status 1: decode it with inflate_device instead."""
        rc = lib().dmx_inflate_device_async(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                            ctypes.c_void_p(d_result), 1 if piece else 0,
                                            ctypes.c_void_p(stream) if stream else None)
        _check(rc, "inflate_device_async")

    def inflate_piece_device(self, d_in, n, d_out, cap, stream=None):
        """inflate_device for one piece of a larger stream: a reference before the piece start
        raises (DMX_ERR_DATA) instead of copying nothing (multi-GPU scatter, shard.py)."""
        out_len = ctypes.c_size_t()
        rc = lib().dmx_inflate_piece_device(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap,
                                            ctypes.byref(out_len), ctypes.c_void_p(stream) if stream else None)
        _check(rc, "inflate_piece_device")
        return out_len.value

    def segment_check_device(self, d_in, n, starts, stream=None):
        """End byte of the segment at each start (None where it does not decode in piece mode)."""
        k = len(starts)
        if not k:
            return []
        a = (ctypes.c_uint64 * k)(*starts)
        e = (ctypes.c_uint64 * k)()
        _check(lib().dmx_segment_check_device(self.h, ctypes.c_void_p(d_in), n, a, k, e,
                                              ctypes.c_void_p(stream) if stream else None), "segment_check")
        return [None if x == 0xFFFFFFFFFFFFFFFF else x for x in e]

    def segment_starts_device(self, d_in, n, stream=None):
        """Candidate segment starts (bytes after each 00 00 FF FF) of a device-resident stream."""
        cnt = ctypes.c_size_t()
        sp = ctypes.c_void_p(stream) if stream else None
        _check(lib().dmx_segment_starts_device(self.h, ctypes.c_void_p(d_in), n, None, 0, ctypes.byref(cnt), sp),
               "segment_starts")
        buf = (ctypes.c_uint64 * max(1, cnt.value))()
        _check(lib().dmx_segment_starts_device(self.h, ctypes.c_void_p(d_in), n, buf, cnt.value, ctypes.byref(cnt),
                                               sp), "segment_starts")
        return list(buf[: cnt.value])

    # ---- batched API: many independent buffers per call -----------------------------------
    @staticmethod
    def _batch_arrays(ptrs, sizes, out_ptrs, caps):
        k = len(ptrs)
        if not (len(sizes) == len(out_ptrs) == len(caps) == k):
            raise ValueError("batch arrays differ in length")
        m = max(1, k)
        return (k, (ctypes.c_void_p * m)(*ptrs), (ctypes.c_size_t * m)(*sizes), (ctypes.c_void_p * m)(*out_ptrs),
                (ctypes.c_size_t * m)(*caps), (BatchResult * m)())

    def deflate_batch_device(self, ptrs, sizes, level, out_ptrs, caps, stream=None, dict_ptr=None, dict_len=0):
        """dmx_deflate_batch_device: device pointers / sizes per buffer -> [(bytes, status, path)].
        Buffer i gets exactly the stream deflate_device writes for it alone.  dict_ptr / dict_len:
        a preset dictionary in device memory (dmx_deflate_batch_dict_device); the streams then
        decode with zlib.decompressobj(-15, zdict=...)."""
        k, a_in, a_n, a_out, a_cap, res = self._batch_arrays(ptrs, sizes, out_ptrs, caps)
        sp = ctypes.c_void_p(stream) if stream else None
        if dict_ptr is None and not dict_len:
            _check(lib().dmx_deflate_batch_device(self.h, a_in, a_n, k, level, a_out, a_cap, res, sp),
                   "deflate_batch_device")
        else:
            _check(lib().dmx_deflate_batch_dict_device(self.h, a_in, a_n, k, level, ctypes.c_void_p(dict_ptr),
                                                       dict_len, a_out, a_cap, res, sp), "deflate_batch_dict_device")
        return [(r.bytes, r.status, r.path) for r in res[:k]]

    def inflate_batch_device(self, ptrs, sizes, out_ptrs, caps, stream=None, no_route=False, dict_ptr=None,
                             dict_len=0):
        """dmx_inflate_batch_device -> [(bytes, status, path)]; no_route: every stream on the
        batch decoder, however long (developer A/B).  dict_ptr / dict_len: the preset dictionary
        the streams were made with, in device memory (dmx_inflate_batch_dict_device)."""
        k, a_in, a_n, a_out, a_cap, res = self._batch_arrays(ptrs, sizes, out_ptrs, caps)
        fl = DMX_BATCH_NO_ROUTE if no_route else 0
        sp = ctypes.c_void_p(stream) if stream else None
        if dict_ptr is None and not dict_len:
            _check(lib().dmx_inflate_batch_device(self.h, a_in, a_n, k, a_out, a_cap, res, fl, sp),
                   "inflate_batch_device")
        else:
            _check(lib().dmx_inflate_batch_dict_device(self.h, a_in, a_n, k, ctypes.c_void_p(dict_ptr), dict_len,
                                                       a_out, a_cap, res, fl, sp), "inflate_batch_dict_device")
        return [(r.bytes, r.status, r.path) for r in res[:k]]

    # ---- asynchronous batches: the descriptor arrays live in device memory -------------------
    def batch_reserve(self, count, max_n, max_total=0, dict_len=0):
        """dmx_batch_reserve: grow the scratch for async batches of this shape now (may allocate
        and synchronise), so that the calls themselves only enqueue."""
        _check(lib().dmx_batch_reserve(self.h, count, max_n, max_total, dict_len), "batch_reserve")

    def deflate_batch_async(self, d_in, d_n, count, max_n, level, d_out, d_cap, d_res, max_total=0, dict_ptr=None,
                            dict_len=0, stream=None):
        """dmx_deflate_batch_async: d_in / d_n / d_out / d_cap are device arrays of `count` 64-bit
        entries, d_res a device array of count x 16 bytes (batch_results reads it); all raw device
        pointers.  Enqueues on `stream` and returns: no result is known before the caller
        synchronises.  max_n bounds every size, max_total their sum (0: unknown)."""
        _check(lib().dmx_deflate_batch_async(self.h, ctypes.c_void_p(d_in), ctypes.c_void_p(d_n), count, max_n,
                                             max_total, level, ctypes.c_void_p(dict_ptr) if dict_ptr else None,
                                             dict_len, ctypes.c_void_p(d_out), ctypes.c_void_p(d_cap),
                                             ctypes.c_void_p(d_res), ctypes.c_void_p(stream) if stream else None),
               "deflate_batch_async")

    def inflate_batch_async(self, d_in, d_n, count, max_n, d_out, d_cap, d_res, no_route=False, dict_ptr=None,
                            dict_len=0, stream=None):
        """dmx_inflate_batch_async: arrays as in deflate_batch_async.  Without no_route (and without
        a dictionary) a stream above the routing threshold is not decoded: its status is
        DMX_BATCH_DEFERRED and the caller decodes it with inflate_device."""
        _check(lib().dmx_inflate_batch_async(self.h, ctypes.c_void_p(d_in), ctypes.c_void_p(d_n), count, max_n,
                                             ctypes.c_void_p(dict_ptr) if dict_ptr else None, dict_len,
                                             ctypes.c_void_p(d_out), ctypes.c_void_p(d_cap), ctypes.c_void_p(d_res),
                                             DMX_BATCH_NO_ROUTE if no_route else 0,
                                             ctypes.c_void_p(stream) if stream else None),
               "inflate_batch_async")

    def _batch_host(self, fn, datas, caps, mid=(), tail=()):
        datas = [bytes(d) for d in datas]
        k = len(datas)
        ins = [ctypes.create_string_buffer(d, max(1, len(d))) for d in datas]
        outs = [ctypes.create_string_buffer(max(1, c)) for c in caps]
        _, a_in, a_n, a_out, a_cap, res = self._batch_arrays(
            [ctypes.addressof(b) for b in ins], [len(d) for d in datas], [ctypes.addressof(b) for b in outs], caps)
        args = (self.h, a_in, a_n, k) + mid + (a_out, a_cap, res) + tail
        _check(getattr(lib(), fn)(*args), fn)
        return outs, res[:k]

    def compress_batch(self, datas, level=2, zdict=None):
        """Raw DEFLATE stream of every buffer in one call: equal to [compress(d, level) ...].
        zdict: a preset dictionary shared by all buffers, as zlib.compressobj's zdict."""
        caps = [deflate_bound(len(d)) for d in datas]
        if zdict is None:
            outs, res = self._batch_host("dmx_deflate_batch", datas, caps, mid=(level,))
        else:
            zdict = bytes(zdict)
            outs, res = self._batch_host("dmx_deflate_batch_dict", datas, caps, mid=(level, zdict, len(zdict)))
        for r in res:
            _check(r.status, "deflate_batch")
        return [o.raw[: r.bytes] for o, r in zip(outs, res)]

    def decompress_batch(self, datas, caps, zdict=None, no_route=False, with_results=False):
        """Inflate every stream in one call.  caps[i] bounds output i; each element is the
        decoded bytes, or the DmxError that decompress would raise for that stream alone
        (DMX_ERR_CAPACITY when it needs more than caps[i]).  zdict: the preset dictionary the
        streams were made with, as zlib.decompressobj's zdict.  with_results: also the list of
        (bytes, status, path) per stream."""
        fl = DMX_BATCH_NO_ROUTE if no_route else 0
        if zdict is None:
            outs, res = self._batch_host("dmx_inflate_batch", datas, list(caps), tail=(fl,))
        else:
            zdict = bytes(zdict)
            outs, res = self._batch_host("dmx_inflate_batch_dict", datas, list(caps), mid=(zdict, len(zdict)),
                                         tail=(fl,))
        vals = [o.raw[: r.bytes] if r.status == DMX_OK else DmxError(r.status, "inflate_batch")
                for o, r in zip(outs, res)]
        return (vals, [(r.bytes, r.status, r.path) for r in res]) if with_results else vals

    # ---- framed batch calls: zlib / gzip / BGZF around the batched API ---------------------
    def deflate_batch_framed_device(self, ptrs, sizes, level, out_ptrs, caps, format="gzip", stream=None):
        """dmx_deflate_batch_framed_device -> [(bytes, status, path)]: buffer i gets the zlib stream
        / gzip member compress_zlib / compress_gzip gives for it alone, or one BGZF member."""
        k, a_in, a_n, a_out, a_cap, res = self._batch_arrays(ptrs, sizes, out_ptrs, caps)
        _check(lib().dmx_deflate_batch_framed_device(self.h, a_in, a_n, k, level, FRAME[format], a_out, a_cap, res,
                                                     ctypes.c_void_p(stream) if stream else None),
               "deflate_batch_framed_device")
        return [(r.bytes, r.status, r.path) for r in res[:k]]

    def inflate_batch_framed_device(self, ptrs, sizes, out_ptrs, caps, format="gzip", verify=True, no_route=False,
                                    stream=None):
        """dmx_inflate_batch_framed_device -> [(bytes, status, path)]; verify: check every trailer
        on the GPU (DMX_BATCH_VERIFY)."""
        k, a_in, a_n, a_out, a_cap, res = self._batch_arrays(ptrs, sizes, out_ptrs, caps)
        fl = (DMX_BATCH_VERIFY if verify else 0) | (DMX_BATCH_NO_ROUTE if no_route else 0)
        _check(lib().dmx_inflate_batch_framed_device(self.h, a_in, a_n, k, FRAME[format], a_out, a_cap, res, fl,
                                                     ctypes.c_void_p(stream) if stream else None),
               "inflate_batch_framed_device")
        return [(r.bytes, r.status, r.path) for r in res[:k]]

    def compress_batch_framed(self, datas, level=2, format="gzip"):
        """zlib stream / gzip member / BGZF member of every buffer in one call: for "zlib" and
        "gzip" equal to [compress_zlib(d, level) ...] / [compress_gzip(d, level) ...]."""
        fmt = FRAME[format]
        caps = [lib().dmx_batch_framed_bound(fmt, len(d)) for d in datas]
        outs, res = self._batch_host("dmx_deflate_batch_framed", datas, caps, mid=(level, fmt))
        for r in res:
            _check(r.status, "deflate_batch_framed")
        return [o.raw[: r.bytes] for o, r in zip(outs, res)]

    def decompress_batch_framed(self, datas, caps, format="gzip", verify=True, no_route=False, with_results=False):
        """Inflate every framed buffer in one call; elements as in decompress_batch: the decoded
        bytes, or the DmxError that inflate_zlib / inflate_gzip would raise for that buffer alone."""
        fl = (DMX_BATCH_VERIFY if verify else 0) | (DMX_BATCH_NO_ROUTE if no_route else 0)
        outs, res = self._batch_host("dmx_inflate_batch_framed", datas, list(caps), mid=(FRAME[format],), tail=(fl,))
        vals = [o.raw[: r.bytes] if r.status == DMX_OK else DmxError(r.status, "inflate_batch_framed")
                for o, r in zip(outs, res)]
        return (vals, [(r.bytes, r.status, r.path) for r in res]) if with_results else vals

    def compress_bgzf(self, data, level=2):
        """A BGZF file: members of 65280 input bytes plus the empty EOF member (dmx_deflate_bgzf)."""
        data = bytes(data)
        cap = lib().dmx_bgzf_bound(len(data))
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_size_t()
        _check(lib().dmx_deflate_bgzf(self.h, data, len(data), level, out, cap, ctypes.byref(n)), "deflate_bgzf")
        return out.raw[: n.value]

    def decompress_bgzf(self, data, verify=True):
        """BGZF file -> bytes, all members in one batch call (dmx_inflate_bgzf)."""
        return self._unframed("dmx_inflate_bgzf", data, verify)

    # ---- BGZF files in device memory ------------------------------------------------------
    @staticmethod
    def _check_needed(rc, what, needed):
        """_check; a DMX_ERR_CAPACITY error carries the size that was needed as .needed"""
        if rc != DMX_OK:
            e = DmxError(rc, what)
            e.needed = needed if rc == DMX_ERR_CAPACITY else None
            raise e

    def deflate_bgzf_device(self, d_in, n, level, d_out, cap, stream=None):
        """The BGZF file compress_bgzf gives for the n bytes at device pointer d_in, written at
        device pointer d_out -> its size (dmx_deflate_bgzf_device; bgzf_bound(n) bounds it)."""
        out_len = ctypes.c_size_t()
        rc = lib().dmx_deflate_bgzf_device(self.h, ctypes.c_void_p(d_in), n, level, ctypes.c_void_p(d_out), cap,
                                           ctypes.byref(out_len), ctypes.c_void_p(stream) if stream else None)
        self._check_needed(rc, "deflate_bgzf_device", out_len.value)
        return out_len.value

    def bgzf_index_device(self, d_in, n, stream=None):
        """The member index of a BGZF file in device memory, found on the GPU without decoding
        (dmx_bgzf_index_device) -> (members + 1, 2) uint64 array: row k = member k's start in the
        file and in the plain bytes, the last row the sentinel (n, plain bytes)."""
        import numpy as np
        sp = ctypes.c_void_p(stream) if stream else None
        m = ctypes.c_size_t()
        _check(lib().dmx_bgzf_index_device(self.h, ctypes.c_void_p(d_in), n, None, 0, ctypes.byref(m), None, sp),
               "bgzf_index_device")
        idx = np.zeros((m.value + 1, 2), dtype=np.uint64)
        _check(lib().dmx_bgzf_index_device(self.h, ctypes.c_void_p(d_in), n,
                                           idx.ctypes.data_as(ctypes.POINTER(BgzfEntry)), m.value + 1,
                                           ctypes.byref(m), None, sp), "bgzf_index_device")
        return idx

    def inflate_bgzf_device(self, d_in, n, d_out, cap, verify=True, stream=None):
        """decompress_bgzf of the file at device pointer d_in, into device pointer d_out -> the
        plain size (dmx_inflate_bgzf_device)."""
        out_len = ctypes.c_size_t()
        rc = lib().dmx_inflate_bgzf_device(self.h, ctypes.c_void_p(d_in), n, DMX_VERIFY if verify else 0,
                                           ctypes.c_void_p(d_out), cap, ctypes.byref(out_len),
                                           ctypes.c_void_p(stream) if stream else None)
        self._check_needed(rc, "inflate_bgzf_device", out_len.value)
        return out_len.value

    def inflate_bgzf_range_device(self, d_in, n, index, uoffset, length, d_out, verify=True, stream=None):
        """Bytes [uoffset, uoffset + length) of the plain file into device pointer d_out, decoding
        only the members that overlap them; index: what bgzf_index_device returned."""
        import numpy as np
        idx = np.ascontiguousarray(index, dtype=np.uint64)
        if idx.ndim != 2 or idx.shape[1] != 2 or idx.shape[0] < 1:
            raise ValueError("index must be an (m + 1, 2) array")
        _check(lib().dmx_inflate_bgzf_range_device(self.h, ctypes.c_void_p(d_in), n,
                                                   idx.ctypes.data_as(ctypes.POINTER(BgzfEntry)), idx.shape[0] - 1,
                                                   uoffset, length, DMX_VERIFY if verify else 0,
                                                   ctypes.c_void_p(d_out), ctypes.c_void_p(stream) if stream else None),
               "inflate_bgzf_range_device")

    # ---- multi-member gzip files ---------------------------------------------------------------
    def inflate_gzip_members_device(self, d_in, n, d_out, cap, verify=True, want_index=False, stream=None):
        """gzip.decompress of the gzip file (one or more members back to back, zero padding allowed)
        at device pointer d_in, into device pointer d_out (dmx_inflate_gzip_members_device) ->
        (plain bytes, members), with want_index also the (members + 1, 2) uint64 array of
        bgzf_index_device: row k = member k's first header byte and the plain bytes before it, the
        last row the sentinel (n, plain bytes).  A DMX_ERR_CAPACITY error carries the output size
        that was needed as .needed (0: not known)."""
        import numpy as np
        sp = ctypes.c_void_p(stream) if stream else None
        fl = DMX_VERIFY if verify else 0
        out_len, m = ctypes.c_size_t(), ctypes.c_size_t()
        ecap = 4096 if want_index else 0
        while True:
            idx = np.zeros((max(ecap, 1), 2), dtype=np.uint64)
            ent = idx.ctypes.data_as(ctypes.POINTER(BgzfEntry)) if want_index else None
            rc = lib().dmx_inflate_gzip_members_device(self.h, ctypes.c_void_p(d_in), n, fl, ctypes.c_void_p(d_out), cap,
                                                       ent, ecap, ctypes.byref(m), ctypes.byref(out_len), sp)
            if rc == DMX_ERR_CAPACITY and want_index and ecap < m.value + 1:  # the table was too small
                ecap = m.value + 1
                continue
            break
        self._check_needed(rc, "inflate_gzip_members_device", out_len.value)
        return (out_len.value, m.value, idx[:m.value + 1].copy()) if want_index else (out_len.value, m.value)

    def decompress_gzip_members(self, data, verify=True, cap=None):
        """gzip.decompress: a gzip file of one or more members -> bytes (dmx_inflate_gzip_members).
        cap=None starts at max(1 MiB, 8 * len(data)); on DMX_ERR_CAPACITY the call is repeated with
        the size needed where that is reported, else with twice the capacity, bounded by DEFLATE's
        largest expansion, 1032 * len(data) + 65536."""
        data = bytes(data)
        limit = 1032 * len(data) + 65536
        given = cap is not None
        cap = max(1 << 20, 8 * len(data)) if cap is None else cap
        while True:
            out = ctypes.create_string_buffer(max(cap, 1))
            n, m = ctypes.c_size_t(), ctypes.c_size_t()
            rc = lib().dmx_inflate_gzip_members(self.h, data, len(data), DMX_VERIFY if verify else 0, out, cap,
                                                ctypes.byref(m), ctypes.byref(n))
            if rc == DMX_ERR_CAPACITY and not given and cap < limit:
                cap = n.value if n.value > cap else min(2 * cap, limit)
                continue
            self._check_needed(rc, "inflate_gzip_members", n.value)
            return out.raw[: n.value]

    # ---- ZIP archives ----------------------------------------------------------------------------
    def zip_index_device(self, d_in, n, stream=None):
        """The central directory of the ZIP archive at device pointer d_in, read on the GPU without
        decoding anything (dmx_zip_index_device) -> (entries, plain_bytes): a ctypes array of
        ZipEntry in directory order and the sum of their plain sizes."""
        sp = ctypes.c_void_p(stream) if stream else None
        count, plain = ctypes.c_size_t(), ctypes.c_uint64()
        ecap = 4096
        while True:
            ent = (ZipEntry * ecap)()
            rc = lib().dmx_zip_index_device(self.h, ctypes.c_void_p(d_in), n, ent, ecap, ctypes.byref(count),
                                            ctypes.byref(plain), sp)
            if rc == DMX_ERR_CAPACITY and ecap < count.value:  # the table was too small
                ecap = count.value
                continue
            break
        _check(rc, "zip_index_device")
        return (ZipEntry * count.value).from_buffer(ent), plain.value

    def zip_extract_device(self, d_in, n, entries, d_out, cap, sel=None, verify=True, stream=None):
        """The entries sel (indices into entries; None: all, in order) of the archive at device
        pointer d_in, back to back at device pointer d_out (dmx_zip_extract_device) -> (out_len,
        results): the layout's size and one BatchResult per selected entry.  A DMX_ERR_CAPACITY
        error carries the output size that was needed as .needed."""
        count = len(entries)
        nsel = count if sel is None else len(sel)
        sel_arr = None if sel is None else (ctypes.c_size_t * max(nsel, 1))(*sel)
        res = (BatchResult * max(nsel, 1))()
        out_len = ctypes.c_size_t()
        rc = lib().dmx_zip_extract_device(self.h, ctypes.c_void_p(d_in), n, entries, count, sel_arr, nsel,
                                          DMX_VERIFY if verify else 0, ctypes.c_void_p(d_out), cap, res,
                                          ctypes.byref(out_len), ctypes.c_void_p(stream) if stream else None)
        self._check_needed(rc, "zip_extract_device", out_len.value)
        return out_len.value, res[:nsel]

    def inflate_zip_device(self, d_in, n, d_out, cap, verify=True, stream=None):
        """Index plus extract-all of the archive at device pointer d_in into device pointer d_out
        (dmx_inflate_zip_device) -> (out_len, entries): entry k's bytes are d_out[uoffset, uoffset
        + usize) where its status is DMX_OK.  A DMX_ERR_CAPACITY error for the output carries the
        size that was needed as .needed."""
        sp = ctypes.c_void_p(stream) if stream else None
        fl = DMX_VERIFY if verify else 0
        count, out_len = ctypes.c_size_t(), ctypes.c_size_t()
        ecap = 4096
        while True:
            ent = (ZipEntry * ecap)()
            rc = lib().dmx_inflate_zip_device(self.h, ctypes.c_void_p(d_in), n, fl, ctypes.c_void_p(d_out), cap, ent,
                                              ecap, ctypes.byref(count), ctypes.byref(out_len), sp)
            if rc == DMX_ERR_CAPACITY and ecap < count.value:  # the table was too small
                ecap = count.value
                continue
            break
        self._check_needed(rc, "inflate_zip_device", out_len.value)
        return out_len.value, (ZipEntry * count.value).from_buffer(ent)

    def unzip(self, data, names=None, verify=True):
        """zipfile.ZipFile(...).read for every entry (names: only those) of the archive `data` ->
        dict name -> bytes.  Names are decoded as UTF-8 when flag bit 11 is set, else cp437, as
        zipfile does; of entries with the same name the last one is taken.  A per-entry failure
        raises DmxError with the entry's name."""
        import torch
        data = bytes(data)
        arc = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(
            0, dtype=torch.uint8, device="cuda")
        entries, plain = self.zip_index_device(arc.data_ptr(), len(data))
        decoded = [data[e.name_off:e.name_off + e.name_len].decode("utf-8" if e.gpflags & 0x800 else "cp437")
                   for e in entries]
        last = {name: k for k, name in enumerate(decoded)}
        if names is None:
            sel = sorted(last.values())
        else:
            missing = [x for x in names if x not in last]
            if missing:
                raise KeyError(f"no entry named {missing[0]!r} in the archive")
            sel = [last[x] for x in names]
        need = sum(entries[k].usize for k in sel)
        out = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        _, res = self.zip_extract_device(arc.data_ptr(), len(data), entries, out.data_ptr(), need, sel=sel,
                                         verify=verify)
        host = out.cpu().numpy().tobytes()
        got, at = {}, 0
        for k, r in zip(sel, res):
            if r.status != DMX_OK:
                raise DmxError(r.status, f"unzip: entry {decoded[k]!r}")
            got[decoded[k]] = host[at:at + entries[k].usize]
            at += entries[k].usize
        return got

    def zip_write_device(self, ptrs, sizes, names, d_out, cap, level=2, methods=None, dostimes=None, comment=b"",
                         force64=False, stream=None):
        """A ZIP archive of the buffers at device pointers ptrs, written at device pointer d_out
        (dmx_zip_write_device) -> (bytes, entries): the archive's size and the ZipEntry rows
        zip_index_device reads back from it.  names: bytes or str (UTF-8); methods: 8 (deflated, the
        default) or 0 (stored) per entry.  A DMX_ERR_CAPACITY error carries the size that was needed
        as .needed; zip_bound(sizes, names, ...) is always enough."""
        k = len(ptrs)
        src = zip_sources(ptrs, sizes, names, methods, dostimes)
        comment = bytes(comment)
        ent = (ZipEntry * max(k, 1))()
        out_len = ctypes.c_size_t()
        rc = lib().dmx_zip_write_device(self.h, src, k, level, DMX_ZIP_FORCE64 if force64 else 0, comment,
                                        len(comment), ctypes.c_void_p(d_out), cap, ent, ctypes.byref(out_len),
                                        ctypes.c_void_p(stream) if stream else None)
        self._check_needed(rc, "zip_write_device", out_len.value)
        return out_len.value, (ZipEntry * k).from_buffer(ent)

    def zip(self, members, level=2, stored=(), comment=b"", force64=False):
        """The inverse of unzip: members, a dict or a list of (name, bytes), -> the archive's bytes
        (dmx_zip_write).  Entries are deflated at `level` but for the names in `stored`."""
        items = [(k, bytes(v)) for k, v in (members.items() if isinstance(members, dict) else members)]
        bufs = [ctypes.create_string_buffer(v, max(1, len(v))) for _, v in items]
        sizes = [len(v) for _, v in items]
        names = [k for k, _ in items]
        methods = [0 if k in stored else 8 for k in names]
        src = zip_sources([ctypes.addressof(b) for b in bufs], sizes, names, methods)
        comment = bytes(comment)
        fl = DMX_ZIP_FORCE64 if force64 else 0
        cap = lib().dmx_zip_bound(src, len(items), len(comment), fl)
        out = ctypes.create_string_buffer(max(1, cap))
        out_len = ctypes.c_size_t()
        rc = lib().dmx_zip_write(self.h, src, len(items), level, fl, comment, len(comment), out, cap, None,
                                 ctypes.byref(out_len))
        self._check_needed(rc, "zip_write", out_len.value)
        return out.raw[:out_len.value]

    # ---- seek index and ranged reads for unblocked streams ---------------------------------
    def inflate_index_device(self, d_in, n, d_out, cap, spacing=262144, stream=None):
        """inflate_device plus the seek index (dmx_inflate_index_device), one call with buffers
        sized by cap -> (out_len, entries, windows): entries a (count + 1, 4) uint64 array of
        (bit, uoffset, window, flags), the last row the sentinel; windows a uint8 CUDA tensor whose
        slot k, bytes [k * 32768, (k + 1) * 32768), goes with row k.  A DMX_ERR_CAPACITY error
        carries the output size that was needed as .needed."""
        import numpy as np
        import torch
        wcap = seek_windows_bound(cap, spacing)
        ecap = wcap // DMX_SEEK_WINDOW + 1
        windows = torch.empty(max(wcap, 1), dtype=torch.uint8, device="cuda")
        ent = (SeekEntry * max(ecap, 1))()
        count, out_len = ctypes.c_size_t(), ctypes.c_size_t()
        rc = lib().dmx_inflate_index_device(self.h, ctypes.c_void_p(d_in), n, ctypes.c_void_p(d_out), cap, spacing,
                                            ent, ecap, ctypes.c_void_p(windows.data_ptr()), wcap,
                                            ctypes.byref(count), ctypes.byref(out_len),
                                            ctypes.c_void_p(stream) if stream else None)
        self._check_needed(rc, "inflate_index_device", out_len.value)
        rows = [(e.bit, e.uoffset, e.window, e.flags) for e in ent[:count.value + 1]]
        return out_len.value, np.array(rows, dtype=np.uint64).reshape(-1, 4), windows[:count.value * DMX_SEEK_WINDOW]

    def inflate_range_device(self, d_in, n, entries, windows, uoffset, length, d_out, stream=None):
        """Plain bytes [uoffset, uoffset + length) into device pointer d_out, decoding only from
        the checkpoints that cover them (dmx_inflate_range_device); entries and windows: what
        inflate_index_device returned for the stream (windows: a tensor, a device pointer or None)."""
        import numpy as np
        idx = np.ascontiguousarray(entries, dtype=np.uint64)
        if idx.ndim != 2 or idx.shape[1] != 4 or idx.shape[0] < 1:
            raise ValueError("entries must be a (count + 1, 4) array")
        ent = (SeekEntry * idx.shape[0])(*[SeekEntry(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF,
                                                     int(r[3]) & 0xFFFFFFFF) for r in idx])
        wp = windows.data_ptr() if hasattr(windows, "data_ptr") else windows
        _check(lib().dmx_inflate_range_device(self.h, ctypes.c_void_p(d_in), n, ent, idx.shape[0] - 1,
                                              ctypes.c_void_p(wp) if wp else None, uoffset, length,
                                              ctypes.c_void_p(d_out), ctypes.c_void_p(stream) if stream else None),
               "inflate_range_device")

    def set_timing(self, on=True):
        _check(lib().dmx_set_timing(self.h, 1 if on else 0), "set_timing")

    def stats(self):
        s = Stats()
        _check(lib().dmx_last_stats(self.h, ctypes.byref(s)), "stats")
        return s


_default = None


def batch_results(tensor):
    """The d_res array of an async batch call -- a uint8 CUDA tensor of count x 16 bytes -- as
    [(bytes, status, path)]; the caller has synchronised."""
    raw = tensor.detach().cpu().contiguous().numpy().tobytes()
    if len(raw) % ctypes.sizeof(BatchResult):
        raise ValueError("not a whole number of dmx_batch_result records")
    res = (BatchResult * (len(raw) // ctypes.sizeof(BatchResult))).from_buffer_copy(raw)
    return [(r.bytes, r.status, r.path) for r in res]


def default_context():
    global _default
    if _default is None:
        _default = Context()
    return _default


def compress(data, level=2):
    return default_context().compress(data, level)


def decompress(data, cap=None):
    return default_context().decompress(data, cap)


def decompress_zlib(data):
    return default_context().decompress_zlib(data)


def bgzf_bound(n):
    return lib().dmx_bgzf_bound(n)


def gzi_bytes(index):
    """htslib's .gzi file for an index of Context.bgzf_index_device: a little-endian u64 count,
    then the (compressed offset, uncompressed offset) pair of every member but the first; the
    sentinel row is not stored."""
    import struct
    rows = [(int(c), int(u)) for c, u in index][1:-1]
    return struct.pack("<Q", len(rows)) + b"".join(struct.pack("<QQ", c, u) for c, u in rows)
