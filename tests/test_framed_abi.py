"""CPU: the framed batch and BGZF entry points of include/dmx.h exist, reject a null context, and
their bounds and constants are the header's.  No GPU work is launched here."""
import ctypes
import os
import re

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMED = ["dmx_batch_framed_bound", "dmx_deflate_batch_framed_device", "dmx_inflate_batch_framed_device",
          "dmx_deflate_batch_framed", "dmx_inflate_batch_framed", "dmx_bgzf_bound", "dmx_deflate_bgzf",
          "dmx_inflate_bgzf"]


def test_framed_symbols_exported():
    lib = dmx.lib()
    for s in FRAMED:
        assert hasattr(lib, s), s
        assert s in dmx.EXPORTS


def test_framed_null_context_is_arg_error():
    lib = dmx.lib()
    one = (ctypes.c_void_p * 1)()
    n = (ctypes.c_size_t * 1)(0)
    res = (dmx.BatchResult * 1)()
    for count in (0, 1):
        for fmt in (dmx.DMX_FRAME_ZLIB, dmx.DMX_FRAME_GZIP, dmx.DMX_FRAME_BGZF):
            assert lib.dmx_deflate_batch_framed_device(None, one, n, count, 2, fmt, one, n, res, None) == dmx.DMX_ERR_ARG
            assert lib.dmx_inflate_batch_framed_device(None, one, n, count, fmt, one, n, res, 0, None) == dmx.DMX_ERR_ARG
            assert lib.dmx_deflate_batch_framed(None, one, n, count, 2, fmt, one, n, res) == dmx.DMX_ERR_ARG
            assert lib.dmx_inflate_batch_framed(None, one, n, count, fmt, one, n, res, 0) == dmx.DMX_ERR_ARG


def test_framed_bounds():
    lib = dmx.lib()
    for n in (0, 1, 65280, 65281, 1 << 20, (1 << 30) + 5):
        raw = dmx.deflate_bound(n)
        assert lib.dmx_batch_framed_bound(dmx.DMX_FRAME_ZLIB, n) == raw + 6
        assert lib.dmx_batch_framed_bound(dmx.DMX_FRAME_GZIP, n) == raw + 18
        assert lib.dmx_batch_framed_bound(dmx.DMX_FRAME_BGZF, n) == raw + 26
        for fmt in (0, 4, 0xFFFFFFFF):
            assert lib.dmx_batch_framed_bound(fmt, n) == 0
    # a full BGZF block always fits the 16-bit BSIZE
    assert lib.dmx_batch_framed_bound(dmx.DMX_FRAME_BGZF, 65280) == 65362 <= 65536
    assert lib.dmx_bgzf_bound(0) == 28
    assert lib.dmx_bgzf_bound(1) == 28 + dmx.deflate_bound(1) + 26
    assert lib.dmx_bgzf_bound(65280) == 28 + 65362
    assert lib.dmx_bgzf_bound(65281) == 28 + 65362 + dmx.deflate_bound(1) + 26
    assert lib.dmx_bgzf_bound(3 * 65280 + 7) == 28 + 3 * 65362 + dmx.deflate_bound(7) + 26


def test_framed_constants_match_header():
    hdr = open(os.path.join(ROOT, "include", "dmx.h")).read()
    for name, val in (("DMX_FRAME_ZLIB", 1), ("DMX_FRAME_GZIP", 2), ("DMX_FRAME_BGZF", 3), ("DMX_BATCH_VERIFY", 2),
                      ("DMX_BATCH_NO_ROUTE", 1)):
        assert re.search(r"#define %s %du\b" % (name, val), hdr), name
        assert getattr(dmx, name) == val
    assert dmx.FRAME == {"zlib": 1, "gzip": 2, "bgzf": 3}
