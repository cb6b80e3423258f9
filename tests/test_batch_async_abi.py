"""CPU: the C-ABI of the asynchronous batch calls (dmx_batch_reserve, dmx_deflate_batch_async,
dmx_inflate_batch_async): exported, listed, declared, and refusing a null context before any
device is touched.  No GPU work is launched here."""
import ctypes
import os
import re

import dmx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["dmx_batch_reserve", "dmx_deflate_batch_async", "dmx_inflate_batch_async"]


def test_symbols_exported_and_listed():
    lib = dmx.lib()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in dmx.EXPORTS, s


def test_header_declares_calls_and_deferred_status():
    hdr = open(os.path.join(ROOT, "include", "dmx.h")).read()
    assert re.search(r"^#define DMX_BATCH_DEFERRED 1\b", hdr, re.M)
    assert dmx.DMX_BATCH_DEFERRED == 1
    for s in SYMS:
        assert re.search(r"^int %s\(dmx_ctx\* ctx," % s, hdr, re.M), s


def test_null_context_is_arg_error():
    lib = dmx.lib()
    a = (ctypes.c_uint64 * 2)()  # stands for a device array: a null context is refused before any use
    p = ctypes.cast(a, ctypes.c_void_p)
    for count in (0, 1):
        assert lib.dmx_batch_reserve(None, count, 4096, 0, 0) == dmx.DMX_ERR_ARG
        assert lib.dmx_deflate_batch_async(None, p, p, count, 4096, 0, 2, None, 0, p, p, p, None) == dmx.DMX_ERR_ARG
        assert lib.dmx_inflate_batch_async(None, p, p, count, 4096, None, 0, p, p, p, 0, None) == dmx.DMX_ERR_ARG


def test_python_surface():
    for name in ("batch_reserve", "deflate_batch_async", "inflate_batch_async"):
        assert callable(getattr(dmx.Context, name)), name
    assert callable(dmx.batch_results)
