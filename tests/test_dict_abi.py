"""CPU: the preset-dictionary entry points of include/dmx.h exist and reject a null context and
a null dictionary of non-zero length.  No GPU work is launched here."""
import ctypes

import dmx

DICT = ["dmx_deflate_batch_dict_device", "dmx_inflate_batch_dict_device", "dmx_deflate_batch_dict",
        "dmx_inflate_batch_dict"]


def test_dict_symbols_exported():
    lib = dmx.lib()
    for s in DICT:
        assert hasattr(lib, s), s
        assert s in dmx.EXPORTS


def calls(lib, ctx, count, d, dlen):
    one = (ctypes.c_void_p * 1)()
    n = (ctypes.c_size_t * 1)(0)
    res = (dmx.BatchResult * 1)()
    return [lib.dmx_deflate_batch_dict_device(ctx, one, n, count, 2, d, dlen, one, n, res, None),
            lib.dmx_inflate_batch_dict_device(ctx, one, n, count, d, dlen, one, n, res, 0, None),
            lib.dmx_deflate_batch_dict(ctx, one, n, count, 2, d, dlen, one, n, res),
            lib.dmx_inflate_batch_dict(ctx, one, n, count, d, dlen, one, n, res, 0)]


def test_dict_null_context_is_arg_error():
    lib = dmx.lib()
    d = ctypes.create_string_buffer(b"0123456789abcdef")
    for count in (0, 1):
        assert calls(lib, None, count, None, 0) == [dmx.DMX_ERR_ARG] * 4
        assert calls(lib, None, count, d, 16) == [dmx.DMX_ERR_ARG] * 4


def test_dict_null_dictionary_with_length_is_arg_error():
    lib = dmx.lib()
    for count in (0, 1):
        assert calls(lib, None, count, None, 1) == [dmx.DMX_ERR_ARG] * 4
