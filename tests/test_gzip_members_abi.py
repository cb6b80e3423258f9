"""CPU: the C-ABI of the multi-member gzip calls (dmx_inflate_gzip_members_device,
dmx_inflate_gzip_members).  No GPU work is launched: the argument check comes before anything of
the context is looked at, so the context here is a block of zeros that a correct check never reads."""
import ctypes

import dmx

NAMES = ["dmx_inflate_gzip_members_device", "dmx_inflate_gzip_members"]


def test_symbols_exported():
    lib = dmx.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in dmx.EXPORTS


def _calls(ctx, flags, out_len, data=b"\x1f\x8b"):
    lib = dmx.lib()
    m = ctypes.c_size_t(7)
    buf = ctypes.create_string_buffer(64)
    return (lib.dmx_inflate_gzip_members_device(ctx, None, 0, flags, None, 0, None, 0, ctypes.byref(m), out_len, None),
            lib.dmx_inflate_gzip_members(ctx, data, len(data), flags, buf, 64, ctypes.byref(m), out_len))


def test_argument_errors_need_no_gpu():
    n = ctypes.c_size_t(123)
    fake = ctypes.create_string_buffer(1 << 16)  # never read: every call below fails its argument check
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    assert _calls(None, 0, ctypes.byref(n)) == (dmx.DMX_ERR_ARG, dmx.DMX_ERR_ARG)      # a null context
    assert _calls(None, dmx.DMX_VERIFY, ctypes.byref(n)) == (dmx.DMX_ERR_ARG, dmx.DMX_ERR_ARG)
    assert _calls(ctx, 0, None) == (dmx.DMX_ERR_ARG, dmx.DMX_ERR_ARG)                  # a null out_len
    for flags in (2, 4, 0x80000000, dmx.DMX_VERIFY | 2):                                # an unknown flag
        assert _calls(ctx, flags, ctypes.byref(n)) == (dmx.DMX_ERR_ARG, dmx.DMX_ERR_ARG), flags
    assert n.value == 123  # nothing was written
    lib = dmx.lib()
    buf = ctypes.create_string_buffer(8)
    # a null input with n > 0, a null output with cap > 0
    assert lib.dmx_inflate_gzip_members_device(ctx, None, 5, 0, buf, 8, None, 0, None, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_gzip_members_device(ctx, buf, 5, 0, None, 8, None, 0, None, ctypes.byref(n), None) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_gzip_members(ctx, None, 5, 0, buf, 8, None, ctypes.byref(n)) == dmx.DMX_ERR_ARG
    assert lib.dmx_inflate_gzip_members(ctx, buf, 5, 0, None, 8, None, ctypes.byref(n)) == dmx.DMX_ERR_ARG


def test_the_empty_file_needs_no_gpu():
    """n == 0 is DMX_OK with no member and no byte, before any device work."""
    fake = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    lib = dmx.lib()
    n, m = ctypes.c_size_t(9), ctypes.c_size_t(9)
    ent = (dmx.BgzfEntry * 1)()
    ent[0].coffset = ent[0].uoffset = 5
    assert lib.dmx_inflate_gzip_members_device(ctx, None, 0, dmx.DMX_VERIFY, None, 0, ent, 1, ctypes.byref(m),
                                               ctypes.byref(n), None) == dmx.DMX_OK
    assert (n.value, m.value, ent[0].coffset, ent[0].uoffset) == (0, 0, 0, 0)
    assert lib.dmx_inflate_gzip_members_device(ctx, None, 0, 0, None, 0, ent, 0, ctypes.byref(m), ctypes.byref(n),
                                               None) == dmx.DMX_ERR_CAPACITY
    assert lib.dmx_inflate_gzip_members(ctx, None, 0, 0, None, 0, ctypes.byref(m), ctypes.byref(n)) == dmx.DMX_OK
    assert (n.value, m.value) == (0, 0)
