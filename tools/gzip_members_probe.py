"""Measurement of the multi-member gzip inflate (GPU only; fails without a device).  Reads only
dmx.corpus data and writes profiles/gzip_members_probe.json, which DESIGN quotes.

1. small members: 16384 members of 4 KiB of the text corpus, zlib level 6, one file in device
   memory.  dmx_inflate_gzip_members_device against dmx_inflate_batch_framed_device on the same
   members with their extents given (taken from the index the first call returns) -- what knowing
   the extents saves, and the floor the call cannot beat.  Both verify the trailers.  The phases
   (candidate scan, measuring pass, batch decode) are the library's own HIP events: with
   dmx_set_timing on, DMX_GZM_MAIN selects the phase that dmx_stats.ms_main_kernel brackets, one
   series of calls per phase.
2. long members: 256 MiB of text as four 64 MiB zlib level 6 members, against the sum of four
   dmx_inflate_device calls on the raw streams (no trailer check on either side).

Timing: HIP events around each call on the current stream (every call ends in a host
synchronisation of its own), WARM warm-up calls, then --reps measured ones; the median is reported
with the minimum beside it.

  python tools/gzip_members_probe.py [--reps 20] [--members 16384] [--mib 256]
"""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
import torch  # noqa: E402

import dmx  # noqa: E402

WARM = 5


def member(d, level=6):
    z = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = z.compress(d) + z.flush()
    return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(d), len(d) & 0xFFFFFFFF), raw


def series(fn, reps, value=None):
    """WARM unmeasured calls, then reps measured ones -> milliseconds per call (HIP events, or
    value() read after each call)."""
    out = []
    for k in range(WARM + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= WARM:
            out.append(a.elapsed_time(b) if value is None else value())
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": len(ms)}


def small_members(ctx, count, size, reps):
    plain = dmx.corpus("text", count * size)
    f = b"".join(member(plain[size * k:size * k + size])[0] for k in range(count))
    n = len(f)
    d_in = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    d_out = torch.empty(len(plain), dtype=torch.uint8, device="cuda")
    want = torch.frombuffer(bytearray(plain), dtype=torch.uint8).cuda()
    got, members, idx = ctx.inflate_gzip_members_device(d_in.data_ptr(), n, d_out.data_ptr(), len(plain), want_index=True)
    assert got == len(plain) and members == count and torch.equal(d_out, want)

    def call():
        ctx.inflate_gzip_members_device(d_in.data_ptr(), n, d_out.data_ptr(), len(plain))

    rec = {"members": count, "member_plain_bytes": size, "file_bytes": n, "plain_bytes": len(plain),
           "zlib_level": 6, "verify": True, "inflate_gzip_members_device": summary(series(call, reps))}
    ctx.set_timing(True)
    for phase in ("scan", "measure", "batch"):
        os.environ["DMX_GZM_MAIN"] = phase
        rec[phase] = summary(series(call, reps, value=lambda: ctx.stats().ms_main_kernel))
    del os.environ["DMX_GZM_MAIN"]
    ctx.set_timing(False)
    # the yardstick: the same members with their extents given
    ptrs = [d_in.data_ptr() + int(idx[k, 0]) for k in range(count)]
    sizes = [int(idx[k + 1, 0] - idx[k, 0]) for k in range(count)]
    outs = [d_out.data_ptr() + int(idx[k, 1]) for k in range(count)]
    caps = [int(idx[k + 1, 1] - idx[k, 1]) for k in range(count)]
    d_out.zero_()

    # (the argument arrays are built once: the call itself is what is timed)
    a_in, a_n = (ctypes.c_void_p * count)(*ptrs), (ctypes.c_size_t * count)(*sizes)
    a_out, a_cap = (ctypes.c_void_p * count)(*outs), (ctypes.c_size_t * count)(*caps)
    res = (dmx.BatchResult * count)()

    def framed():
        rc = dmx.lib().dmx_inflate_batch_framed_device(ctx.h, a_in, a_n, count, dmx.DMX_FRAME_GZIP, a_out, a_cap, res,
                                                       dmx.DMX_BATCH_VERIFY, None)
        assert rc == dmx.DMX_OK

    rec["inflate_batch_framed_device"] = summary(series(framed, reps))
    assert torch.equal(d_out, want) and all(r.status == dmx.DMX_OK for r in res)
    total = rec["inflate_gzip_members_device"]["median_ms"]
    rec["ratio_to_framed_batch"] = total / rec["inflate_batch_framed_device"]["median_ms"]
    rec["measure_share_of_call"] = rec["measure"]["median_ms"] / total
    rec["measure_to_batch_decode"] = rec["measure"]["median_ms"] / rec["batch"]["median_ms"]
    return rec


def long_members(ctx, mib, reps):
    part = (mib << 20) // 4
    plain = dmx.corpus("text", 4 * part)
    ms = [member(plain[part * k:part * k + part]) for k in range(4)]
    f = b"".join(m[0] for m in ms)
    n = len(f)
    d_in = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    d_out = torch.empty(len(plain), dtype=torch.uint8, device="cuda")
    want = torch.frombuffer(bytearray(plain), dtype=torch.uint8).cuda()
    got, members = ctx.inflate_gzip_members_device(d_in.data_ptr(), n, d_out.data_ptr(), len(plain))
    assert got == len(plain) and members == 4 and torch.equal(d_out, want)

    def call(verify=False):
        ctx.inflate_gzip_members_device(d_in.data_ptr(), n, d_out.data_ptr(), len(plain), verify=verify)

    starts, o = [], 0
    for m, raw in ms:
        starts.append((o + 10, len(raw)))
        o += len(m)
    d_out.zero_()

    def four():
        for k, (at, ln) in enumerate(starts):
            ctx.inflate_device(d_in.data_ptr() + at, ln, d_out.data_ptr() + part * k, part)

    rec = {"members": 4, "member_plain_bytes": part, "file_bytes": n, "plain_bytes": len(plain), "zlib_level": 6,
           "four_inflate_device_calls": summary(series(four, reps))}
    assert torch.equal(d_out, want)
    rec["inflate_gzip_members_device"] = summary(series(call, reps))
    rec["inflate_gzip_members_device_verify"] = summary(series(lambda: call(True), reps))
    ctx.set_timing(True)  # the measuring pass alone: every member's window runs to the limit
    os.environ["DMX_GZM_MAIN"] = "measure"
    rec["measure"] = summary(series(call, reps, value=lambda: ctx.stats().ms_main_kernel))
    del os.environ["DMX_GZM_MAIN"]
    ctx.set_timing(False)
    rec["measure_share_of_call"] = rec["measure"]["median_ms"] / rec["inflate_gzip_members_device"]["median_ms"]
    rec["ratio_to_four_calls"] = (rec["inflate_gzip_members_device"]["median_ms"] /
                                  rec["four_inflate_device_calls"]["median_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--members", type=int, default=16384)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gzip_members_probe.json"))
    args = ap.parse_args()
    ctx = dmx.Context()
    res = {"corpus": "text", "device": torch.cuda.get_device_name(0), "warmup": WARM}
    res["small_members"] = small_members(ctx, args.members, 4096, args.reps)
    print(json.dumps({"small_members": res["small_members"]}), flush=True)
    res["long_members"] = long_members(ctx, args.mib, args.reps)
    print(json.dumps({"long_members": res["long_members"]}), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
