"""Measurement of the seek index (GPU only; fails without a device).  Writes
profiles/seek_probe.json, which DESIGN quotes.

The stream: zlib level 6 (raw, window 15) of 256 MiB of the text corpus, in device memory.

1. index cost: dmx_inflate_index_device against dmx_inflate_device on the same stream and the same
   output buffer, alternated in one run; the difference is what the index costs (the checkpoint
   selection on the host, the window gather and its host synchronisation).  At spacings of
   64 KiB, 256 KiB and 1 MiB, with the checkpoint count and the window store's size.
2. ranged read: 1 MiB from the middle of the plain bytes (dmx_inflate_range_device) against the
   full decode (dmx_inflate_device), alternated in one run, with the index of each spacing.

Timing: synchronised host wall clock around each call (every call ends in a host
synchronisation of its own), WARM warm-up rounds, then --reps measured ones; the median is
reported with the minimum beside it.

  python tools/seek_probe.py [--reps 20] [--mib 256]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
import torch  # noqa: E402

import dmx  # noqa: E402

WARM = 2
SPACINGS = (65536, 262144, 1 << 20)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(a, b, reps):
    """Run a and b alternately: WARM unmeasured rounds, then reps measured ones."""
    ta, tb = [], []
    for k in range(WARM + reps):
        x, y = timed(a), timed(b)
        if k >= WARM:
            ta.append(x)
            tb.append(y)
    return ta, tb


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seek_probe.json"))
    args = ap.parse_args()
    n_plain = args.mib << 20
    plain = dmx.corpus("text", n_plain)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = z.compress(plain) + z.flush()
    n = len(stream)
    d_in = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    d_out = torch.empty(n_plain, dtype=torch.uint8, device="cuda")
    want = torch.frombuffer(bytearray(plain), dtype=torch.uint8).cuda()
    ctx = dmx.Context()
    res = {"stream": "zlib level 6, raw", "corpus": "text", "plain_bytes": n_plain, "stream_bytes": n,
           "device": torch.cuda.get_device_name(0), "warmup": WARM, "spacings": {}}
    u0, ln = n_plain // 2 + 12345, 1 << 20
    part = torch.empty(ln, dtype=torch.uint8, device="cuda")

    def full():
        ctx.inflate_device(d_in.data_ptr(), n, d_out.data_ptr(), n_plain)

    for spacing in SPACINGS:
        box = {}

        def index():
            box["r"] = ctx.inflate_index_device(d_in.data_ptr(), n, d_out.data_ptr(), n_plain, spacing)

        t_index, t_plain = alternate(index, full, args.reps)
        out_len, entries, windows = box["r"]
        assert out_len == n_plain and torch.equal(d_out, want)
        path = ctx.stats().path
        count = entries.shape[0] - 1

        def ranged():
            ctx.inflate_range_device(d_in.data_ptr(), n, entries, windows, u0, ln, part.data_ptr())

        t_range, t_full = alternate(ranged, full, args.reps)
        assert torch.equal(part, want[u0:u0 + ln])
        first = int((entries[:count, 1] <= u0).sum()) - 1
        last = int((entries[:count + 1, 1] < u0 + ln).sum())
        rec = {"checkpoints": count, "window_bytes": int(windows.numel()),
               "window_share_of_plain": windows.numel() / n_plain,
               "inflate_index_device": summary(t_index), "inflate_device": summary(t_plain),
               "index_cost_ms": statistics.median(t_index) - statistics.median(t_plain),
               "range": {"uoffset": u0, "len": ln, "spans": last - first,
                         "inflate_range_device": summary(t_range), "inflate_device": summary(t_full)},
               "path": path}
        res["spacings"][str(spacing)] = rec
        print(json.dumps({str(spacing): rec}), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
