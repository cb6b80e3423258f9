"""Measurement of the batched API (GPU only; fails without a device).  Writes
profiles/batch_probe.json, which DESIGN quotes.

1. batch against loop: 16384 x 4 KiB and 4096 x 64 KiB buffers of text and of mixed data,
   level 2, deflate and inflate; one batch call against a loop of deflate_device /
   inflate_device over the same device buffers, the two alternated within the run.
2. routing crossover: single libdmx level-2 text streams of 64 KiB .. 16 MiB,
   inflate_batch_device(no_route=True) against inflate_device.

3. preset dictionary (--dict, writes profiles/batch_probe_dict.json): 16384 x 1 KiB and
   16384 x 4 KiB pages of synthetic JSON log records, level 2, an 8 KiB dictionary of other
   records of the same generator; the batch calls with the dictionary against the same calls
   without it, alternated; ms per call and total compressed bytes of both.

4. framed batch (--framed, writes profiles/batch_probe_framed.json): the shapes of part 1, level
   2; the gzip-framed batch deflate against the plain batch deflate on the same buffers (the
   difference is what checksums and framing cost), the framed batch inflate with and without
   DMX_BATCH_VERIFY against the plain batch inflate, the loop over dmx_deflate_gzip /
   dmx_inflate_gzip (host buffers, --loop-reps repetitions), and dmx_deflate_bgzf /
   dmx_inflate_bgzf of 256 MiB of text with their GB/s.

5. BGZF in device memory (--bgzf-device, writes profiles/batch_probe_bgzf.json): 256 MiB of text,
   level 2; dmx_deflate_bgzf / dmx_inflate_bgzf (host buffers) against dmx_deflate_bgzf_device /
   dmx_inflate_bgzf_device (device buffers), alternated in one run, with the chain walk alone
   (dmx_bgzf_index_device) and a 1 MiB ranged read beside them.

6. asynchronous batch calls (--async, writes profiles/batch_probe_async.json): 16384 x 4 KiB and
   4096 x 64 KiB of text, level 2; dmx_deflate_batch_device / dmx_inflate_batch_device (host
   descriptor arrays, prebuilt; the call synchronises) against dmx_deflate_batch_async /
   dmx_inflate_batch_async (device descriptor arrays) plus one torch.cuda.synchronize(),
   alternated in one run; the async call's host time until it returns; and a deflate -> inflate
   chain: two synchronous calls with a host read of the sizes between them against two
   asynchronous calls, one torch op on the stream that takes the sizes, and one synchronise.

Timing: synchronised host wall clock around each call (every call ends in a host
synchronisation of its own), WARM warm-up repetitions, then REPS measured ones; the median is
reported with the minimum beside it.

  python tools/batch_probe.py [--reps 20] [--quick] [--dict | --framed [--loop-reps 20] | --bgzf-device | --async]
"""
import argparse
import ctypes
import gc
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
import torch  # noqa: E402

import dmx  # noqa: E402

WARM = 2


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


def batch_vs_loop(ctx, kind, count, size, reps):
    data = dmx.corpus(kind, count * size, offset=1 << 20)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bound = (dmx.deflate_bound(size) + 15) & ~15
    d_c = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(count * size, dtype=torch.uint8, device="cuda")
    ins = [d_in.data_ptr() + i * size for i in range(count)]
    comps = [d_c.data_ptr() + i * bound for i in range(count)]
    outs = [d_o.data_ptr() + i * size for i in range(count)]
    sizes, bounds = [size] * count, [bound] * count
    clen = []

    def df_batch():
        clen[:] = [r[0] for r in ctx.deflate_batch_device(ins, sizes, 2, comps, bounds)]

    def df_loop():
        for i in range(count):
            ctx.deflate_device(ins[i], size, 2, comps[i], bound)

    def if_batch():
        res = ctx.inflate_batch_device(comps, clen, outs, sizes)
        assert all(r[1] == dmx.DMX_OK for r in res)

    def if_loop():
        for i in range(count):
            ctx.inflate_device(comps[i], clen[i], outs[i], size)

    db, dl = alternate(df_batch, df_loop, reps)
    ib, il = alternate(if_batch, if_loop, reps)
    assert d_o.cpu().numpy().tobytes() == data, "round trip mismatch"
    row = {"kind": kind, "count": count, "size": size, "compressed_bytes": sum(clen),
           "deflate_batch": summary(db), "deflate_loop": summary(dl),
           "inflate_batch": summary(ib), "inflate_loop": summary(il)}
    row["deflate_loop_over_batch"] = row["deflate_loop"]["median_ms"] / row["deflate_batch"]["median_ms"]
    row["inflate_loop_over_batch"] = row["inflate_loop"]["median_ms"] / row["inflate_batch"]["median_ms"]
    return row


def crossover(ctx, size, reps):
    data = dmx.corpus("text", size, offset=7 << 20)
    s = ctx.compress(data, 2)
    d_s = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    d_o = torch.empty(size, dtype=torch.uint8, device="cuda")

    def one_wave():
        res = ctx.inflate_batch_device([d_s.data_ptr()], [len(s)], [d_o.data_ptr()], [size], no_route=True)
        assert res[0] == (size, dmx.DMX_OK, dmx.BATCH_PATH), res

    def single():
        assert ctx.inflate_device(d_s.data_ptr(), len(s), d_o.data_ptr(), size) == size

    tb, ts = alternate(one_wave, single, reps)
    assert d_o.cpu().numpy().tobytes() == data
    return {"plain_bytes": size, "stream_bytes": len(s), "batch_kernel": summary(tb), "inflate_device": summary(ts),
            "batch_kernel_wins": statistics.median(tb) < statistics.median(ts)}


HOSTS = ["gpu-node-%02d.cluster.example" % i for i in range(12)]
LEVELS = ["INFO", "WARN", "ERROR", "DEBUG"]
MSGS = ["kernel launch completed", "allocation of device buffer failed", "segment table uploaded",
        "stream synchronised", "checksum verified", "window hand-off finished"]


def records(seed, nbytes):
    """Deterministic JSON-ish log lines (the generator of tests/test_gpu_dict.py)."""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < nbytes:
        out += ('{"timestamp":"2026-10-%02dT%02d:%02d:%02dZ","host":"%s","level":"%s","message":"%s",'
                '"bytes":%d,"latency_us":%d}\n' % (
                    r.randrange(1, 29), r.randrange(24), r.randrange(60), r.randrange(60), r.choice(HOSTS),
                    r.choice(LEVELS), r.choice(MSGS), r.randrange(1 << 20), r.randrange(100000))).encode()
    return bytes(out[:nbytes])


def dict_vs_plain(ctx, count, size, reps, dict_bytes=8192):
    d = records(1, dict_bytes)
    data = records(100, count * size)
    d_d = torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda()
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bound = (dmx.deflate_bound(size) + 15) & ~15
    d_c = [torch.empty(count * bound, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_o = torch.empty(count * size, dtype=torch.uint8, device="cuda")
    ins = [d_in.data_ptr() + i * size for i in range(count)]
    comps = [[t.data_ptr() + i * bound for i in range(count)] for t in d_c]
    outs = [d_o.data_ptr() + i * size for i in range(count)]
    sizes, bounds = [size] * count, [bound] * count
    clen = [[], []]
    kw = [{}, {"dict_ptr": d_d.data_ptr(), "dict_len": len(d)}]

    def deflate(k):
        def run():
            res = ctx.deflate_batch_device(ins, sizes, 2, comps[k], bounds, **kw[k])
            assert all(r[1] == dmx.DMX_OK for r in res)
            clen[k][:] = [r[0] for r in res]
        return run

    def inflate(k):
        def run():
            d_o.zero_()
            res = ctx.inflate_batch_device(comps[k], clen[k], outs, sizes, **kw[k])
            assert all(r[1:] == (dmx.DMX_OK, dmx.BATCH_PATH) for r in res)
        return run

    dp, dd = alternate(deflate(0), deflate(1), reps)
    ip, id_ = alternate(inflate(0), inflate(1), reps)
    assert d_o.cpu().numpy().tobytes() == data, "round trip mismatch (with dictionary)"
    inflate(0)()
    assert d_o.cpu().numpy().tobytes() == data, "round trip mismatch (without)"
    return {"kind": "records", "count": count, "size": size, "dict_bytes": len(d), "level": 2,
            "compressed_bytes_plain": sum(clen[0]), "compressed_bytes_dict": sum(clen[1]),
            "bytes_dict_over_plain": sum(clen[1]) / sum(clen[0]),
            "deflate_plain": summary(dp), "deflate_dict": summary(dd),
            "inflate_plain": summary(ip), "inflate_dict": summary(id_)}


def alternate_all(fns, reps):
    """Run the variants in turn, round after round: WARM unmeasured rounds, then reps measured."""
    ts = [[] for _ in fns]
    gc.collect()
    gc.disable()  # the calls build lists of thousands of tuples; a collection inside a timed call
    try:          # costs tens of ms and recurs with a period that can lock onto one variant
        for k in range(WARM + reps):
            for t, f in zip(ts, fns):
                x = timed(f)
                if k >= WARM:
                    t.append(x)
            gc.collect()
    finally:
        gc.enable()
    return ts


def framed_vs_plain(ctx, kind, count, size, reps, loop_reps):
    data = dmx.corpus(kind, count * size, offset=1 << 20)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bound = (dmx.lib().dmx_batch_framed_bound(dmx.DMX_FRAME_GZIP, size) + 15) & ~15
    d_c = [torch.empty(count * bound, dtype=torch.uint8, device="cuda") for _ in range(2)]  # plain, framed
    d_o = torch.empty(count * size, dtype=torch.uint8, device="cuda")
    ins = [d_in.data_ptr() + i * size for i in range(count)]
    comps = [[t.data_ptr() + i * bound for i in range(count)] for t in d_c]
    outs = [d_o.data_ptr() + i * size for i in range(count)]
    sizes, bounds = [size] * count, [bound] * count
    clen = [[], []]

    def df_plain():
        clen[0][:] = [r[0] for r in ctx.deflate_batch_device(ins, sizes, 2, comps[0], bounds)]

    def df_framed():
        res = ctx.deflate_batch_framed_device(ins, sizes, 2, comps[1], bounds, format="gzip")
        assert all(r[1] == dmx.DMX_OK for r in res)
        clen[1][:] = [r[0] for r in res]

    def if_plain():
        assert all(r[1] == dmx.DMX_OK for r in ctx.inflate_batch_device(comps[0], clen[0], outs, sizes))

    def if_framed(verify):
        def run():
            res = ctx.inflate_batch_framed_device(comps[1], clen[1], outs, sizes, format="gzip", verify=verify)
            assert all(r[:2] == (size, dmx.DMX_OK) for r in res)
        return run

    dp, dfr = alternate_all([df_plain, df_framed], reps)
    assert [c + 18 for c in clen[0]] == clen[1]
    ip, iv, inv = alternate_all([if_plain, if_framed(True), if_framed(False)], reps)
    assert d_o.cpu().numpy().tobytes() == data, "round trip mismatch"

    # the loop over the single-buffer container calls (host buffers, as their callers hold them)
    lib, h = dmx.lib(), ctx.h
    hin = ctypes.create_string_buffer(data, len(data))
    hout = ctypes.create_string_buffer(count * bound)
    base_in, base_out = ctypes.addressof(hin), ctypes.addressof(hout)
    glen = [0] * count
    n = ctypes.c_size_t()
    p = ctypes.POINTER(ctypes.c_uint8)()

    def df_loop():
        for i in range(count):
            rc = lib.dmx_deflate_gzip(h, base_in + i * size, size, 2, base_out + i * bound, bound, ctypes.byref(n))
            assert rc == dmx.DMX_OK
            glen[i] = n.value

    def if_loop():
        for i in range(count):
            rc = lib.dmx_inflate_gzip(h, base_out + i * bound, glen[i], dmx.DMX_VERIFY, ctypes.byref(p), ctypes.byref(n))
            assert rc == dmx.DMX_OK and n.value == size
            lib.dmx_free(p)

    dl, il = alternate_all([df_loop, if_loop], loop_reps)
    assert glen == clen[1]
    row = {"kind": kind, "count": count, "size": size, "level": 2, "format": "gzip", "compressed_bytes": sum(clen[1]),
           "deflate_batch_plain": summary(dp), "deflate_batch_framed": summary(dfr),
           "inflate_batch_plain": summary(ip), "inflate_batch_framed_verify": summary(iv),
           "inflate_batch_framed_noverify": summary(inv),
           "deflate_gzip_loop": summary(dl), "inflate_gzip_loop": summary(il)}
    m = lambda k: row[k]["median_ms"]  # noqa: E731
    row["deflate_framing_cost_ms"] = m("deflate_batch_framed") - m("deflate_batch_plain")
    row["inflate_verify_cost_ms"] = m("inflate_batch_framed_verify") - m("inflate_batch_plain")
    row["deflate_loop_over_framed_batch"] = m("deflate_gzip_loop") / m("deflate_batch_framed")
    row["inflate_loop_over_framed_batch"] = m("inflate_gzip_loop") / m("inflate_batch_framed_verify")
    return row


def bgzf_file(ctx, nbytes, reps):
    data = dmx.corpus("text", nbytes, offset=3 << 20)
    f = []

    def deflate():
        f[:] = [ctx.compress_bgzf(data, 2)]

    def inflate():
        assert len(ctx.decompress_bgzf(f[0], verify=True)) == nbytes

    td, ti = alternate_all([deflate, inflate], reps)
    assert ctx.decompress_bgzf(f[0]) == data
    row = {"kind": "text", "plain_bytes": nbytes, "file_bytes": len(f[0]), "level": 2,
           "deflate_bgzf": summary(td), "inflate_bgzf": summary(ti)}
    row["deflate_gb_per_s"] = nbytes / (row["deflate_bgzf"]["median_ms"] * 1e6)
    row["inflate_gb_per_s"] = nbytes / (row["inflate_bgzf"]["median_ms"] * 1e6)
    return row


def bgzf_device_file(ctx, nbytes, reps):
    """The host forms dmx_deflate_bgzf / dmx_inflate_bgzf against the device forms on the same
    bytes, alternated in one run; the chain walk alone (dmx_bgzf_index_device) beside them."""
    data = dmx.corpus("text", nbytes, offset=3 << 20)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bound = dmx.bgzf_bound(nbytes)
    d_file = torch.empty(bound, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d_part = torch.empty(min(1 << 20, nbytes // 4), dtype=torch.uint8, device="cuda")
    f, flen, idx = [], [0], []

    def deflate_host():
        f[:] = [ctx.compress_bgzf(data, 2)]

    def deflate_dev():
        flen[0] = ctx.deflate_bgzf_device(d_in.data_ptr(), nbytes, 2, d_file.data_ptr(), bound)

    def inflate_host():
        assert len(ctx.decompress_bgzf(f[0], verify=True)) == nbytes

    def inflate_dev():
        assert ctx.inflate_bgzf_device(d_file.data_ptr(), flen[0], d_out.data_ptr(), nbytes, verify=True) == nbytes

    def index_dev():
        idx[:] = [ctx.bgzf_index_device(d_file.data_ptr(), flen[0])]

    def range_dev():  # 1 MiB from the middle of the file
        ctx.inflate_bgzf_range_device(d_file.data_ptr(), flen[0], idx[0], nbytes // 2 + 12345, d_part.numel(),
                                      d_part.data_ptr())

    dh, dd, ih, idv, ix, rg = alternate_all([deflate_host, deflate_dev, inflate_host, inflate_dev, index_dev, range_dev],
                                            reps)
    assert d_file[:flen[0]].cpu().numpy().tobytes() == f[0]
    assert torch.equal(d_out, d_in)
    assert torch.equal(d_part, d_in[nbytes // 2 + 12345:nbytes // 2 + 12345 + d_part.numel()])
    # the chain kernels alone, by HIP events (the two read-backs between them included)
    ctx.set_timing(True)
    chain = []
    for _ in range(WARM + reps):
        index_dev()
        chain.append(ctx.stats().ms_device_total)
    ctx.set_timing(False)
    row = {"kind": "text", "plain_bytes": nbytes, "file_bytes": flen[0], "members": int(idx[0].shape[0] - 1), "level": 2,
           "deflate_bgzf_host": summary(dh), "deflate_bgzf_device": summary(dd),
           "inflate_bgzf_host": summary(ih), "inflate_bgzf_device": summary(idv),
           "bgzf_index_device": summary(ix), "bgzf_range_1MiB_device": summary(rg),
           "chain_device_ms": summary(chain[WARM:]),
           "device_beats_host_every_pass": {"deflate": all(d < h for d, h in zip(dd, dh)),
                                            "inflate": all(d < h for d, h in zip(idv, ih))}}
    for k in ("deflate_bgzf_host", "deflate_bgzf_device", "inflate_bgzf_host", "inflate_bgzf_device"):
        row[k + "_gb_per_s"] = nbytes / (row[k]["median_ms"] * 1e6)
    return row


def async_vs_sync(ctx, count, size, reps):
    import numpy as np
    data = dmx.corpus("text", count * size, offset=1 << 20)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    bound = (dmx.deflate_bound(size) + 15) & ~15
    d_c = torch.empty(count * bound, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(count * size, dtype=torch.uint8, device="cuda")
    ins = [d_in.data_ptr() + i * size for i in range(count)]
    comps = [d_c.data_ptr() + i * bound for i in range(count)]
    outs = [d_o.data_ptr() + i * size for i in range(count)]
    # synchronous side: the host arrays, built once (the calls themselves are what is timed)
    vp, sz = ctypes.c_void_p * count, ctypes.c_size_t * count
    h_in, h_comp, h_out = vp(*ins), vp(*comps), vp(*outs)
    h_size, h_bound, h_clen = sz(*[size] * count), sz(*[bound] * count), sz()
    h_res = (dmx.BatchResult * count)()
    res_np = np.frombuffer(h_res, dtype=np.dtype([("bytes", "<u8"), ("status", "<i4"), ("path", "<u4")]))
    clen_np = np.frombuffer(h_clen, dtype=np.uint64)
    lib, h = dmx.lib(), ctx.h
    # asynchronous side: the same arrays as device tensors, the results on the device
    i64 = lambda v: torch.tensor(v, dtype=torch.int64).cuda()  # noqa: E731
    t_in, t_comp, t_out = i64(ins), i64(comps), i64(outs)
    t_size, t_bound = i64([size] * count), i64([bound] * count)
    t_res = [torch.zeros(count * 16, dtype=torch.uint8, device="cuda") for _ in range(2)]  # deflate, inflate
    t_clen = torch.zeros(count, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    ctx.batch_reserve(count, bound, count * size)
    host_ms = {"deflate": [], "inflate": []}

    def sizes_to_host():  # the host read of the sizes (the synchronous call has them in h_res)
        assert (res_np["status"] == dmx.DMX_OK).all()
        clen_np[:] = res_np["bytes"]

    def df_sync():
        assert lib.dmx_deflate_batch_device(h, h_in, h_size, count, 2, h_comp, h_bound, h_res, None) == dmx.DMX_OK

    def if_sync():
        assert lib.dmx_inflate_batch_device(h, h_comp, h_clen, count, h_out, h_size, h_res, 0, None) == dmx.DMX_OK

    def df_async(record=True):
        t = time.perf_counter()
        ctx.deflate_batch_async(t_in.data_ptr(), t_size.data_ptr(), count, size, 2, t_comp.data_ptr(),
                                t_bound.data_ptr(), t_res[0].data_ptr(), max_total=count * size, stream=sp)
        if record:
            host_ms["deflate"].append((time.perf_counter() - t) * 1e3)

    def if_async(record=True):
        t = time.perf_counter()
        ctx.inflate_batch_async(t_comp.data_ptr(), t_clen.data_ptr(), count, bound, t_out.data_ptr(),
                                t_size.data_ptr(), t_res[1].data_ptr(), stream=sp)
        if record:
            host_ms["inflate"].append((time.perf_counter() - t) * 1e3)

    def take_sizes():
        with torch.cuda.stream(st):
            t_clen.copy_(t_res[0].view(torch.int64).view(-1, 2)[:, 0])

    def chain_sync():
        df_sync()
        sizes_to_host()
        if_sync()

    def chain_async():
        df_async(False)
        take_sizes()
        if_async(False)

    ds, da = alternate_all([df_sync, df_async], reps)
    sizes_to_host()
    take_sizes()
    torch.cuda.synchronize()
    assert (t_clen.cpu().numpy().astype(np.uint64) == clen_np).all(), "async deflate sizes differ"
    is_, ia = alternate_all([if_sync, if_async], reps)
    assert d_o.cpu().numpy().tobytes() == data, "round trip mismatch"
    assert all(r[:2] == (size, dmx.DMX_OK) for r in dmx.batch_results(t_res[1]))
    d_o.zero_()
    cs, ca = alternate_all([chain_sync, chain_async], reps)
    assert d_o.cpu().numpy().tobytes() == data, "chain round trip mismatch"
    row = {"kind": "text", "count": count, "size": size, "level": 2, "compressed_bytes": int(clen_np.sum()),
           "deflate_sync": summary(ds), "deflate_async_plus_sync": summary(da),
           "deflate_async_host_return": summary(host_ms["deflate"][WARM:]),
           "inflate_sync": summary(is_), "inflate_async_plus_sync": summary(ia),
           "inflate_async_host_return": summary(host_ms["inflate"][WARM:]),
           "chain_sync": summary(cs), "chain_async": summary(ca)}
    m = lambda k: row[k]["median_ms"]  # noqa: E731
    row["deflate_async_over_sync"] = m("deflate_async_plus_sync") / m("deflate_sync")
    row["inflate_async_over_sync"] = m("inflate_async_plus_sync") / m("inflate_sync")
    row["chain_async_over_sync"] = m("chain_async") / m("chain_sync")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="an eighth of the buffer counts (a check of the tool)")
    ap.add_argument("--dict", action="store_true", help="only the preset-dictionary shapes (part 3)")
    ap.add_argument("--framed", action="store_true", help="only the framed batch and BGZF shapes (part 4)")
    ap.add_argument("--loop-reps", type=int, default=20, help="--framed: repetitions of the single-buffer loops")
    ap.add_argument("--bgzf-device", action="store_true", help="only BGZF in device memory against the host forms (part 5)")
    ap.add_argument("--async", dest="async_", action="store_true",
                    help="only the asynchronous batch calls against the synchronous ones (part 6)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    name = ("batch_probe_dict.json" if a.dict else "batch_probe_framed.json" if a.framed else
            "batch_probe_bgzf.json" if a.bgzf_device else "batch_probe_async.json" if a.async_ else
            "batch_probe.json")
    a.out = a.out or os.path.join(ROOT, "profiles", name)
    if not torch.cuda.is_available():
        sys.exit("batch_probe: no GPU")
    ctx = dmx.Context()
    q = 8 if a.quick else 1
    if a.async_:
        result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARM, "quick": a.quick,
                  "timing": "host wall clock from before the call to after torch.cuda.synchronize(); synchronous "
                            "and asynchronous forms alternated in one run, Python's garbage collector run between "
                            "rounds; the synchronous calls go straight to the C ABI with host arrays built once; "
                            "*_host_return: wall clock of the asynchronous call alone, until it returns",
                  "async_vs_sync": []}
        for count, size in ((16384 // q, 4096), (4096 // q, 65536)):
            row = async_vs_sync(ctx, count, size, a.reps)
            result["async_vs_sync"].append(row)
            print(json.dumps(row), flush=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        ctx.close()
        return
    if a.bgzf_device:
        result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARM, "quick": a.quick,
                  "timing": "synchronised host wall clock per call, host and device forms alternated in one run, "
                            "Python's garbage collector run between rounds; chain_device_ms: HIP events around "
                            "dmx_bgzf_index_device's device work",
                  "bgzf_device": [bgzf_device_file(ctx, (256 << 20) // q, a.reps)]}
        print(json.dumps(result["bgzf_device"][0]), flush=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        ctx.close()
        return
    if a.dict:
        result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARM, "quick": a.quick,
                  "timing": "synchronised host wall clock per call, with and without dictionary alternated",
                  "dict_vs_plain": []}
        for size in (1024, 4096):
            row = dict_vs_plain(ctx, 16384 // q, size, a.reps)
            result["dict_vs_plain"].append(row)
            print(json.dumps(row), flush=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        ctx.close()
        return
    if a.framed:
        result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "loop_reps": a.loop_reps, "warmup": WARM,
                  "quick": a.quick,
                  "timing": "synchronised host wall clock per call, the variants alternated, Python's garbage "
                            "collector run between rounds and not inside a timed call",
                  "framed_vs_plain": [], "bgzf": []}

        def save_framed():
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")

        row = bgzf_file(ctx, (256 << 20) // q, min(a.reps, 5))
        result["bgzf"].append(row)
        print(json.dumps(row), flush=True)
        save_framed()
        for count, size in ((4096 // q, 65536), (16384 // q, 4096)):
            for kind in ("text", "mixed"):
                row = framed_vs_plain(ctx, kind, count, size, a.reps, a.loop_reps)
                result["framed_vs_plain"].append(row)
                print(json.dumps(row), flush=True)
                save_framed()
        ctx.close()
        return
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": WARM, "quick": a.quick,
              "timing": "synchronised host wall clock per call, batch and loop alternated",
              "batch_vs_loop": [], "routing_crossover": []}
    def save():  # after every row: a run cut short still leaves what it measured
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    # the cheap parts first: the 4 KiB loops take minutes (16384 single calls per repetition)
    for size in (64 << 10, 256 << 10, 1 << 20, 4 << 20, 16 << 20):
        row = crossover(ctx, size, a.reps)
        result["routing_crossover"].append(row)
        print(json.dumps(row), flush=True)
        save()
    for count, size in ((4096 // q, 65536), (16384 // q, 4096)):
        for kind in ("text", "mixed"):
            row = batch_vs_loop(ctx, kind, count, size, a.reps)
            result["batch_vs_loop"].append(row)
            print(json.dumps(row), flush=True)
            save()
    ctx.close()


if __name__ == "__main__":
    main()
