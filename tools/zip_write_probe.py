"""Measurement of the ZIP writer (GPU only; fails without a device).  Writes
profiles/zip_write_probe.json, which DESIGN quotes.

Archives, the plain bytes already in device memory:
  a. the 65536 tiny entries of tests/zip_write_cases.tiny (every third deflated, the others stored)
  b. 64 entries of 16 MiB of the mixed corpus, deflated at level 2

Per archive, WARM warm-up calls and --reps timed ones, the median (the minimum beside it):
  zip_write_device        the whole call, HIP events around it (it ends in a host synchronisation)
  deflate_batch_device    dmx_deflate_batch_device on the same method 8 buffers alone
  remainder               the difference: CRC-32, layout, pack
  pack                    the pack launch alone, the library's own events (dmx_set_timing:
                          dmx_stats.ms_main_kernel), and its rate 2 x payload bytes / time, counted
                          like bench.py's d2d_copy_GBps, beside a device-to-device copy of as many
                          bytes measured here
  host alternative        the payloads device-to-host (pageable), the archive assembled serially
                          on the host from them (struct.pack and one join in Python, zlib.crc32 of
                          the plain bytes not counted), the archive host-to-device

  python tools/zip_write_probe.py [--reps 15] [--entries 64] [--mib 16]
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import struct
import sys
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import dmx  # noqa: E402
import zip_write_cases as zw  # noqa: E402

WARM = 3
CHUNK = 65536  # zip_write.h: kZipwChunk


def series(fn, reps, value=None):
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


def wall(fn, reps):
    out = []
    for k in range(WARM + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= WARM:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "reps": len(ms)}


def host_assemble(names, methods, plain_sizes, crcs, payloads):
    """the archive from payloads that sit on the host: classic records (no entry here needs ZIP64
    but the end record of 65535 entries or more)"""
    parts, central, off = [], [], 0
    for name, method, usize, crc, p in zip(names, methods, plain_sizes, crcs, payloads):
        parts.append(struct.pack("<IHHHIIIIHH", 0x04034B50, 20, 0, method, 0x00210000, crc, len(p), usize, len(name), 0))
        parts.append(name)
        parts.append(p)
        central.append(struct.pack("<IHHHHIIIIHHHHHII", 0x02014B50, 20, 20, 0, method, 0x00210000, crc, len(p), usize,
                                   len(name), 0, 0, 0, 0, 0, off) + name)
        off += 30 + len(name) + len(p)
    cd = b"".join(central)
    count = len(names)
    end = b""
    if count >= 0xFFFF:
        end = struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, count, count, len(cd), off)
        end += struct.pack("<IIQI", 0x07064B50, 0, off + len(cd), 1)
        end += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
    else:
        end = struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, count, count, len(cd), off, 0)
    return b"".join(parts) + cd + end


def probe(ctx, label, datas, names, methods, reps, level=2):
    count = len(datas)
    sizes = [len(d) for d in datas]
    # the plain inputs back to back, 16-byte aligned each
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + 15) & ~15
    host = bytearray(max(at, 16))
    for o, d in zip(offs, datas):
        host[o:o + len(d)] = d
    d_in = torch.frombuffer(host, dtype=torch.uint8).cuda()
    ptrs = [d_in.data_ptr() + o for o in offs]
    cap = dmx.zip_bound(sizes, names, methods)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n_arc, entries = ctx.zip_write_device(ptrs, sizes, names, d_out.data_ptr(), cap, level=level, methods=methods)
    torch.cuda.synchronize()
    archive = d_out[:n_arc].cpu().numpy().tobytes()
    with zipfile.ZipFile(io.BytesIO(archive)) as z:  # the archive that is timed is a good one
        infos = z.infolist()
        assert len(infos) == count
        for k in sorted({0, count // 2, count - 1}):
            assert z.read(infos[k]) == datas[k]
    payload = sum(e.csize for e in entries)
    rec = {"entries": count, "plain_bytes": sum(sizes), "archive_bytes": n_arc, "payload_bytes": payload, "level": level,
           "chunk_bytes": CHUNK}

    # (the argument array is built once: the call itself is what is timed)
    src = dmx.zip_sources(ptrs, sizes, names, methods)
    ent = (dmx.ZipEntry * count)()
    out_len = ctypes.c_size_t()

    def call():
        rc = dmx.lib().dmx_zip_write_device(ctx.h, src, count, level, 0, None, 0, ctypes.c_void_p(d_out.data_ptr()), cap,
                                            ent, ctypes.byref(out_len), None)
        assert rc == dmx.DMX_OK and out_len.value == n_arc

    rec["zip_write_device"] = summary(series(call, reps))
    ctx.set_timing(True)
    rec["pack"] = summary(series(call, reps, value=lambda: ctx.stats().ms_main_kernel))
    ctx.set_timing(False)
    rec["pack"]["GBps_read_plus_written"] = 2 * payload / (rec["pack"]["median_ms"] * 1e-3) / 1e9
    copy_src = torch.empty(max(payload, 16), dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty_like(copy_src)
    rec["d2d_copy_same_bytes"] = summary(series(lambda: copy_dst.copy_(copy_src), reps))
    rec["d2d_copy_same_bytes"]["GBps_read_plus_written"] = 2 * payload / (rec["d2d_copy_same_bytes"]["median_ms"] * 1e-3) / 1e9

    # the batch deflate of the method 8 buffers alone
    dk = [k for k in range(count) if methods[k] == 8]
    bounds = [dmx.deflate_bound(sizes[k]) for k in dk]
    soffs, at = [], 0
    for b in bounds:
        soffs.append(at)
        at += (b + 15) & ~15
    slots = torch.empty(max(at, 16), dtype=torch.uint8, device="cuda")
    nd = len(dk)
    a_in = (ctypes.c_void_p * nd)(*[ptrs[k] for k in dk])
    a_n = (ctypes.c_size_t * nd)(*[sizes[k] for k in dk])
    a_out = (ctypes.c_void_p * nd)(*[slots.data_ptr() + o for o in soffs])
    a_cap = (ctypes.c_size_t * nd)(*bounds)
    res = (dmx.BatchResult * nd)()

    def deflate():
        assert dmx.lib().dmx_deflate_batch_device(ctx.h, a_in, a_n, nd, level, a_out, a_cap, res, None) == dmx.DMX_OK

    rec["deflate_batch_device"] = summary(series(deflate, reps))
    rec["remainder_ms"] = rec["zip_write_device"]["median_ms"] - rec["deflate_batch_device"]["median_ms"]

    # the host alternative: payloads down, serial assembly, archive up
    crcs = [e.crc for e in entries]
    state = {}

    def down():
        state["slots"] = slots.cpu().numpy().tobytes()
        state["plain"] = d_in.cpu().numpy().tobytes() if nd < count else b""

    def assemble():
        at_slot = dict(zip(dk, soffs))
        csize = dict(zip(dk, [r.bytes for r in res]))
        pay = [state["slots"][at_slot[k]:at_slot[k] + csize[k]] if methods[k] == 8 else
               state["plain"][offs[k]:offs[k] + sizes[k]] for k in range(count)]
        state["archive"] = host_assemble(names, methods, sizes, crcs, pay)

    def up():
        state["dev"] = torch.frombuffer(bytearray(state["archive"]), dtype=torch.uint8).cuda()

    hreps = max(3, reps // 3)
    d, a, u = summary(wall(down, hreps)), None, None
    a = summary(wall(assemble, hreps))
    u = summary(wall(up, hreps))
    same = state["archive"] == archive  # the same bytes, so the same work
    rec["host_alternative"] = {"d2h": d, "assemble_python": a, "h2d": u,
                               "sum_median_ms": d["median_ms"] + a["median_ms"] + u["median_ms"], "same_bytes": same}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--entries", type=int, default=64)
    ap.add_argument("--mib", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zip_write_probe.json"))
    args = ap.parse_args()
    ctx = dmx.Context()
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM}
    tiny = zw.tiny(65536)
    res["tiny_65536"] = probe(ctx, "tiny", [m[1] for m in tiny], [m[0] for m in tiny], [m[2] for m in tiny], args.reps)
    print(json.dumps({"tiny_65536": res["tiny_65536"]}), flush=True)
    part = args.mib << 20
    datas = [dmx.corpus("mixed", part, offset=k * part) for k in range(args.entries)]
    names = [b"shard_%03d.bin" % k for k in range(args.entries)]
    key = f"mixed_{args.entries}x{args.mib}MiB"
    res[key] = probe(ctx, key, datas, names, [8] * args.entries, args.reps)
    print(json.dumps({key: res[key]}), flush=True)
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
