"""Developer probe: per-phase cycle breakdown of the deflate / inflate kernels (DMX_PHASES)."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deflate.hpp_amd"))
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "gpurun_out", "phases.txt")
os.environ["DMX_PHASES"] = out
import torch  # noqa: E402
import dmx  # noqa: E402
ctx = dmx.Context(segment_bytes=int(os.environ.get("DMX_SEG", "32768")))
ctx.set_timing(True)
n = int(os.environ.get("DMX_MIB", "256")) << 20
for kind in os.environ.get("DMX_KINDS", "repeat,text,zeros").split(","):
    host = torch.empty(n, dtype=torch.uint8).pin_memory()
    dmx.corpus_into(kind, n, host.data_ptr())
    d_in = host.cuda()
    cap = dmx.deflate_bound(n) + 64
    d_c = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_o = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    with open(out, "a") as f:
        f.write(f"# corpus {kind}\n")
    for lvl in (int(os.environ.get("DMX_LEVEL", "2")),):
        clen = ctx.deflate_device(d_in.data_ptr(), n, lvl, d_c.data_ptr(), cap)
        kd = ctx.stats().ms_main_kernel
        olen = ctx.inflate_device(d_c.data_ptr(), clen, d_o.data_ptr(), n + 64)
        ki = ctx.stats().ms_main_kernel
        with open(out, "a") as f:
            f.write(f"# {kind} L{lvl} ratio {n/clen:.3f} deflate_kernel_ms {kd:.3f} inflate_kernel_ms {ki:.3f} ok {olen == n and torch.equal(d_o[:n], d_in)}\n")
print(open(out).read())

# The front kernel's phases per corpus, cycles per segment from wave 0's stamps (the rows of
# profiles/r0N_variants.txt), and what no phase counts: the interval from a segment's token words
# (stamp 11) to the loaded image of the same workgroup's next segment (stamp 1 of seg + grid).
COLS = "load | round 0 | round 1 | to stamp 14 | bitmap + fill | parse walk | fix-up + token ranges | token words | prefetch | total | 11 -> next 1 | 10 -> next 0"
print("# " + COLS)
kind = None
for line in open(out):
    if line.startswith("# corpus "):
        kind = line.split()[2]
    elif line.startswith("deflate ") and kind:
        v = dict(kv.split("=") for kv in line.split()[2:] if "=" in kv)
        t = lambda k: float(v.get("t%d" % k, 0))  # noqa: E731
        row = [t(1), t(12) - t(1), t(13) - t(12), t(14) - t(13), t(2) - t(14), t(3) - t(2), t(15) - t(3),
               t(11) - t(15), t(10) - t(11), t(10), float(v.get("gap", 0)), float(v.get("gap0", 0))]
        print(f"{kind}: {os.environ.get('DMX_TAG', '')}  " + " | ".join("%.0f" % x for x in row))
        kind = None
