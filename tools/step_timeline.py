"""Developer aid: every GPU operation of one timed round-trip step, in order, with the idle gaps.

Input: the CSV files of one
    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- \
        python bench.py --gpus 1 --steps 20 --warmup 5
run (counters belong in a run of their own, never with tracing).

argv: DIR (searched for *kernel_trace.csv and *memory_copy_trace.csv) [step index, default the
middle one of the last `--steps` steps] [--steps K, default 20].

A step is a deflate call followed by an inflate call.  The deflate call starts at the first
k_deflate_segments* after an inflate; the inflate call starts at k_marker_count.  For each
operation of the chosen step: name, start relative to the step's first operation, duration and
the gap to the latest end of the operations before it (0 when it overlaps one).  Then the summed
gaps of the deflate call, between the calls and of the inflate call; the time of the small
operations (everything but the front, emission, lane and 256-thread resolve kernels); the count
of runtime fill / copy kernels and memory copies; and the same sums as means over the timed steps.
"""
import csv
import glob
import os
import sys

BIG = ("k_deflate_segments", "k_deflate_emit", "k_inflate_lanes")


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError(names)


def short(name):
    s = name.replace("void ", "").replace("dmx::", "")
    cut = s.find("(")
    return s if cut < 0 else s[:cut]


def is_big(name):
    if any(b in name for b in BIG):
        return True
    return "k_inflate_resolve<" in name and not name.rstrip(">").endswith(" 64")


def load(d):
    ops = []
    for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            ops.append((int(col(r, "Start_Timestamp", "Start")), int(col(r, "End_Timestamp", "End")),
                        short(col(r, "Kernel_Name", "Name"))))
    for p in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            kind = r.get("Direction") or r.get("Kind") or "copy"
            ops.append((int(col(r, "Start_Timestamp", "Start")), int(col(r, "End_Timestamp", "End")),
                        "memcpy:" + kind))
    ops.sort()
    return ops


def steps_of(ops):
    """[(first op index, index of its k_marker_count, one past its last op)]"""
    out, i, n = [], 0, len(ops)
    while i < n:
        if "k_deflate_segments" not in ops[i][2]:
            i += 1
            continue
        j = i
        while j < n and "k_marker_count" not in ops[j][2]:
            j += 1
        if j == n:
            break
        k = j
        while k < n and "k_deflate_segments" not in ops[k][2]:
            k += 1
        # the step ends with the last k_inflate_validate before the next front kernel and the
        # result copies right behind it (what follows is the benchmark's own verification)
        e = k
        while e > j and ops[e - 1][2] != "k_inflate_validate":
            e -= 1
        if e == j:
            e = k
        while e < k and ("copyBuffer" in ops[e][2] or ops[e][2].startswith("memcpy")) and ops[e][0] - ops[e - 1][1] < 30_000:
            e += 1
        out.append((i, j, e))
        i = k
    return out


def sums(ops, st, detail=False):
    i, j, e = st
    t0, latest = ops[i][0], ops[i][0]
    g = {"deflate": 0, "between": 0, "inflate": 0}
    small = fills = copies = memcpy = 0
    for x in range(i, e):
        a, b, name = ops[x]
        gap = max(0, a - latest)
        g["deflate" if x < j else "between" if x == j else "inflate"] += gap
        if not is_big(name):
            small += b - a
        fills += "fillBuffer" in name
        copies += "copyBuffer" in name
        memcpy += name.startswith("memcpy")
        if detail:
            print(f"{name[:70]:70s} {(a - t0) / 1e3:10.1f} {(b - a) / 1e3:9.1f} {gap / 1e3:8.1f}")
        latest = max(latest, b)
    return g, small, fills, copies, memcpy, latest - t0, e - i


def main():
    args = [a for a in sys.argv[1:]]
    nsteps = 20
    if "--steps" in args:
        k = args.index("--steps")
        nsteps = int(args[k + 1])
        del args[k:k + 2]
    ops = load(args[0])
    steps = steps_of(ops)
    timed = steps[-nsteps:] if len(steps) >= nsteps else steps
    pick = int(args[1]) if len(args) > 1 else len(timed) // 2
    print(f"{len(ops)} operations, {len(steps)} steps; step {pick} of the last {len(timed)}")
    print(f"{'operation':70s} {'start us':>10s} {'dur us':>9s} {'gap us':>8s}")
    g, small, fills, copies, memcpy, span, nops = sums(ops, timed[pick], detail=True)
    print(f"step {pick}: {nops} operations over {span / 1e3:.1f} us; gaps: deflate call {g['deflate'] / 1e3:.1f} us, "
          f"between the calls {g['between'] / 1e3:.1f} us, inflate call {g['inflate'] / 1e3:.1f} us; "
          f"small operations {small / 1e3:.1f} us; runtime fill kernels {fills}, runtime copy kernels {copies}, "
          f"memory copies {memcpy}")
    acc = [sums(ops, s) for s in timed]
    m = len(acc)
    print(f"mean of {m} steps: {sum(a[6] for a in acc) / m:.1f} operations over {sum(a[5] for a in acc) / m / 1e3:.1f} us; "
          f"gaps: deflate call {sum(a[0]['deflate'] for a in acc) / m / 1e3:.1f} us, "
          f"between the calls {sum(a[0]['between'] for a in acc) / m / 1e3:.1f} us, "
          f"inflate call {sum(a[0]['inflate'] for a in acc) / m / 1e3:.1f} us; "
          f"small operations {sum(a[1] for a in acc) / m / 1e3:.1f} us; "
          f"runtime fill kernels {sum(a[2] for a in acc) / m:.2f}, runtime copy kernels {sum(a[3] for a in acc) / m:.2f}, "
          f"memory copies {sum(a[4] for a in acc) / m:.2f}")


if __name__ == "__main__":
    main()
