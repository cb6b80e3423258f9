"""Developer aid: what a rocprofv3 --kernel-trace CSV says about the deflate's chunk pipeline.

argv: kernel_trace.csv files.  Per file: calls and mean duration of the front (k_deflate_segments*)
and emission (k_deflate_emit*) kernels; the share of the emission kernels' time that lies inside a
front kernel's interval; the idle gap between consecutive front kernels of one call (the chunk
boundary: end of one front kernel to the start of the next, gaps above 0.3 ms separate calls);
and the mean deflate window per call (first front start to last emission end).
"""
import csv
import sys
from collections import defaultdict


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    raise KeyError(names)


for path in sys.argv[1:]:
    front, emit, dur = [], [], defaultdict(list)
    for row in csv.DictReader(open(path)):
        name = col(row, "Kernel_Name", "Name")
        a, b = int(col(row, "Start_Timestamp", "Start")), int(col(row, "End_Timestamp", "End"))
        short = name.split("(")[0].replace("void ", "").replace("dmx::", "")
        if "k_deflate_segments" in name:
            front.append((a, b))
            dur[short].append(b - a)
        elif "k_deflate_emit" in name:
            emit.append((a, b))
            dur[short].append(b - a)
    front.sort()
    emit.sort()
    print(f"== {path}")
    for k, v in sorted(dur.items()):
        print(f"  {k[:60]:60s} {len(v):5d} calls  mean {sum(v) / len(v) / 1e3:9.1f} us")
    if not front or not emit:
        continue
    # emission time inside a front interval (front kernels of one stream never overlap each other)
    inside = total = 0
    j = 0
    for a, b in emit:
        total += b - a
        while j < len(front) and front[j][1] <= a:
            j += 1
        k = j
        while k < len(front) and front[k][0] < b:
            inside += max(0, min(b, front[k][1]) - max(a, front[k][0]))
            k += 1
    print(f"  emission time inside a front kernel's interval: {100.0 * inside / total:.1f} %")
    gaps = [front[i + 1][0] - front[i][1] for i in range(len(front) - 1)]
    gaps = [g for g in gaps if g < 300_000]
    if gaps:
        print(f"  chunk-boundary gaps: {len(gaps)}  mean {sum(gaps) / len(gaps) / 1e3:.1f} us  "
              f"max {max(gaps) / 1e3:.1f} us")
    # calls: a front kernel more than 0.3 ms after the previous one's end starts a new call
    calls, start = [], front[0][0]
    ends = []
    for i in range(len(front)):
        if i + 1 == len(front) or front[i + 1][0] - front[i][1] >= 300_000:
            nxt = front[i + 1][0] if i + 1 < len(front) else 1 << 62
            last = max([b for a, b in emit if start <= a < nxt] + [front[i][1]])
            calls.append(last - start)
            ends.append(last - front[i][1])
            if i + 1 < len(front):
                start = front[i + 1][0]
    print(f"  deflate window (first front start to last emission end): {len(calls)} calls  "
          f"mean {sum(calls) / len(calls) / 1e3:.1f} us; tail after the last front kernel mean "
          f"{sum(ends) / len(ends) / 1e3:.1f} us")
