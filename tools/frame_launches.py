#!/usr/bin/env python3
"""Per-launch times of selected kernels over the last forwards of a rocprofv3 --kernel-trace CSV (a forward = the launches from one
marker kernel to the next; tools/frame_kernels.py shows one forward by kernel): median, min and max per launch over the last N
forwards, and the whole-forward kernel time.
tools/frame_launches.py <kernel_trace.csv> <marker substring> <N> <kernel substring> [...]"""
import csv
import statistics
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
marker, nframes, wanted = sys.argv[2], int(sys.argv[3]), sys.argv[4:]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
idx = [i for i, r in enumerate(rows) if marker in r["Kernel_Name"]]
frames = [rows[a:b] for a, b in zip(idx[:-1], idx[1:])][-nframes:]
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
total = [sum(dur(r) for r in f) for f in frames]
print(f"{len(frames)} forwards of {len(frames[-1])} launches; kernel time per forward (us): " + " ".join(f"{t:.1f}" for t in total))
print(f"kernel time: median {statistics.median(total):.1f} us, min {min(total):.1f}, max {max(total):.1f}")
per = {}
for f in frames:
    seen = {}
    for r in f:
        name = r["Kernel_Name"]
        if any(w in name for w in wanted):
            k = (name, seen.get(name, 0))
            seen[name] = k[1] + 1
            per.setdefault(k, []).append((dur(r), r.get("Grid_Size", "?"), r.get("VGPR_Count", r.get("Arch_VGPR_Count", "?"))))
for (name, n), v in per.items():
    t = [d for d, _, _ in v]
    short = name.replace("void mvd::", "").replace("mvd::", "").split("(")[0]
    print(f"  {short:44s} #{n} grid {v[0][1]:>8} vgpr {v[0][2]:>4}  median {statistics.median(t):7.1f} us  min {min(t):7.1f} max {max(t):7.1f}")
