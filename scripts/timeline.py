#!/usr/bin/env python3
"""Prints the last N kernel dispatches of a rocprofv3 kernel trace as a timeline (us since the first
one shown): start, end, duration, queue, kernel — to see which launches overlap."""
import csv, glob, os, sys
d = sys.argv[1]; n = int(sys.argv[2]) if len(sys.argv) > 2 else 60
rows = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        for k in ("k_raster_queue", "k_raster", "k_frame", "k_setup_wave", "k_setup", "k_count_wave", "k_scan", "k_fill_wave", "k_fill"):
            if k in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], k))
                break
rows.sort()
rows = rows[-n:]
t0 = rows[0][0]
for a, b, q, k in rows:
    print(f"{(a - t0) / 1e3:10.1f} {(b - t0) / 1e3:10.1f} {(b - a) / 1e3:9.1f}us q={q} {k}")
# Summary over ALL k_frame dispatches of the trace: how many were in flight at once at the most (a sweep over
# the start and end times, ends before starts at equal times), on how many queues, and their scratch.
frames = []
for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_frame" in r["Kernel_Name"]:
            frames.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"],
                           r.get("Scratch_Size", r.get("Private_Segment_Size", "?"))))
if frames:
    edges = sorted([(a, 1) for a, _, _, _ in frames] + [(b, 0) for _, b, _, _ in frames])
    live = most = 0
    hist = {}
    last = edges[0][0]
    for t, start in edges:
        hist[live] = hist.get(live, 0) + (t - last)
        last = t
        live += 1 if start else -1
        most = max(most, live)
    busy = sum(v for k, v in hist.items() if k > 0) or 1
    share = " ".join(f"{k}:{100.0 * v / busy:.0f}%" for k, v in sorted(hist.items()) if k > 0)
    print(f"k_frame dispatches={len(frames)} max_overlapping={most} queues={len({q for _, _, q, _ in frames})} "
          f"scratch={','.join(sorted({s for _, _, _, s in frames}))}  time with n in flight, of the time with any: {share}")
