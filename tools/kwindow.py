"""usage: kwindow.py <kernel_trace.csv> <marker> <steps> [rows=25]: per-step kernel table over the LAST `steps` steps of a
rocprofv3 --kernel-trace run of tools/model_step_profile.py (35 steps: 5 warm-up + 30 timed).  The window opens at the
first launch of that step's `marker` kernel (a name fragment of the first layer's aggregation), so the data-path kernels
that fetched the resident batch stay out of the table (kstats.py over --stats counts the whole process)."""
import collections
import csv
import sys

path, marker, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
starts = [int(r["Start_Timestamp"]) for r in rows if marker in r["Kernel_Name"]]
per = len(starts) // 35                                  # marker launches per step
t0 = starts[len(starts) - steps * per]
agg = collections.defaultdict(lambda: [0, 0])
for r in rows:
    if int(r["Start_Timestamp"]) >= t0:
        a = agg[r["Kernel_Name"]]
        a[0] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        a[1] += 1
for name, (ns, calls) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:int(sys.argv[4]) if len(sys.argv) > 4 else 25]:
    print(f"{ns / steps / 1e3:8.1f} us/step {calls / steps:5.1f}/step {ns / calls / 1e3:7.1f} us  {name[:110]}")
print(f"{sum(v[0] for v in agg.values()) / steps / 1e3:8.1f} us/step total kernel time")
