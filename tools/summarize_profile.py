#!/usr/bin/env python3
"""Condense gpurun_out/prof_<tag>/ (tools/profile_bench.sh) into the small summaries kept under profiles/."""
import collections
import csv
import json
import os
import sys


def short(name):
    return name.split("(")[0].replace("void ", "")


def main(tag, rnd):
    src = os.path.join("gpurun_out", "prof_" + tag)
    dst = "profiles"
    # 1. kernel stats (rocprofv3 --kernel-trace --stats)
    rows = list(csv.DictReader(open(os.path.join(src, "trace", "t_kernel_stats.csv"))))
    with open(os.path.join(dst, "%s_kernel_stats.csv" % rnd), "w") as f:
        f.write("Name,Calls,TotalDurationNs,AverageNs,Percentage,MinNs,MaxNs\n")
        for r in rows:
            f.write('"%s",%s,%s,%s,%s,%s,%s\n' % (short(r["Name"]), r["Calls"], r["TotalDurationNs"], r["AverageNs"],
                                              r["Percentage"], r["MinNs"], r["MaxNs"]))
    written_stats = True
    avg_ns = {short(r["Name"]): float(r["AverageNs"]) for r in rows}
    # The public-key kernels are launched twice per call (two-phase planning); the phase-2 launch normally has nothing to do
    # and lasts ~5 us, which halves the --stats average.  Per-dispatch durations from the kernel trace give the average over
    # the launches that did work (>= 10 % of the kernel's longest launch) -- the figure bench.py's HIP events measure.
    nonempty, in_order = {}, {}
    tp = os.path.join(src, "trace", "t_kernel_trace.csv")
    if os.path.exists(tp):
        per = collections.defaultdict(list)
        for r in csv.DictReader(open(tp)):
            per[short(r["Kernel_Name"])].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for k, v in per.items():
            big = [x for x in v if x >= 0.1 * max(v)]
            nonempty[k] = (sum(big) / len(big), len(big), len(v))
        in_order = {k: [round(x / 1e6, 3) for x in v] for k, v in per.items() if max(v) >= 1e6 and len(v) <= 200}   # ms, launch order
    with open(os.path.join(dst, "%s_kernel_stats.csv" % rnd), "a") as f:
        pass
    # 2. HBM counters, one pass each
    def agg(path, counter):
        d = collections.defaultdict(list)
        if not os.path.exists(path):
            return {}
        for r in csv.DictReader(open(path)):
            if r["Counter_Name"] == counter:
                d[short(r["Kernel_Name"])].append(float(r["Counter_Value"]))
        out = {}
        for k, v in d.items():
            big = [x for x in v if x >= 0.1 * max(v)] if max(v) > 0 else v
            out[k] = sum(big) / len(big)
        return out
    fetch = agg(os.path.join(src, "pmc_fetch", "f_counter_collection.csv"), "FETCH_SIZE")
    write = agg(os.path.join(src, "pmc_write", "w_counter_collection.csv"), "WRITE_SIZE")
    sq = collections.defaultdict(dict)
    p = os.path.join(src, "pmc_sq", "s_counter_collection.csv")
    if os.path.exists(p):
        tmp = collections.defaultdict(lambda: collections.defaultdict(list))
        for r in csv.DictReader(open(p)):
            tmp[short(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k in tmp:
            sq[k] = {}
            for c, v in tmp[k].items():
                big = [x for x in v if x >= 0.1 * max(v)] if max(v) > 0 else v
                sq[k][c] = sum(big) / len(big)
    plain = json.loads(open(os.path.join(src, "bench_plain.json")).read().strip().splitlines()[-1])
    out = {"source": "rocprofv3 separate --pmc passes (FETCH_SIZE | WRITE_SIZE | SQ_*) over the bench command of tools/profile_bench.sh "
                     "(`python bench.py --config N --full --steps 5 --warmup 2 --no-cpu-baseline`)",
           "correction": "MI355X_MICROARCH.md HBM section: on gfx950 FETCH_SIZE reports 1/2 of the bytes moved -> doubled; calibrated "
                         "for this path's access patterns (profiles/r03_fetch_size_calibration.csv: FETCH_SIZE = 1/2 x 128 B x lines "
                         "touched for streaming and scattered reads alike, WRITE_SIZE exact); both are KiB per dispatch",
           "workload": plain["config"], "kernels": {}}
    with open(os.path.join(dst, "%s_pmc_hbm.csv" % rnd), "w") as f:
        f.write("Kernel,AvgDurationNs,FETCH_SIZE_KiB_raw,WRITE_SIZE_KiB_raw,HBM_bytes_corrected\n")
        for k in sorted(set(fetch) | set(write), key=lambda k: -(fetch.get(k, 0) + write.get(k, 0))):
            if not k.startswith("bftkv::"):
                continue
            b = int((2 * fetch.get(k, 0) + write.get(k, 0)) * 1024)
            f.write('"%s",%.0f,%.1f,%.1f,%d\n' % (k, avg_ns.get(k, 0), fetch.get(k, 0), write.get(k, 0), b))
            out["kernels"][k] = {"avg_ns": avg_ns.get(k, 0),
                                 "avg_ns_working_launches": nonempty.get(k, (avg_ns.get(k, 0), 0, 0))[0],
                                 "working_launches": "%d of %d" % nonempty.get(k, (0, 0, 0))[1:], "fetch_kib_raw": fetch.get(k, 0), "write_kib_raw": write.get(k, 0),
                                 "hbm_bytes_corrected": b, "sq": sq.get(k, {})}
            if k in in_order:
                # every launch of the profiled command in order (ms): warm-up, the timed region's launches (batches in flight: a launch
                # queued behind the turnstile starts as its predecessor drains and its span is not the kernel alone), and -- cfg 2 --
                # the three NON-OVERLAPPED calls bench.py makes after the timed region, whose durations are the kernel's own and are what
                # `kernel_ms.single_flight.rsa` (HIP events) reports
                out["kernels"][k]["launch_ms_in_order"] = in_order[k]
    with open(os.path.join(dst, "%s_pmc_summary.json" % rnd), "w") as f:
        json.dump(out, f, indent=1)
    for n in ("bench_plain.json", "bench_trace.json"):
        with open(os.path.join(src, n)) as g, open(os.path.join(dst, "%s_%s" % (rnd, n)), "w") as f:
            f.write(g.read())
    print("wrote profiles/%s_*" % rnd)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
