#!/usr/bin/env python3
"""Times of star detection on the device (stars.hip: star.FindStars).

  python tools/stars_probe.py --out DIR
      wall time per call (median of 20 after 3 warm-up calls; every call ends in host work on the short lists and a
      stream sync, so this is device time plus launch, sync and host overhead) of
        resident form                 nl_stack_frame_find_stars on a 4096^2 field of ~2 000 stars (defaults of the
                                      `stack` command: starSig 15, radius 16, starInOut 1.4, bpSigma 5, given std)
        resident form, nil stats      the same with diff_std NaN (deviation 1: the std over the whole frame)
        resident form, adversarial    a bright extended region (a 1024 x 1024 plateau with noise): many candidates
        host form                     nl_find_stars (64 MiB over PCIe, then the same)
      then runs the calls once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time
      limit) and prints every star kernel's per-dispatch durations, with the scan kernel's share of the MI355X's
      8 TB/s HBM peak.  DIR receives the summary (stars_probe.txt) and the trace.
"""
import argparse
import csv
import glob
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
N = W * H
HBM_PEAK = 8.0e12
BYTES = {"star_scan_kernel": 4 * N}           # the frame, read once
STD = 12.5


def fields():
    rng = np.random.default_rng(5)
    img = 1000.0 + 10.0 * rng.standard_normal((H, W))
    yy, xx = np.mgrid[-12:13, -12:13]
    for _ in range(2000):
        x0, y0 = rng.uniform(20, W - 20), rng.uniform(20, H - 20)
        peak, sigma = 10.0 ** rng.uniform(2.0, 4.5), rng.uniform(0.8, 2.5)
        ix, iy = int(x0), int(y0)
        img[iy - 12:iy + 13, ix - 12:ix + 13] += peak * np.exp(-((xx + ix - x0) ** 2 + (yy + iy - y0) ** 2)
                                                                / (2 * sigma * sigma))
    natural = img.astype(np.float32)
    adv = natural.copy()
    adv[1500:2524, 1500:2524] += 5000.0 + 100.0 * rng.standard_normal((1024, 1024))
    return natural.reshape(-1), adv.reshape(-1)


def median_ms(fn, reps, warm=3):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def run_calls(reps):
    import nightlight_amd as nl
    natural, adv = fields()
    loc, scale = np.float32(1000.0), np.float32(10.0)
    lines = []
    with nl.StackHandle(2, W, H) as st:
        st.upload_frame(0, natural)
        st.upload_frame(1, adv)
        for name, idx, ds in (("natural", 0, STD), ("natural, nil stats", 0, None), ("adversarial", 1, STD)):
            stars, _, hfr = st.frame_find_stars(idx, loc, scale, diff_std=ds)
            med, mn = median_ms(lambda: st.frame_find_stars(idx, loc, scale, diff_std=ds), reps)
            lines.append("resident form 4096^2 %s: median %.3f ms, min %.3f ms, %d stars, avg HFR %.4f"
                         % (name, med, mn, stars.size, hfr))
    med, mn = median_ms(lambda: nl.find_stars(natural, W, H, loc, scale, diff_std=STD), max(5, reps // 4))
    lines.append("host form nl_find_stars 4096^2 natural: median %.3f ms, min %.3f ms" % (med, mn))
    return lines


def dispatches(trace):
    """{kernel name: [duration ns of every dispatch]} from rocprofv3's results database or kernel_trace.csv."""
    out = {}
    dbs = glob.glob(os.path.join(trace, "**", "*.db"), recursive=True)
    if dbs:
        rows = sqlite3.connect(dbs[0]).execute("select name, end - start from kernels")
    else:
        csvs = glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)
        rows = []
        if csvs:
            with open(csvs[0]) as f:
                rows = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(f)]
    for name, ns in rows:
        out.setdefault(name.replace("(anonymous namespace)::", "").split("(")[0], []).append(float(ns))
    return out


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "stars_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per-dispatch min / median / max in us over the natural (given and nil stats)",
             "and adversarial calls; share = algorithmic bytes / min / 8 TB/s"]
    for name, ns in sorted(dispatches(trace).items(), key=lambda kv: -np.median(kv[1])):
        if "star_" not in name:
            continue
        med = float(np.median(ns))
        key = next((k for k in BYTES if k in name), None)
        share = ""
        if key:
            share = "  %4.0f MB  %3.0f %%" % (BYTES[key] / 1e6, 100.0 * BYTES[key] / (min(ns) * 1e-9) / HBM_PEAK)
        lines.append("%-40s %4d %9.1f %9.1f %9.1f%s" % (name[-40:], len(ns), min(ns) / 1e3, med / 1e3, max(ns) / 1e3,
                                                         share))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true", help="the calls only (the run under rocprofv3)")
    ap.add_argument("--out", required=True, help="directory for the summary and the rocprofv3 trace")
    a = ap.parse_args()
    if a.inner:
        run_calls(5)
        return
    os.makedirs(a.out, exist_ok=True)
    lines = run_calls(20) + [""] + kernel_stats(a.out)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "stars_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
