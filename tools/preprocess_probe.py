#!/usr/bin/env python3
"""Times of OpCalibrate / OpBadPixel on the device (preprocess.hip).

  python tools/preprocess_probe.py --out DIR
      wall time per call (median of 20 after 3 warm-up calls; every call ends in a stream sync, so this is
      device time plus launch and sync overhead) of
        resident calibrate (dark + flat)        nl_stack_frame_calibrate on a 4096^2 slot
        resident bad-pixel step                 nl_stack_frame_badpixel, natural 4096^2 frame (~0.2 % hot)
        resident bad-pixel step, adversarial    hot column + hot row + 64x64 hot block on top
        host form                               nl_preprocess_frame (calibrate + bad pixels, 2 x 64 MiB PCIe)
      then runs the calls once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time
      limit) and prints every preprocess kernel's per-dispatch durations with its algorithmic bytes and share of
      the MI355X's 8 TB/s HBM peak.  DIR receives the summary (preprocess_probe.txt) and the trace.
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
# algorithmic bytes per launch (4 B per pixel per stream; the 3x3 halo comes from cache)
BYTES = {
    "calibrate_kernel": 4 * 4 * N,           # light in, dark, flat, light out
    "bp_diff_kernel": 2 * 4 * N,             # frame in, diff out
    "bp_variance_kernel": 4 * N,             # diff in
    "bp_classify_kernel": 4 * N,             # diff in (+ the few bad pixels' neighbourhoods)
}


def frames():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    img = 1000.0 + 150.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 30.0 * rng.standard_normal((H, W))
    hot = rng.random((H, W)) < 0.002
    img[hot] += 5000.0 * rng.random(np.count_nonzero(hot))
    natural = img.astype(np.float32)
    adv = natural.copy()
    adv[:, 1000] += 20000.0
    adv[2000, :] += 20000.0
    adv[3000:3064, 500:564] += 20000.0
    dark = (50.0 + 5.0 * rng.standard_normal(N)).astype(np.float32)
    flat = (0.8 + 0.2 * rng.random(N)).astype(np.float32)
    return natural.reshape(-1), adv.reshape(-1), dark, flat


def median_ms(fn, reps, warm=3):
    t = []
    for k in range(warm + reps):
        dt, _ = fn()
        if k >= warm:
            t.append(dt)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def run_calls(reps):
    import nightlight_amd as nl
    natural, adv, dark, flat = frames()
    lines = []
    with nl.Calibration(0, W, H, dark=dark, flat=flat) as c, nl.StackHandle(2, W, H) as st:
        st.upload_frame(0, natural)
        med, mn = median_ms(lambda: clock(lambda: st.frame_calibrate(0, c)), reps)
        lines.append("resident calibrate 4096^2 (dark + flat): median %.3f ms, min %.3f ms" % (med, mn))
        for name, idx, frame in (("natural", 0, natural), ("adversarial", 1, adv)):
            result = []

            def one():
                st.upload_frame(idx, frame)              # (untimed: every call starts from the raw frame)
                dt, r = clock(lambda: st.frame_badpixel(idx, 3.0, 5.0))
                result[:] = [r]
                return dt, r
            med, mn = median_ms(one, reps)
            removed, stats = result[0]
            lines.append("resident bad-pixel step 4096^2 %s: median %.3f ms, min %.3f ms, removed %d, diff std %.4f"
                         % (name, med, mn, removed, stats[1]))
        med, mn = median_ms(lambda: clock(lambda: nl.preprocess_frame(natural, W, H, calib=c)), max(5, reps // 4))
        lines.append("host form nl_preprocess_frame 4096^2 (calibrate + bad pixels): median %.3f ms, min %.3f ms"
                     % (med, mn))
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
    trace = os.path.join(out_dir, "preprocess_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per-dispatch min / median / max in us (the natural and the adversarial frame",
             "alternate: min = natural, max = adversarial where they differ); share = algorithmic bytes / median / 8 TB/s"]
    for name, ns in sorted(dispatches(trace).items(), key=lambda kv: -np.median(kv[1])):
        if "calibrate_kernel" not in name and "bp_" not in name:
            continue
        med = float(np.median(ns))
        key = next((k for k in BYTES if k in name), None)
        share = ""
        if key:
            share = "  %4.0f MB  %3.0f %%" % (BYTES[key] / 1e6, 100.0 * BYTES[key] / (med * 1e-9) / HBM_PEAK)
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
    with open(os.path.join(a.out, "preprocess_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
