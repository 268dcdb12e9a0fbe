#!/usr/bin/env python3
"""Times of the colour-camera front on the device (bayer.hip: OpBadPixel's Bayer branch, OpDebayer).

  python tools/bayer_probe.py --out DIR
      wall time per call (median of 20 after 3 warm-up calls; every call ends in a stream sync) on a 4096^2 RGGB
      mosaic (~0.2 % hot, ~0.1 % cold pixels), dark + flat masters, of
        resident, debayer only         nl_stack_upload_frame_cfa, sigma 0 (raw upload + calibrate + debayer)
        resident, correction + debayer nl_stack_upload_frame_cfa, sigma 3 / 5, channels R and G
        host form                      nl_preprocess_frame_cfa, channel G (64 MiB in, 64 MiB out over PCIe)
      The resident calls include the raw mosaic's host-to-device copy; the device-side step is taken from the trace.
      Then the calls run once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time
      limit): every bayer / debayer / calibrate kernel's per-dispatch durations with its algorithmic bytes and share
      of the MI355X's 8 TB/s HBM peak, and the span of one correction + debayer (first bayer_median_kernel start to
      the following debayer_kernel end).  DIR receives the summary (bayer_probe.txt) and the trace.
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
RB = (W // 2) * (H // 2)          # red or blue pixels of the mosaic
G = N // 2
# algorithmic bytes per launch (the same-colour halo comes from cache); R = red, G = green channel
BYTES = {
    "calibrate_kernel": 4 * 4 * N,                 # raw in, dark, flat, raw out
    "debayer_kernel": 2 * 4 * N,                   # raw in once, plane out once
    "bayer_median_kernel R": 4 * N + 8 * RB,       # raw in (its lines hold every colour), delta + median out
    "bayer_median_kernel G": 4 * N + 8 * G,
    "bayer_rowsum_kernel R": 4 * RB,
    "bayer_rowsum_kernel G": 4 * G,
    "bayer_replace_kernel R": 8 * RB,              # delta + median in (the few replaced pixels written)
    "bayer_replace_kernel G": 8 * G,
}


def mosaic():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    level = np.where((yy & 1) == (xx & 1), 1200.0, 900.0) + 100.0 * (yy & 1)
    img = level + 150.0 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 30.0 * rng.standard_normal((H, W))
    hot = rng.random((H, W)) < 0.002
    img[hot] += 5000.0 * rng.random(np.count_nonzero(hot))
    cold = rng.random((H, W)) < 0.001
    img[cold] -= 900.0 * rng.random(np.count_nonzero(cold))
    dark = (50.0 + 5.0 * rng.standard_normal(N)).astype(np.float32)
    flat = (0.8 + 0.2 * rng.random(N)).astype(np.float32)
    return (img.astype(np.float32) + np.float32(100)).reshape(-1), dark, flat


def median_ms(fn, reps, warm=3):
    t = []
    r = None
    for k in range(warm + reps):
        t0 = time.perf_counter()
        r = fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t)), r


def run_calls(reps):
    import nightlight_amd as nl
    raw, dark, flat = mosaic()
    ow, oh = nl.debayer_shape(W, H, "G", "RGGB")
    lines = []
    with nl.Calibration(0, W, H, dark=dark, flat=flat) as c, nl.StackHandle(1, ow, oh) as st:
        med, mn, _ = median_ms(lambda: st.upload_frame_cfa(0, raw, W, H, "G", "RGGB", calib=c, sigma_low=0.0), reps)
        lines.append("resident, debayer only (G, RGGB, dark + flat) 4096^2: median %.3f ms, min %.3f ms" % (med, mn))
        for ch in ("R", "G"):
            med, mn, r = median_ms(lambda: st.upload_frame_cfa(0, raw, W, H, ch, "RGGB", calib=c), reps)
            lines.append("resident, correction + debayer (%s, RGGB, dark + flat) 4096^2: median %.3f ms, min %.3f ms,"
                         " removed %d, delta mean %.4f std %.4f" % (ch, med, mn, r[0], r[1][0], r[1][1]))
        med, mn, _ = median_ms(lambda: nl.preprocess_frame_cfa(raw, W, H, "G", "RGGB", calib=c), max(5, reps // 4))
        lines.append("host form nl_preprocess_frame_cfa (G, RGGB, dark + flat) 4096^2: median %.3f ms, min %.3f ms"
                     % (med, mn))
    return lines


def trace_rows(trace):
    """[(name, start ns, end ns)] in start order from rocprofv3's results database or kernel_trace.csv."""
    dbs = glob.glob(os.path.join(trace, "**", "*.db"), recursive=True)
    if dbs:
        rows = list(sqlite3.connect(dbs[0]).execute("select name, start, end from kernels"))
    else:
        rows = []
        for path in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)[:1]:
            with open(path) as f:
                rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
                        for r in csv.DictReader(f)]
    rows = [(n.replace("(anonymous namespace)::", "").split("(")[0], int(s), int(e)) for n, s, e in rows]
    return sorted(rows, key=lambda r: r[1])


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "bayer_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    rows = [r for r in trace_rows(trace) if "bayer_" in r[0] or "debayer_kernel" in r[0] or "calibrate_kernel" in r[0]]
    # one correction = bayer_median_kernel ... debayer_kernel<channel, ...>: its kernels keyed by that channel
    per, spans, call = {}, {}, []
    for name, s, e in rows:
        if "bayer_median_kernel" in name:
            call = [(name, s, e)]
        elif call:
            call.append((name, s, e))
        if "debayer_kernel" in name and call:
            call_key = "G" if "<1," in name else "R" if "<0," in name else "B"
            spans.setdefault(call_key, []).append((e - call[0][1]) / 1e3)
            for n, s2, e2 in call:
                if "debayer_kernel" in n:
                    continue
                key = n + " " + call_key
                per.setdefault(key, []).append((e2 - s2) / 1e3)
            call = []
        if "debayer_kernel" in name or "calibrate_kernel" in name:
            per.setdefault(name, []).append((e - s) / 1e3)
    lines = ["rocprofv3 --kernel-trace: per-dispatch min / median / max in us; share = algorithmic bytes / median / 8 TB/s"]
    for name, us in sorted(per.items(), key=lambda kv: -np.median(kv[1])):
        med = float(np.median(us))
        base = name.replace("void ", "").replace("nl::", "").split("<")[0].split(" ")[0]
        chan = name.split(" ")[-1] if name[-2:] in (" R", " G") else ""
        key = next((k for k in (base + " " + chan, base) if k in BYTES), None)
        share = ""
        if key:
            share = "  %4.0f MB  %3.0f %%" % (BYTES[key] / 1e6, 100.0 * BYTES[key] / (med * 1e-6) / HBM_PEAK)
        lines.append("%-46s %4d %8.1f %8.1f %8.1f%s" % (name[-46:], len(us), min(us), med, max(us), share))
    for ch, us in sorted(spans.items()):
        lines.append("correction + debayer span, channel %s (bayer_median start to debayer end): median %.1f us over %d"
                     " calls" % (ch, float(np.median(us)), len(us)))
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
    with open(os.path.join(a.out, "bayer_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
