#!/usr/bin/env python3
"""Times of debanding and binning on the device (deband.hip: OpDebandHoriz, OpDebandVert, OpBin).

  python tools/deband_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; every deband call ends in the host's window steps and a
      stream sync, so this is device time plus launch, copy, sync and host overhead) of nl_stack_frame_deband_horiz,
      nl_stack_frame_deband_vert (percentile 50, window 128, sigma 3: the reference's defaults) and
      nl_stack_frame_bin_from (n = 2, 3, 4) on a banded 4096^2 sky; then runs the calls once more under
      `rocprofv3 --kernel-trace --stats` (a child process with its own time limit) and prints every kernel's
      per-dispatch durations, with the scale kernel's share of the MI355X's 8 TB/s HBM peak.  DIR receives the summary
      (deband_probe.txt) and the trace.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stars_probe import dispatches  # noqa: E402

W = H = 4096
N = W * H
HBM_PEAK = 8.0e12
# algorithmic bytes: the frame read once and written once (scale, transpose); the frame read once, the keys stay in
# LDS (row percentile)
BYTES = {"deband_scale_kernel": 8 * N, "deband_transpose_kernel": 8 * N, "deband_row_percentile_kernel": 4 * N}
BINS = (2, 3, 4)


def sky():
    rng = np.random.default_rng(5)
    rows = 1.0 + 0.03 * np.sin(np.arange(H) * 0.9)
    cols = 1.0 + 0.03 * np.cos(np.arange(W) * 0.7)
    img = (1000.0 + 10.0 * rng.standard_normal((H, W), dtype=np.float32)) * rows[:, None] * cols[None, :]
    return img.astype(np.float32).reshape(-1)


def median_ms(fn, reps, warm=2):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def run_calls(reps):
    import nightlight_amd as nl
    data = sky()
    loc = np.float32(np.median(data))
    scale = np.float32(1.4826 * np.median(np.abs(data - loc)))
    lines = []
    with nl.StackHandle(1, W, H) as st:
        up, _ = median_ms(lambda: st.upload_frame(0, data), reps)
        for name, call in (("frame_deband_horiz", st.frame_deband_horiz), ("frame_deband_vert", st.frame_deband_vert)):
            def step():
                st.upload_frame(0, data)          # the step is in place: every call starts from the same frame
                return call(0, 50.0, 128, 3.0, loc, scale)
            info = step()
            med, mn = median_ms(step, reps)
            lines.append("%-18s 4096^2 P 50 window 128 sigma 3 (threshold %.2f, factors in [%.3f, %.3f]): median %.3f ms, "
                         "min %.3f ms (less the re-upload of the frame, median %.3f ms)"
                         % (name, info["threshold"], info["lowest"], info["highest"], med - up, mn - up, up))
        for n in BINS:
            ow, oh = nl.bin_shape(W, H, n)
            with nl.StackHandle(1, ow, oh) as dst:
                med, mn = median_ms(lambda: dst.frame_bin_from(0, st, 0, n), reps)
            lines.append("frame_bin_from     4096^2 n %d -> %dx%d: median %.3f ms, min %.3f ms" % (n, ow, oh, med, mn))
    return lines


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "deband_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per-dispatch min / median / max in us; share = algorithmic bytes / min / 8 TB/s",
             "(bin_kernel<2, true>, <0, false>, <4, true>: n = 2, 3, 4)"]
    for name, ns in sorted(dispatches(trace).items(), key=lambda kv: -np.median(kv[1])):
        if "deband_" not in name and "bin_kernel" not in name:
            continue
        med = float(np.median(ns))
        key = next((k for k in BYTES if k in name), None)
        share = ""
        if key:
            share = "  %4.0f MB  %3.0f %%" % (BYTES[key] / 1e6, 100.0 * BYTES[key] / (min(ns) * 1e-9) / HBM_PEAK)
        lines.append("%-48s %4d %9.1f %9.1f %9.1f%s" % (name[-48:], len(ns), min(ns) / 1e3, med / 1e3, max(ns) / 1e3,
                                                         share))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true", help="the calls only (the run under rocprofv3)")
    ap.add_argument("--out", required=True, help="directory for the summary and the rocprofv3 trace")
    a = ap.parse_args()
    if a.inner:
        run_calls(3)
        return
    os.makedirs(a.out, exist_ok=True)
    lines = run_calls(10) + [""] + kernel_stats(a.out)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "deband_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
