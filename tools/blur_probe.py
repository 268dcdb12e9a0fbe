#!/usr/bin/env python3
"""Times of the Gaussian blur and the unsharp mask on the device (blur.hip: OpGaussianBlur, OpUnsharpMask).

  python tools/blur_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; every call uploads its taps and ends in a stream sync, so
      this is device time plus launch, copy and sync overhead) of nl_stack_frame_gaussian_blur at sigma 1.5 / 2 / 10
      (5, 9 and 45 taps) and of nl_stack_frame_unsharp_mask at sigma 1.5 on a resident 4096^2 slot; then runs the calls
      once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time limit) and prints every
      kernel's per-dispatch durations with its rate against the bytes it must move -- 8 B / pixel for the row pass and
      the column pass, 12 with the unsharp-mask epilogue -- as a share of the MI355X's 8 TB/s HBM peak.  DIR receives
      the summary (blur_probe.txt) and the trace.  Recorded, not gated: there is no earlier device form to compare.
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
# (label, sigma, unsharp mask?)
CASES = (("blur sigma 1.5", 1.5, False), ("blur sigma 2", 2.0, False), ("blur sigma 10", 10.0, False),
         ("usm sigma 1.5", 1.5, True))


def sky():
    rng = np.random.default_rng(5)
    return (0.2 + 0.02 * rng.standard_normal(N, dtype=np.float32)).astype(np.float32)


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
    lines = []
    with nl.StackHandle(1, W, H) as st:
        st.upload_frame(0, sky())
        for label, sigma, usm in CASES:
            # in place: the frame drifts from call to call, the work per call does not depend on the values
            call = (lambda: st.frame_unsharp_mask(0, sigma, 1.0, 0.0, 1.0, 0.2)) if usm else \
                   (lambda: st.frame_gaussian_blur(0, sigma))
            med, mn = median_ms(call, reps)
            lines.append("%-16s 4096^2, %2d taps: median %.3f ms, min %.3f ms per call"
                         % (label, nl.gaussian_kernel_1d(sigma).size, med, mn))
    return lines


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "blur_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: dispatches in call order, 5 per case (%s);" % ", ".join(c[0] for c in CASES),
             "per case min / median / max in us; share = algorithmic bytes / min / 8 TB/s",
             "(blur_row_kernel<staged, vec>, blur_col_kernel<staged, vec, usm>)"]
    for name, ns in sorted(dispatches(trace).items()):
        if "blur_" not in name:
            continue
        usm = "true>" in name.replace(" ", "")[-6:] and "blur_col" in name
        per_pixel = 12 if usm else 8
        # the blur cases share one instantiation: split its dispatches by case in call order
        n_cases = 1 if usm else len(CASES) - 1 if "blur_col" in name else len(CASES)
        per = len(ns) // n_cases
        for i in range(n_cases):
            part = ns[i * per:(i + 1) * per]
            if not part:
                continue
            label = CASES[-1][0] if usm else CASES[i][0]
            lines.append("%-44s %-15s %3d %9.1f %9.1f %9.1f  %4.0f MB  %3.0f %%"
                         % (name[-44:], label, len(part), min(part) / 1e3, float(np.median(part)) / 1e3,
                            max(part) / 1e3, per_pixel * N / 1e6, 100.0 * per_pixel * N / (min(part) * 1e-9) / HBM_PEAK))
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
    with open(os.path.join(a.out, "blur_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
