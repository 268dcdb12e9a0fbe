#!/usr/bin/env python3
"""Times of background extraction on the device (background.hip: OpBackExtract).

  python tools/background_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; every call ends in the host's grid steps and a stream
      sync, so this is device time plus launch, copy, sync and host overhead) of nl_stack_frame_back_extract on a
      4096^2 field with the star list nl_stack_frame_find_stars gives (~1 500 stars), for g = 32, 64, 128, 256;
      then runs the calls once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time
      limit) and prints every background kernel's per-dispatch durations, with the subtract kernel's share of the
      MI355X's 8 TB/s HBM peak.  DIR receives the summary (background_probe.txt) and the trace.
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

from stars_probe import dispatches, fields  # noqa: E402

W = H = 4096
N = W * H
HBM_PEAK = 8.0e12
BYTES = {"back_subtract_kernel": 8 * N}      # the frame, read once and written once
GRIDS = (32, 64, 128, 256)


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
    natural, _ = fields()
    lines = []
    with nl.StackHandle(1, W, H) as st:
        st.upload_frame(0, natural)
        stars, _, _ = st.frame_find_stars(0, np.float32(1000.0), np.float32(10.0), diff_std=12.5)
        for g in GRIDS:
            f = 4.0

            def call():
                st.upload_frame(0, natural)       # the step is in place: every call starts from the same frame
                return st.frame_back_extract(0, stars, g, hfr_factor=f)
            try:
                _, _, cells, info = call()
            except nl.NlError as e:               # the reference panics too (a cell the star discs cover)
                lines.append("resident form 4096^2 g %3d hfrFactor 4: rejected as the reference panics: %s" % (g, e))
                f = 1.0
                _, _, cells, info = call()
            up, _ = median_ms(lambda: st.upload_frame(0, natural), reps)
            med, mn = median_ms(call, reps)
            lines.append("resident form 4096^2 g %3d hfrFactor %g (%dx%d cells, %d stars): median %.3f ms, min %.3f ms "
                         "(less the re-upload of the frame, median %.3f ms)"
                         % (g, f, info["cells_x"], info["cells_y"], stars.size, med - up, mn - up, up))
    return lines


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "background_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per-dispatch min / median / max in us over all grids (back_fit_kernel<false>:",
             "the cells past the LDS budget, g 256 here); share = algorithmic bytes / min / 8 TB/s"]
    for name, ns in sorted(dispatches(trace).items(), key=lambda kv: -np.median(kv[1])):
        if "back_" not in name:
            continue
        med = float(np.median(ns))
        key = next((k for k in BYTES if k in name), None)
        share = ""
        if key:
            share = "  %4.0f MB  %3.0f %%" % (BYTES[key] / 1e6, 100.0 * BYTES[key] / (min(ns) * 1e-9) / HBM_PEAK)
        lines.append("%-44s %4d %9.1f %9.1f %9.1f%s" % (name[-44:], len(ns), min(ns) / 1e3, med / 1e3, max(ns) / 1e3,
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
    with open(os.path.join(a.out, "background_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
