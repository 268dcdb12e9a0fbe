#!/usr/bin/env python3
"""Times of the tone curves and the gray export on the device (tone.hip: the per-pixel operators of the stretch command,
OpSave's quantisation).

  python tools/tone_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; every call ends in a stream sync, the ones with statistics
      also in a 48 KiB copy of the partials, the exports in the download of their counts -- so this is device time plus
      launch, copy and sync overhead) on a resident 4096^2 slot: every kind of nl_stack_frame_tone without and with the
      fused statistics, nl_stack_frame_export_gray at 16 and 8 bits without and with a gamma, and the one comparison
      there is: nl_stack_frame_affine followed by nl_stack_frame_stats against NL_TONE_SCALE_OFFSET with statistics.
      Then the calls run once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time limit)
      and every tone / export kernel's per-dispatch durations are printed with its rate against the 8 B / pixel a curve
      must move (6 or 5 for the exports) as a share of the MI355X's 8 TB/s HBM peak.  DIR receives the summary
      (tone_probe.txt) and the trace.  Recorded, not gated: there is no earlier device form of the curves.
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


def sky():
    return np.random.default_rng(5).random(N, dtype=np.float32)


def median_ms(fn, reps, warm=2):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def cases(nl, st):
    """(label, call): in place, so the frame drifts from call to call; the work per call does not depend on the values
    (the device's pow takes one path for every finite positive base)"""
    curves = (("scale_offset", nl.TONE_SCALE_OFFSET, (0.999, 0.0005)), ("normalize", nl.TONE_NORMALIZE, (0.0, 1.0)),
              ("gamma 2.2", nl.TONE_GAMMA, (2.2,)), ("partial_gamma", nl.TONE_PARTIAL_GAMMA, (0.1, 1.0, 1.5)),
              ("midtones", nl.TONE_MIDTONES, (0.25, 0.01)), ("shift_black", nl.TONE_SHIFT_BLACK, (0.3, 0.29)))
    out = []
    for label, kind, p in curves:
        out.append((label, lambda kind=kind, p=p: st.frame_tone(0, kind, *p)))
        out.append((label + " + stats", lambda kind=kind, p=p: st.frame_tone(0, kind, *p, stats=True)))
    out.append(("affine, then frame_stats", lambda: (st.frame_affine(0, 0.999, 0.0005), st.frame_stats(0, variance=False))))
    for bits in (16, 8):
        out.append(("export %d bits" % bits, lambda bits=bits: st.frame_export_gray(0, 0.0, 1.0, 1.0, bits)))
        out.append(("export %d bits, gamma 2.2" % bits, lambda bits=bits: st.frame_export_gray(0, 0.0, 1.0, 2.2, bits)))
    return out


def run_calls(reps):
    import nightlight_amd as nl
    lines = []
    with nl.StackHandle(1, W, H) as st:
        st.upload_frame(0, sky())
        for label, call in cases(nl, st):
            med, mn = median_ms(call, reps)
            lines.append("%-28s 4096^2: median %.3f ms, min %.3f ms per call" % (label, med, mn))
    return lines


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "tone_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per kernel dispatches, min / median / max in us; share = algorithmic bytes / min / 8 TB/s",
             "(tone_kernel<op, stats, vec>: op 0 affine, 1 gamma, 2 partial gamma, 3 midtones, 4 shift black; "
             "export_gray_kernel<bits, gamma, vec>; min_sum_max_kernel and affine_kernel: the parent's pair)"]
    for name, ns in sorted(dispatches(trace).items()):
        if not any(k in name for k in ("tone_kernel", "export_gray_kernel", "min_sum_max_kernel", "affine_kernel")):
            continue
        per_pixel = 6 if "export_gray_kernel<16" in name else 5 if "export_gray_kernel<8" in name else \
            4 if "min_sum_max" in name else 8
        lines.append("%-44s %3d %9.1f %9.1f %9.1f  %4.0f MB  %3.0f %%"
                     % (name[-44:], len(ns), min(ns) / 1e3, float(np.median(ns)) / 1e3, max(ns) / 1e3,
                        per_pixel * N / 1e6, 100.0 * per_pixel * N / (min(ns) * 1e-9) / HBM_PEAK))
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
    with open(os.path.join(a.out, "tone_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
