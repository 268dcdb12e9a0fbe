#!/usr/bin/env python3
"""Times of OpAlign's estimate on the device (align.hip: triangles, nearest reference triangle, star matching).

  python tools/align_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; a call ends in the host's shortlist and transforms between
      two stream syncs, so this is device time plus launch, copy, sync and host overhead) of nl_aligner_match at the
      operator's K = 50 with 2 000 stars on either side (19 600 triangles against 19 600), and of nl_aligner_create;
      then runs the calls once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time
      limit) and prints every kernel's per-dispatch durations.  DIR receives the summary (align_probe.txt) and the
      trace.  The reference's own time for these steps has not been measured (there is no Go toolchain to build it).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stars_probe import dispatches  # noqa: E402

W, H, K, N_STARS = 4096, 3072, 50, 2000


def median_ms(fn, reps, warm=2):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def run_calls(reps):
    import align_ref
    import nightlight_amd as nl
    from nightlight_amd import capi
    ref_x, ref_y, x, y, _ = align_ref.make_case(seed=1, n_ref=N_STARS, width=W, height=H, drop=0.1, add=0.1)
    x, y = x[:N_STARS], y[:N_STARS]

    def stars_of(x, y):
        s = np.zeros(len(x), capi.STAR_DTYPE)
        s["x"], s["y"] = x, y
        return s
    ref, frame = stars_of(ref_x, ref_y), stars_of(x, y)
    lines = []
    med, mn = median_ms(lambda: nl.Aligner(W, H, ref, k=K).close(), reps)
    lines.append("aligner_create + destroy  K %d, %d reference stars: median %.3f ms, min %.3f ms" % (K, len(ref), med, mn))
    with nl.Aligner(W, H, ref, k=K) as a:
        cands, ref_index, info = a.match(W, frame)
        med, mn = median_ms(lambda: a.match(W, frame), reps)
        lines.append("aligner_match             K %d, %d stars against %d: %d triangles against %d, %d candidates, %d with "
                     "enough matches, at most %d stars matched: median %.3f ms, min %.3f ms"
                     % (K, len(frame), len(ref), info["n_triangles"], len(a.info()[1]), len(cands),
                        int(cands["enough"].sum()), int(cands["num_matches"].max()), med, mn))
    return lines


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "align_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per-dispatch count, min / median / max in us"]
    for name, ns in sorted(dispatches(trace).items(), key=lambda kv: -np.median(kv[1])):
        if "align_" not in name:
            continue
        lines.append("%-48s %4d %9.1f %9.1f %9.1f" % (name[-48:], len(ns), min(ns) / 1e3, float(np.median(ns)) / 1e3,
                                                      max(ns) / 1e3))
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
    with open(os.path.join(a.out, "align_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
