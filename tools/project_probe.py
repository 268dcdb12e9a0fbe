#!/usr/bin/env python3
"""Times of the projection on the device (project.hip: OpAlign's Project from a resident frame).

  python tools/project_probe.py --out DIR [--parent-tree DIR] [--chain]
      4096^2 -> 4096^2 through four transforms: a sub-pixel shift, a shift plus a 0.3 degree turn (what alignment
      produces), a quarter turn and a 0.5x scale (large source footprints).
      - wall time per nl_stack_frame_project_from call (median and minimum of 20 after 3 warm-up calls; the call ends
        in a stream sync, so this is kernel time plus launch and sync);
      - the kernel's own time per dispatch from `rocprofv3 --kernel-trace --stats` (a child process with its own time
        limit), for the default kernel, with no tile staged in LDS (developer switch 32768) and with plain result
        stores (65536), with the GB/s against 8 * W * H algorithmic bytes;
      - with --parent-tree: the same four transforms through nl_stack_upload_frame_projected of ANOTHER built checkout
        (the parent commit's: its project_kernel is the yardstick), kernel time only, the same way;
      - with --chain: 128 frames loaded into a stack handle two ways, projected from a staging slot, and downloaded
        from the staging slot and uploaded again with nl_stack_upload_frame_projected.
      DIR receives the summary (project_probe.txt) and the traces.
"""
import argparse
import csv
import glob
import math
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NL_PROBE_TREE") or ROOT)          # (the tree whose nightlight_amd is imported)

W = H = 4096
N = W * H
BYTES = 8 * N
REPS = 20
_c, _s = math.cos(math.radians(0.3)), math.sin(math.radians(0.3))
TRANSFORMS = (("sub-pixel shift", [1, 0, 0.5, 0, 1, 0.25]),
              ("shift + 0.3 degree turn", [_c, -_s, 17.3, _s, _c, -9.6]),
              ("quarter turn", [0, -1, W - 1, 1, 0, 0]),
              ("0.5x scale", [0.5, 0, 0, 0, 0.5, 0]))
VARIANTS = (("default", 0), ("no tile staged (32768)", 32768), ("plain stores (65536)", 65536))


def sky():
    rng = np.random.default_rng(5)
    return (1000.0 + 10.0 * rng.standard_normal(N, dtype=np.float32)).astype(np.float32)


def timed_ms(fn, reps=REPS, warm=3):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def run_resident(report):
    """every variant x transform, REPS + 3 calls each, in this order (the trace is read back by position)"""
    import nightlight_amd as nl
    lines = []
    with nl.StackHandle(1, W, H) as src, nl.StackHandle(1, W, H) as dst:
        src.upload_frame(0, sky())
        for vname, flags in VARIANTS:
            dst.set_dev_flags(flags)
            for tname, t in TRANSFORMS:
                staged, direct = dst.project_tile_paths(src, 0, t)
                med, mn = timed_ms(lambda: dst.frame_project_from(0, src, 0, t))
                lines.append("frame_project_from  %-24s %-24s tiles staged %5d direct %5d: median %.3f ms, min %.3f ms"
                             % (vname, tname, staged, direct, med, mn))
    return lines if report else []


def run_host_source():
    """the four transforms through upload_frame_projected (any build of the library), REPS + 3 calls each"""
    import nightlight_amd as nl
    data = sky()
    with nl.StackHandle(1, W, H) as st:
        for _, t in TRANSFORMS:
            for _ in range(REPS + 3):
                st.upload_frame_projected(0, data, W, H, t)


def run_chain(frames=128):
    import nightlight_amd as nl
    data = sky()
    t = TRANSFORMS[1][1]
    lines = []
    with nl.StackHandle(1, W, H) as staging, nl.StackHandle(frames, W, H) as st:
        staging.upload_frame(0, data)
        for name, load in (("project from the staging slot", lambda k: st.frame_project_from(k, staging, 0, t)),
                           ("download, then upload_frame_projected",
                            lambda k: st.upload_frame_projected(k, staging.download_tile(0), W, H, t))):
            for k in range(3):
                load(k)
            t0 = time.perf_counter()
            for k in range(frames):
                load(k)
            lines.append("loading %d x 4096^2 (%s): %.1f ms" % (frames, name, 1e3 * (time.perf_counter() - t0)))
    return lines


def ordered_dispatches(trace, key):
    """[duration ns] of the dispatches whose kernel name contains `key`, in start order"""
    dbs = glob.glob(os.path.join(trace, "**", "*.db"), recursive=True)
    if dbs:
        rows = list(sqlite3.connect(dbs[0]).execute("select name, start, end - start from kernels"))
    else:
        rows = []
        for path in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)[:1]:
            with open(path) as f:
                rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                        for r in csv.DictReader(f)]
    return [float(d) for name, _, d in sorted(rows, key=lambda r: r[1]) if key in name]


def traced(out_dir, tag, inner, key, groups, env=None):
    """runs `inner` under rocprofv3; per group of REPS + 3 dispatches of `key` the (median, min, max) us of the last REPS"""
    trace = os.path.join(out_dir, tag)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), inner, "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT, env=dict(os.environ, **(env or {})), stdout=subprocess.DEVNULL)
    if rc != 0:
        return None, "rocprofv3 run (%s) failed with status %d" % (tag, rc)
    ns = ordered_dispatches(trace, key)
    if len(ns) != groups * (REPS + 3):
        return None, "%s: %d dispatches of %s, expected %d" % (tag, len(ns), key, groups * (REPS + 3))
    out = []
    for g in range(groups):
        part = np.array(ns[g * (REPS + 3) + 3:(g + 1) * (REPS + 3)]) / 1e3
        out.append((float(np.median(part)), float(part.min()), float(part.max())))
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner-resident", action="store_true", help="the resident calls only (the run under rocprofv3)")
    ap.add_argument("--inner-host", action="store_true", help="the host-source calls only (the run under rocprofv3)")
    ap.add_argument("--parent-tree", help="a built checkout of another commit: its projection kernel is the yardstick")
    ap.add_argument("--chain", action="store_true", help="also time loading 128 frames both ways")
    ap.add_argument("--out", required=True, help="directory for the summary and the rocprofv3 traces")
    a = ap.parse_args()
    if a.inner_resident:
        run_resident(False)
        return
    if a.inner_host:
        run_host_source()
        return
    os.makedirs(a.out, exist_ok=True)
    lines = run_resident(True) + [""]
    new, err = traced(a.out, "project_rocprof", "--inner-resident", "project_tile_kernel", len(VARIANTS) * len(TRANSFORMS))
    parent = None
    if err:
        lines.append(err)
    if a.parent_tree:
        parent, perr = traced(a.out, "project_parent_rocprof", "--inner-host", "project_kernel", len(TRANSFORMS),
                              env={"NL_PROBE_TREE": os.path.abspath(a.parent_tree)})
        if perr:
            lines.append(perr)
    if new:
        lines.append("rocprofv3 --kernel-trace, per dispatch of project_tile_kernel: median / min / max us over %d; "
                     "GB/s = %d MB / median" % (REPS, BYTES // 1000000))
        for v, (vname, _) in enumerate(VARIANTS):
            for i, (tname, _) in enumerate(TRANSFORMS):
                med, mn, mx = new[v * len(TRANSFORMS) + i]
                text = "%-24s %-24s %7.1f %7.1f %7.1f  %5.0f GB/s" % (vname, tname, med, mn, mx, BYTES / med / 1e3)
                if parent:
                    text += "  parent median / this %.2f" % (parent[i][0] / med)
                lines.append(text)
    if parent:
        lines.append("the yardstick, project_kernel of %s (upload_frame_projected, kernel time only):" % a.parent_tree)
        for i, (tname, _) in enumerate(TRANSFORMS):
            med, mn, mx = parent[i]
            lines.append("%-24s %-24s %7.1f %7.1f %7.1f  %5.0f GB/s" % ("parent", tname, med, mn, mx, BYTES / med / 1e3))
    if a.chain:
        lines += [""] + run_chain()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "project_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
