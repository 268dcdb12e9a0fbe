#!/usr/bin/env python3
"""Times of the bicubic / Lanczos-3 resampling on the device (resample.hip; include/nlstack_resample.h, an extension)
beside the bilinear projection it extends.

  python tools/resample_probe.py [--out DIR]
      One MI355X, 4096^2 -> 4096^2 through the `subpixel` and `small_rot` transforms of
      tests/test_gpu_project_resident.py.  Each row: wall time per call (median and minimum of 20 after 3 warm-up
      calls; a call ends in a stream sync, so this is kernel time plus launch and sync), with the staged and direct
      tile counts of the call.  The rows: frame_project_from -- the yardstick, its code is what it was -- then
      frame_resample_from with the bicubic kernel, with Lanczos-3, and with Lanczos-3 and the clamp.
      DIR (default: profiles/) receives the table as resample_probe.txt.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
N = W * H
REPS, WARM = 20, 3
TRANSFORMS = (("subpixel", [1, 0, 0.5, 0, 1, 0.25]), ("small_rot", [0.999, 0.03, -3.2, -0.03, 0.999, 4.7]))


def sky():
    rng = np.random.default_rng(5)
    return (1000.0 + 10.0 * rng.standard_normal(N, dtype=np.float32)).astype(np.float32)


def timed_ms(fn):
    t = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        fn()
        if k >= WARM:
            t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory for resample_probe.txt")
    a = ap.parse_args()
    import nightlight_amd as nl
    from nightlight_amd import capi
    rows = (("frame_project_from", None, False), ("bicubic", capi.RS_BICUBIC, False),
            ("Lanczos-3", capi.RS_LANCZOS3, False), ("Lanczos-3, clamp", capi.RS_LANCZOS3, True))
    lines = ["%dx%d -> %dx%d, one device, ms per call: median and minimum of %d after %d warm-up calls (wall clock; "
             "a call ends in a stream sync)" % (W, H, W, H, REPS, WARM),
             "%-20s %-10s %12s %12s %10s %10s" % ("call", "transform", "median ms", "min ms", "staged", "direct")]
    with nl.StackHandle(1, W, H) as src, nl.StackHandle(1, W, H) as dst:
        src.upload_frame(0, sky())
        for tname, t in TRANSFORMS:
            for label, kernel, clamp in rows:
                if kernel is None:
                    staged, direct = dst.project_tile_paths(src, 0, t)
                    med, mn = timed_ms(lambda: dst.frame_project_from(0, src, 0, t))
                else:
                    staged, direct = dst.resample_tile_paths(src, 0, t, kernel)
                    med, mn = timed_ms(lambda: dst.frame_resample_from(0, src, 0, t, float("nan"), kernel, clamp))
                lines.append("%-20s %-10s %12.3f %12.3f %10d %10d" % (label, tname, med, mn, staged, direct))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "resample_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
