#!/usr/bin/env python3
"""Times of the drizzle integration on the device (drizzle.hip; include/nlstack_drizzle.h, an extension) beside the
nearest existing kernel, the Lanczos-3 resampling onto the same output grid.

  python tools/drizzle_probe.py [--out DIR]
      One MI355X, a 4096^2 source onto 8192^2 (scale 2), pixfrac 0.7, through a sub-pixel shift and a small rotation.
      Each row: wall time per call (median and minimum of 10 after 2 warm-up calls; a call ends in a stream sync, so
      this is kernel time plus launch and sync), with the staged and direct tile counts of the call.  The rows:
      frame_drizzle_from with the turbo and the point kernel, as the kernel chooses its tile path and with developer
      switch 32768 (no tile stages); frame_resample_from with Lanczos-3 through the same source -> output transform;
      drizzle_finalize; frame_reject_against on the source's grid.
      DIR (default: profiles/) receives the table as drizzle_probe.txt.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
S, PIXFRAC = 2.0, 0.7
OW, OH = 8192, 8192
REPS, WARM = 10, 2
TRANSFORMS = (("subpixel", [1, 0, 0.5, 0, 1, 0.25]), ("small_rot", [0.999, 0.03, -3.2, -0.03, 0.999, 4.7]))


def sky():
    rng = np.random.default_rng(5)
    return (1000.0 + 10.0 * rng.standard_normal(W * H, dtype=np.float32)).astype(np.float32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory for drizzle_probe.txt")
    a = ap.parse_args()
    import nightlight_amd as nl
    from nightlight_amd import capi
    lines = ["%dx%d -> %dx%d (scale %g, pixfrac %g), one device, ms per call: median and minimum of %d after %d warm-up "
             "calls (wall clock; a call ends in a stream sync)" % (W, H, OW, OH, S, PIXFRAC, REPS, WARM),
             "%-34s %-10s %2s %12s %12s %10s %10s" % ("call", "transform", "R", "median ms", "min ms", "staged", "direct")]
    row = "%-34s %-10s %2s %12.3f %12.3f %10s %10s"
    with nl.StackHandle(2, W, H) as src, nl.StackHandle(3, OW, OH) as dst:
        src.upload_frame(0, sky())
        src.upload_frame(1, sky())
        for tname, t in TRANSFORMS:
            F, _, _, R = nl.drizzle_geometry(t, S, PIXFRAC)
            for label, kernel in (("drizzle turbo", capi.DZ_TURBO), ("drizzle point", capi.DZ_POINT)):
                for how, flags in (("", 0), (", no tile stages", 32768)):
                    dst.set_dev_flags(flags)
                    staged, direct = dst.drizzle_tile_paths(src, 0, t, S, PIXFRAC)
                    med, mn = timed_ms(lambda: dst.frame_drizzle_from(0, 1, src, 0, t, S, PIXFRAC, 1.0, False, kernel))
                    lines.append(row % (label + how, tname, R, med, mn, staged, direct))
            dst.set_dev_flags(0)
            staged, direct = dst.resample_tile_paths(src, 0, F, capi.RS_LANCZOS3)
            med, mn = timed_ms(lambda: dst.frame_resample_from(2, src, 0, F, float("nan"), capi.RS_LANCZOS3, False))
            lines.append(row % ("resample Lanczos-3 (yardstick)", tname, "", med, mn, staged, direct))
        dst.frame_drizzle_from(0, 1, src, 0, TRANSFORMS[0][1], S, PIXFRAC, first=True)
        med, mn = timed_ms(lambda: dst.drizzle_finalize(0, 1, 2))
        lines.append(row % ("drizzle_finalize (8192^2)", "", "", med, mn, "", ""))
        med, mn = timed_ms(lambda: src.frame_reject_against(0, 1, 1e30, 1e30))
        lines.append(row % ("frame_reject_against (4096^2)", "", "", med, mn, "", ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "drizzle_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
