#!/usr/bin/env python3
"""Times of the square drizzle on the device (drizzle_square.hip; include/nlstack_sqdrizzle.h, an extension) beside the
turbo drizzle of the same call, which exists at the parent commit.

  python tools/sqdrizzle_probe.py [--out DIR]
      One MI355X, a 4096^2 source onto 8192^2 (scale 2), pixfrac 0.7, through a sub-pixel shift and a small rotation.
      tools/drizzle_probe.py's method: wall time per call, median, minimum and maximum of 10 after 2 warm-up calls, one
      process; a call ends in a stream sync, so this is kernel time plus launch and sync.  The rows: frame_drizzle_from
      with the turbo kernel (the yardstick); frame_drizzle_square_from in both candidate forms -- the edges of a
      candidate skipped where no lane of the wave takes it, and, with developer switch 262144, the edges of every
      candidate -- and with developer switch 32768 (no tile stages); the CFA entries for R and G of an RGGB mosaic,
      turbo and square.  Nothing is gated on the ratios: the square kernel computes more by definition.
      DIR (default: profiles/) receives the table as sqdrizzle_probe.txt.
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
EVERY, DIRECT = 262144, 32768
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
    return 1e3 * float(np.median(t)), 1e3 * float(np.min(t)), 1e3 * float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory for sqdrizzle_probe.txt")
    a = ap.parse_args()
    import nightlight_amd as nl
    lines = ["%dx%d -> %dx%d (scale %g, pixfrac %g), one device, ms per call: median, minimum and maximum of %d after %d "
             "warm-up calls (wall clock; a call ends in a stream sync)" % (W, H, OW, OH, S, PIXFRAC, REPS, WARM),
             "%-52s %-10s %2s %10s %10s %10s %8s %8s" % ("call", "transform", "R", "median ms", "min ms", "max ms", "staged",
                                                         "direct")]
    row = "%-52s %-10s %2d %10.3f %10.3f %10.3f %8d %8d"
    with nl.StackHandle(1, W, H) as src, nl.StackHandle(2, OW, OH) as dst:
        src.upload_frame(0, sky())
        for tname, t in TRANSFORMS:
            dst.set_dev_flags(0)
            R = nl.drizzle_geometry(t, S, PIXFRAC)[3]
            paths = dst.drizzle_tile_paths(src, 0, t, S, PIXFRAC)
            res = timed_ms(lambda: dst.frame_drizzle_from(0, 1, src, 0, t, S, PIXFRAC))
            lines.append(row % (("drizzle_from turbo (yardstick)", tname, R) + res + paths))
            R = nl.drizzle_square_geometry(t, S, PIXFRAC)[4]
            for how, flags in (("skips wave by wave", 0), ("every candidate", EVERY), ("skips, no tile stages", DIRECT),
                               ("every candidate, no tile stages", EVERY | DIRECT)):
                dst.set_dev_flags(flags)
                paths = dst.drizzle_square_tile_paths(src, 0, t, S, PIXFRAC)
                res = timed_ms(lambda: dst.frame_drizzle_square_from(0, 1, src, 0, t, S, PIXFRAC))
                lines.append(row % (("drizzle_square_from, " + how, tname, R) + res + paths))
            for channel in ("R", "G"):
                dst.set_dev_flags(0)
                paths = dst.drizzle_tile_paths(src, 0, t, S, PIXFRAC)
                res = timed_ms(lambda: dst.frame_drizzle_cfa_from(0, 1, src, 0, t, S, channel, "RGGB", pixfrac=PIXFRAC))
                lines.append(row % (("drizzle_cfa_from %s turbo (yardstick)" % channel, tname,
                                     nl.drizzle_geometry(t, S, PIXFRAC)[3]) + res + paths))
                for how, flags in (("skips wave by wave", 0), ("every candidate", EVERY)):
                    dst.set_dev_flags(flags)
                    paths = dst.drizzle_square_tile_paths(src, 0, t, S, PIXFRAC)
                    res = timed_ms(lambda: dst.frame_drizzle_square_cfa_from(0, 1, src, 0, t, S, channel, "RGGB",
                                                                             pixfrac=PIXFRAC))
                    lines.append(row % (("drizzle_square_cfa_from %s, %s" % (channel, how), tname, R) + res + paths))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "sqdrizzle_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
