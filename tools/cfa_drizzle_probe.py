#!/usr/bin/env python3
"""Times of the CFA drizzle on the device (drizzle_cfa.hip; include/nlstack_cfadrizzle.h, an extension) beside its
yardstick, the existing mono drizzle of the NaN-masked copy of the same mosaic, which gives the same planes.

  python tools/cfa_drizzle_probe.py [--out DIR]
      One MI355X, a 4096^2 RGGB mosaic onto 8192^2 (scale 2, pixfrac 0.7) and onto 4096^2 (scale 1, pixfrac 1), through
      a sub-pixel shift and a small rotation, turbo kernel.  tools/drizzle_probe.py's method: wall time per call, median,
      minimum and maximum of 10 after 2 warm-up calls in one process (a call ends in a stream sync, so this is kernel
      time plus launch and sync).  Per geometry, in the same run: frame_drizzle_cfa_from for a sparse channel (R) and for
      G -- the strided walk -- and frame_drizzle_from on the copy of the mosaic whose other pixels are NaN -- the full
      window.  Then frame_reject_against_cfa and frame_badpixel_cfa on the 4096^2 mosaic.
      DIR (default: profiles/) receives the table as cfa_drizzle_probe.txt.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
CFA = "RGGB"
REPS, WARM = 10, 2
GRIDS = ((2.0, 0.7, 8192), (1.0, 1.0, 4096))                  # scale, pixfrac, output side
TRANSFORMS = (("subpixel", [1, 0, 0.5, 0, 1, 0.25]), ("small_rot", [0.999, 0.03, -3.2, -0.03, 0.999, 4.7]))


def sky():
    rng = np.random.default_rng(5)
    return (1000.0 + 10.0 * rng.standard_normal((H, W), dtype=np.float32)).astype(np.float32)


def masked(raw, channel):
    """the RGGB mosaic with the other channels' pixels NaN"""
    keep = np.zeros((H, W), bool)
    if channel == "R":
        keep[0::2, 0::2] = True
    else:
        keep[0::2, 1::2] = True
        keep[1::2, 0::2] = True
    return np.where(keep, raw, np.float32(np.nan)).astype(np.float32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"), help="directory for cfa_drizzle_probe.txt")
    a = ap.parse_args()
    import nightlight_amd as nl
    lines = ["%dx%d %s mosaic, one device, turbo kernel, ms per call: median, minimum and maximum of %d after %d warm-up "
             "calls (wall clock; a call ends in a stream sync)" % (W, H, CFA, REPS, WARM),
             "%-44s %-10s %-14s %2s %10s %10s %10s" % ("call", "transform", "grid", "R", "median ms", "min ms", "max ms")]
    row = "%-44s %-10s %-14s %2s %10.3f %10.3f %10.3f"
    raw = sky()
    with nl.StackHandle(4, W, H) as src:
        src.upload_frame(0, raw.reshape(-1))
        src.upload_frame(1, masked(raw, "R").reshape(-1))
        src.upload_frame(2, masked(raw, "G").reshape(-1))
        src.upload_frame(3, raw.reshape(-1))
        for S, p, side in GRIDS:
            grid = "%dx%d p=%g" % (side, side, p)
            with nl.StackHandle(2, side, side) as dst:
                for tname, t in TRANSFORMS:
                    R = nl.drizzle_geometry(t, S, p)[3]
                    for channel, slot in (("R", 1), ("G", 2)):
                        res = timed_ms(lambda: dst.frame_drizzle_cfa_from(0, 1, src, 0, t, S, channel, CFA, pixfrac=p))
                        lines.append(row % (("drizzle_cfa_from %s (strided walk)" % channel, tname, grid, R) + res))
                        res = timed_ms(lambda: dst.frame_drizzle_from(0, 1, src, slot, t, S, p))
                        lines.append(row % (("drizzle_from, %s-masked copy (yardstick)" % channel, tname, grid, R) + res))
        for channel in ("R", "G"):
            res = timed_ms(lambda: src.frame_reject_against_cfa(0, 3, channel, CFA, 1e30, 1e30))
            lines.append(row % (("frame_reject_against_cfa %s" % channel, "", "4096x4096", "") + res))
            res = timed_ms(lambda: src.frame_badpixel_cfa(0, channel, CFA, 3.0, 5.0))
            lines.append(row % (("frame_badpixel_cfa %s" % channel, "", "4096x4096", "") + res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "cfa_drizzle_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
