#!/usr/bin/env python3
"""GPU times of the deep pass (include/nlstack_deepstack.h: the median and MAD sigma of 513 ... 2048 frames on 8 or 16
lanes per pixel) beside the pass of nl_stack_run, whose kernels beyond 512 frames this pass leaves as they are.

  python tools/deepstack_probe.py [--frames 512,1024,2048 --width 4096 --height 4096 --rows 512 --sigma 3 --reps 10 --out DIR --append]
      Per frame count, on ONE handle in one process -- a tile of --rows rows of the image, the C3 tile shape (8 GiB at 1024
      frames, 16 GiB at 2048): synthetic frames (nl_stack_fill_synthetic); per pass one warm-up run, then the median and
      minimum over --reps runs (fewer where a run takes seconds: about ten seconds of runs per pass, two at least), each
      from the HIP events the library records on the handle's stream (nl_stack_pass_times: whole pass, dominant kernel),
      results left on the device:
        run, median / MAD sigma            nl_stack_run: the yardstick (up to 512 frames the only pass)
        run_deepstack, median / MAD sigma  nl_stack_run_deepstack, with nl_stack_last_fallback_pixels
      and per mode the ratio, the time per sample, whether the median's bits and the MAD totals agree.
      DIR receives the lines as deepstack_probe.txt (--append: added to it, so that a caller can give every frame count a
      process and a time limit of its own).  profiles/deepstack_probe.txt was made so, every step under its own limit:
        timeout -k 10 120 python tools/deepstack_probe.py --frames 512 --out DIR && \
        timeout -k 10 300 python tools/deepstack_probe.py --frames 1024 --out DIR --append && \
        timeout -k 10 420 python tools/deepstack_probe.py --frames 2048 --out DIR --append
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="512,1024,2048")
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import nightlight_amd as nl
    from nightlight_amd import capi
    lines = []

    def emit(line):                      # (printed as it is measured: a pass on the column kernel takes seconds)
        lines.append(line)
        print(line, flush=True)

    if not a.append:
        try:
            import torch
            emit("device: %s" % torch.cuda.get_device_name(0))
        except Exception:
            pass
        emit("a tile of %d rows of %d x %d, sigma %.2f / %.2f; up to %d runs after one warm-up run"
             % (a.rows, a.width, a.height, a.sigma, a.sigma, a.reps))
    px = a.width * a.rows
    for frames in [int(x) for x in a.frames.split(",")]:
        with nl.StackHandle(frames, a.width, a.height, row0=0, rows=a.rows) as st:
            st.fill_synthetic(seed=7)
            emit("%d frames (%.1f GiB):" % (frames, frames * px * 4 / 2.0 ** 30))
            seen = {}
            for mode, mname in ((capi.ST_MEDIAN, "median"), (capi.ST_MAD_SIGMA, "MAD sigma")):
                for entry, ename in ((st.run, "run"), (st.run_deepstack, "run_deepstack")):
                    if ename == "run_deepstack" and frames <= 512:
                        continue
                    _, lo, hi = entry(mode, a.sigma, a.sigma, 0.0, fetch=False)                 # warm-up
                    first = st.pass_times(0)[0]
                    reps = max(2, min(a.reps, int(10000.0 / max(first, 1e-3))))
                    ms = []
                    for _ in range(reps):
                        _, lo, hi = entry(mode, a.sigma, a.sigma, 0.0, fetch=False)
                        ms.append(st.pass_times(0))
                    whole, dom = np.median([m[0] for m in ms]), np.median([m[1] for m in ms])
                    seen[(mname, ename)] = (float(whole), lo, hi, st.result_tile().view(np.uint32))
                    emit("  %-14s %-10s %-28s pass median %.3f ms, min %.3f ms; dominant kernel %.3f ms; %d runs; "
                         "%.2f ps per sample; handed over %d pixels"
                         % (ename, mname, st.last_kernel_name, whole, min(m[0] for m in ms), dom, reps,
                            1e9 * whole / (float(px) * frames), st.last_fallback_pixels))
                if (mname, "run_deepstack") in seen:
                    base, new = seen[(mname, "run")], seen[(mname, "run_deepstack")]
                    same = np.array_equal(base[3], new[3])
                    emit("  %s: run / run_deepstack = %.1f; totals equal: %s (%d / %d); result bits equal: %s%s"
                         % (mname, base[0] / new[0], base[1:3] == new[1:3], new[1], new[2], same,
                            "" if same or mode == capi.ST_MEDIAN else
                            " (another order of summation: %d of %d pixels differ)" % (int((base[3] != new[3]).sum()), px)))
    text = "\n".join(lines)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "deepstack_probe.txt"), "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
