#!/usr/bin/env python3
"""GPU times of the weighted linear-fit pass (include/nlstack_wlinfit.h, an extension) beside the passes it sits next to.

  python tools/wlinfit_probe.py [--frames 128,64,32 --width 4096 --height 4096 --sigma 2.75 --reps 20 --out DIR]
      Per frame count, on ONE handle in one process: synthetic frames (nl_stack_fill_synthetic), weights from
      nl_stack_weights_from_noise, median and minimum over --reps runs after 3 warm-up runs, each from the HIP events
      the library records on the handle's stream (nl_stack_pass_times), results left on the device:
        the default linear fit    nl_stack_run(NL_ST_LINEAR_FIT): unweighted, the yardstick (its code is the parent's)
        the weighted pass         nl_stack_run_linfit_weighted, with nl_stack_last_fallback_pixels
        ... under set_exact(1)    the same call on the column kernel alone
        the weighted mean pass    nl_stack_run(NL_ST_MEAN): what the second read of the frames costs at least
      DIR receives the lines as wlinfit_probe.txt.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return "median %.3f ms, min %.3f ms" % (float(np.median(ms)), float(np.min(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="128,64,32")
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=2.75)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nightlight_amd as nl
    from nightlight_amd import capi
    warm = 3
    lines = []
    try:
        import torch
        lines.append("device: %s" % torch.cuda.get_device_name(0))
    except Exception:
        pass
    lines.append("%d x %d, sigma %.2f / %.2f, weights from noise; %d runs after %d warm-up runs"
                 % (a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    for frames in [int(x) for x in a.frames.split(",")]:
        with nl.StackHandle(frames, a.width, a.height) as st:
            st.fill_synthetic(seed=7)
            st.weights_from_noise()
            handed = {}

            def default_fit():
                st.run(capi.ST_LINEAR_FIT, a.sigma, a.sigma, 0.0, fetch=False)
                return st.pass_times(0)[0]

            def weighted(label):
                def fn():
                    _, lo, hi = st.run_linfit_weighted(a.sigma, a.sigma, 0.0, fetch=False)
                    handed[label] = (st.last_fallback_pixels, lo, hi)
                    return st.pass_times(0)[0]
                return fn

            def mean_pass():
                st.run(capi.ST_MEAN, a.sigma, a.sigma, 0.0, fetch=False)
                return st.pass_times(0)[0]

            times = {}
            lines.append("%d frames:" % frames)
            for label, fn, exact in (("default linear fit", default_fit, 0), ("weighted pass", weighted("weighted pass"), 0),
                                     ("weighted, set_exact(1)", weighted("weighted, set_exact(1)"), 1),
                                     ("weighted mean pass", mean_pass, 0)):
                st.set_exact(exact)
                ms = [fn() for _ in range(warm + a.reps)][warm:]
                st.set_exact(0)
                times[label] = float(np.median(ms))
                lines.append("  %-23s %-40s %s" % (label, st.last_kernel_name, stats(ms)))
            px = a.width * a.height
            h, lo, hi = handed["weighted pass"]
            lines.append("  weighted / default = %.2f; set_exact(1) / weighted = %.2f; handed over %d of %d pixels (%.2f %%); "
                         "rejected %.1f of %d samples per pixel (the column kernel alone: the same totals: %s)"
                         % (times["weighted pass"] / times["default linear fit"],
                            times["weighted, set_exact(1)"] / times["weighted pass"], h, px, 100.0 * h / px,
                            (lo + hi) / px, frames, handed["weighted, set_exact(1)"][1:] == (lo, hi)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "wlinfit_probe.txt"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
