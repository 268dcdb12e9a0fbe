#!/usr/bin/env python3
"""GPU times of the weighted MAD-sigma pass whose weights follow their frames (include/nlstack_wmad.h, an extension)
beside the passes it sits next to.

  python tools/wmad_probe.py [--frames 24,64,128,256,512 --width 4096 --height 4096 --sigma 3 --reps 20 --out DIR --append]
      Per frame count, on ONE handle in one process: synthetic frames (nl_stack_fill_synthetic), weights from
      nl_stack_weights_from_noise, median and minimum over --reps runs after 3 warm-up runs, each from the HIP events the
      library records on the handle's stream (nl_stack_pass_times), results left on the device:
        the unweighted MAD pass   nl_stack_run(NL_ST_MAD_SIGMA) without weights: the yardstick (its code is the parent's)
        the weighted mean pass    nl_stack_run(NL_ST_MEAN) with weights: one streaming read of the frames
        the new pass              nl_stack_run_mad_weighted, with nl_stack_last_fallback_pixels
        ... under set_exact(1)    the same call on the column kernel alone
      DIR receives the lines as wmad_probe.txt (--append: added to it, so that a caller can give every frame count a
      process and a time limit of its own).  profiles/wmad_probe.txt was made so, every step under its own limit:
        timeout -k 10 200 python tools/wmad_probe.py --frames 24 --out DIR && \
        timeout -k 10 200 python tools/wmad_probe.py --frames 64 --out DIR --append && ... (128, 256, 512)
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
    ap.add_argument("--frames", default="24,64,128,256,512")
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import nightlight_amd as nl
    from nightlight_amd import capi
    warm = 3
    lines = []
    if not a.append:
        try:
            import torch
            lines.append("device: %s" % torch.cuda.get_device_name(0))
        except Exception:
            pass
        lines.append("%d x %d, sigma %.2f / %.2f, weights from noise; %d runs after %d warm-up runs"
                     % (a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    px = a.width * a.height
    for frames in [int(x) for x in a.frames.split(",")]:
        with nl.StackHandle(frames, a.width, a.height) as st:
            st.fill_synthetic(seed=7)
            weights = nl.weights_from_scalars(nl.WEIGHT_INVERSE_NOISE, st.weights_from_noise())
            seen = {}

            def default(m, w, label):
                def fn():
                    st.set_weights(w)
                    _, lo, hi = st.run(m, a.sigma, a.sigma, 0.0, fetch=False)
                    seen[label] = (st.last_fallback_pixels, lo, hi)
                    return st.pass_times(0)[0]
                return fn

            def new_pass(label):
                def fn():
                    st.set_weights(weights)
                    _, lo, hi = st.run_mad_weighted(a.sigma, a.sigma, 0.0, fetch=False)
                    seen[label] = (st.last_fallback_pixels, lo, hi)
                    return st.pass_times(0)[0]
                return fn

            times = {}
            lines.append("%d frames:" % frames)
            for label, fn, exact in (("unweighted MAD pass", default(capi.ST_MAD_SIGMA, None, "unweighted"), 0),
                                     ("weighted mean pass", default(capi.ST_MEAN, weights, "mean"), 0),
                                     ("new pass", new_pass("new"), 0),
                                     ("new pass, set_exact(1)", new_pass("exact"), 1)):
                st.set_exact(exact)
                ms = [fn() for _ in range(warm + a.reps)][warm:]
                st.set_exact(0)
                times[label] = float(np.median(ms))
                lines.append("  %-23s %-44s %s" % (label, st.last_kernel_name, stats(ms)))
            h, lo, hi = seen["new"]
            lines.append("  new / unweighted MAD = %.3f; new / (unweighted MAD + mean) = %.2f; set_exact(1) / new = %.1f; handed "
                         "over %d of %d pixels (%.4f %%); rejected %.2f of %d samples per pixel; totals equal the unweighted "
                         "pass's: %s, the column kernel's: %s"
                         % (times["new pass"] / times["unweighted MAD pass"],
                            times["new pass"] / (times["unweighted MAD pass"] + times["weighted mean pass"]),
                            times["new pass, set_exact(1)"] / times["new pass"], h, px, 100.0 * h / px, (lo + hi) / px,
                            frames, seen["unweighted"][1:] == (lo, hi), seen["exact"][1:] == (lo, hi)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "wmad_probe.txt"), "a" if a.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
