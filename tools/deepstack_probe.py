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

  python tools/deepstack_probe.py --maps [--modes mad,sigma,winsor] ...
      The maps pass beyond 512 frames (include/nlstack_deepstackmaps.h), same protocol.  Per frame count and mode:
        run_maps_full       the column kernel: what every maps tier below this one runs there
        run_maps_deepstack  the new pass
        run_deepstack (MAD sigma) / run (sigma, winsorized)   the plain pass beside it, the MAPS kernel's twin
      and the two ratios, whether maps, totals and result bits agree.  The column pass runs in a block of its own, first.
  python tools/deepstack_probe.py --weighted ...
      The weighted MAD-sigma pass (include/nlstack_deepwmad.h): run_mad_weighted (the column kernel beyond 512 frames),
      run_mad_weighted_deepstack, and run_deepstack's unweighted MAD pass beside them; weights 1 / (1 + 3 s_k),
      s_k = (1237 k mod 4099) / 4098.
      Both append to DIR/deepstack_probe.txt with --append; the blocks of profiles/deepstack_probe.txt behind the first were
      made so, one process and one time limit per frame count.
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
    ap.add_argument("--maps", action="store_true")
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--modes", default="mad,sigma,winsor")
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

    def timed(st, call):
        """(median ms of the pass, of its dominant kernel, minimum, runs, what the last run returned)"""
        got = call()                                                                       # warm-up
        first = st.pass_times(0)[0]
        reps = max(2, min(a.reps, int(10000.0 / max(first, 1e-3))))
        ms = []
        for _ in range(reps):
            got = call()
            ms.append(st.pass_times(0))
        return float(np.median([m[0] for m in ms])), float(np.median([m[1] for m in ms])), min(m[0] for m in ms), reps, got

    def line(st, ename, mname, t, frames):
        emit("  %-26s %-10s %-44s pass median %.3f ms, min %.3f ms; dominant kernel %.3f ms; %d runs; %.2f ps per sample; "
             "handed over %d pixels" % (ename, mname, st.last_kernel_name, t[0], t[2], t[1], t[3],
                                        1e9 * t[0] / (float(px) * frames), st.last_fallback_pixels))

    if a.maps or a.weighted:
        modes = {"mad": (capi.ST_MAD_SIGMA, "MAD sigma"), "sigma": (capi.ST_SIGMA, "sigma"),
                 "winsor": (capi.ST_WINSOR_SIGMA, "winsorized")}
        for frames in [int(x) for x in a.frames.split(",")]:
            with nl.StackHandle(frames, a.width, a.height, row0=0, rows=a.rows) as st:
                st.fill_synthetic(seed=7)
                sig = (a.sigma, a.sigma, 0.0)
                if a.maps:
                    emit("%d frames (%.1f GiB), maps passes:" % (frames, frames * px * 4 / 2.0 ** 30))
                    for mode, mname in [modes[m] for m in a.modes.split(",")]:
                        col = timed(st, lambda: st.run_maps_full(mode, *sig))
                        line(st, "run_maps_full", mname, col, frames)
                        new = timed(st, lambda: st.run_maps_deepstack(mode, *sig))
                        line(st, "run_maps_deepstack", mname, new, frames)
                        plain_entry = st.run_deepstack if mode == capi.ST_MAD_SIGMA else st.run
                        twin = timed(st, lambda: plain_entry(mode, *sig))
                        line(st, "run_deepstack" if mode == capi.ST_MAD_SIGMA else "run", mname, twin, frames)
                        c, n, t = col[4], new[4], twin[4]
                        emit("  %s: run_maps_full / run_maps_deepstack = %.1f; run_maps_deepstack / its plain twin = %.3f; "
                             "maps equal: %s; totals equal: %s (%d / %d); result bits equal the column pass's: %s, the twin's: %s"
                             % (mname, col[0] / new[0], new[0] / twin[0],
                                np.array_equal(c[3], n[3]) and np.array_equal(c[4], n[4]), (c[1], c[2]) == (n[1], n[2]) == (t[1], t[2]),
                                n[1], n[2], np.array_equal(c[0].view(np.uint32), n[0].view(np.uint32)),
                                np.array_equal(t[0].view(np.uint32), n[0].view(np.uint32))))
                if a.weighted:
                    emit("%d frames (%.1f GiB), weighted MAD sigma:" % (frames, frames * px * 4 / 2.0 ** 30))
                    k = np.arange(frames, dtype=np.int64)
                    weights = (1.0 / (1.0 + 3.0 * ((1237 * k) % 4099) / 4098.0)).astype(np.float32)
                    st.set_weights(weights)
                    col = timed(st, lambda: st.run_mad_weighted(*sig))
                    line(st, "run_mad_weighted", "MAD sigma", col, frames)
                    new = timed(st, lambda: st.run_mad_weighted_deepstack(*sig))
                    line(st, "run_mad_weighted_deepstack", "MAD sigma", new, frames)
                    st.set_weights(None)
                    twin = timed(st, lambda: st.run_deepstack(capi.ST_MAD_SIGMA, *sig))
                    line(st, "run_deepstack", "MAD sigma", twin, frames)
                    c, n, t = col[4], new[4], twin[4]
                    emit("  weighted MAD sigma: run_mad_weighted / run_mad_weighted_deepstack = %.1f; run_mad_weighted_deepstack / "
                         "run_deepstack = %.3f; totals equal: %s (%d / %d); result bits equal run_mad_weighted's: %s"
                         % (col[0] / new[0], new[0] / twin[0], (c[1], c[2]) == (n[1], n[2]) == (t[1], t[2]), n[1], n[2],
                            np.array_equal(c[0].view(np.uint32), n[0].view(np.uint32))))
        frames_list = []
    else:
        frames_list = [int(x) for x in a.frames.split(",")]
    for frames in frames_list:
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
