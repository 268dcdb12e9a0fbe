#!/usr/bin/env python3
"""GPU times of a maps pass and of the coverage map beside the passes they sit next to (include/nlstack_maps.h).

  python tools/maps_probe.py [--frames 128 --width 4096 --height 4096 --mode 2 --sigma 3 --reps 20 --out DIR]
      On ONE handle in one process, synthetic frames (nl_stack_fill_synthetic), median and minimum over --reps runs
      after 3 warm-up runs, each from the HIP events the library records on the handle's stream
      (nl_stack_pass_times; nl_stack_last_coverage_ms):
        the default pass          nl_stack_run, result left on the device
        the maps pass             nl_stack_run_maps, every host pointer NULL (the download of the maps is not timed)
        the mean pass             nl_stack_run(NL_ST_MEAN): reads the same bytes as the coverage kernel
        nl_stack_coverage         its kernels only (the call also downloads the map)
      DIR receives the lines as maps_probe.txt.

  python tools/maps_probe.py --fastmaps [--width 4096 --height 4096 --sigma 3 --reps 20 --out DIR]
      The fast maps pass (include/nlstack_fastmaps.h) beside the passes it sits next to.  On ONE handle of 128 frames,
      with 128 and then 24 of them active, sigma and winsorized clipping, the same statistics of:
        the default pass          nl_stack_run
        the plain default pass    nl_stack_run under developer switch 1 (memset before, reduction kernel after: the
                                  protocol class of the fast maps pass, and its yardstick)
        the fast maps pass        nl_stack_run_maps_fast, every host pointer NULL
        the column maps pass      nl_stack_run_maps, every host pointer NULL
      and the two hand-over list lengths of the fast maps pass.  DIR receives the lines as fastmaps_probe.txt.

  python tools/maps_probe.py --linfit [--linfit-frames 128,32,256 --width 4096 --height 4096 --sigma 3 --reps 20 --out DIR]
      The resident maps pass of the linear fit (include/nlstack_residentmaps.h) beside the passes it sits next to.  Per
      frame count ONE handle, and on it the same statistics -- whole pass and dominant kernel -- of:
        the default pass          nl_stack_run(NL_ST_LINEAR_FIT): plain protocol already, the yardstick
        the resident maps pass    nl_stack_run_maps_resident, every host pointer NULL
        the default pass again    the spread between two blocks of the same pass, to read the ratio against
        the column maps pass      nl_stack_run_maps, every host pointer NULL
      with the cascade's list lengths and the exact list's.  A frame count whose handle cannot be made (memory) is
      reported and skipped.  DIR receives the lines as linfitmaps_probe.txt.

  python tools/maps_probe.py --deep [--deep-workloads 512x4096x4096:2,256x4096x4096:2,512x4096x512:3 --sigma 3 --reps 20
                                     --column-reps 3 --out DIR]
      The deep maps pass (include/nlstack_deepmaps.h) beside the passes it sits next to.  Per workload
      FRAMESxWIDTHxHEIGHT:MODE (sigma or winsorized clipping of 129 ... 512 frames) ONE handle, and on it, INTERLEAVED --
      one run of each per repetition, so that a drift of the box meets all of them alike -- the same statistics, whole
      pass and dominant kernel, of:
        the default pass          nl_stack_run, twice, the second run timed (behind a plain-protocol pass a fused
                                  pass first clears both scratch sets: the second run is the pass in its steady state)
        the plain default pass    nl_stack_run under developer switch 1 (memset before, reduction kernel after: the
                                  protocol class of the deep maps pass; its dominant kernel is the plain twin)
        the deep maps pass        nl_stack_run_maps_deep, every host pointer NULL
        the column maps pass      nl_stack_run_maps, every host pointer NULL; in the first --column-reps repetitions only
      with the two hand-over list lengths of the deep maps pass.  A workload whose handle cannot be made (memory) is
      reported and skipped.  DIR receives the lines as deepmaps_probe.txt, workload by workload as they finish.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return "median %.3f ms, min %.3f ms" % (float(np.median(ms)), float(np.min(ms)))


def fastmaps(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm, n = 3, 128
    lines = []
    try:
        import torch
        lines.append("device: %s" % torch.cuda.get_device_name(0))
    except Exception:
        pass
    lines.append("%d frames of %d x %d resident, sigma %.2f / %.2f; %d runs after %d warm-up runs; GPU time of the whole pass"
                 % (n, a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    with nl.StackHandle(n, a.width, a.height) as st:
        st.fill_synthetic(seed=7)
        for active in (128, 24):
            st.set_active_frames(active)
            for mode in (capi.ST_SIGMA, capi.ST_WINSOR_SIGMA):
                def default_pass():
                    st.run(mode, a.sigma, a.sigma, 0.0, fetch=False)
                    return st.pass_times(0)

                def fast_maps_pass():
                    capi.check(L.nl_stack_run_maps_fast(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                    return st.pass_times(0)

                def column_maps_pass():
                    capi.check(L.nl_stack_run_maps(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                    return st.pass_times(0)

                lines.append("-- %d active frames, mode %d" % (active, mode))
                med, med_dom = {}, {}
                for label, fn, flags in (("default pass", default_pass, 0), ("plain default pass", default_pass, 1),
                                         ("fast maps pass", fast_maps_pass, 0), ("column maps pass", column_maps_pass, 0)):
                    st.set_dev_flags(flags)
                    both = [fn() for _ in range(warm + a.reps)][warm:]
                    st.set_dev_flags(0)
                    ms, dom = [t[0] for t in both], [t[1] for t in both]
                    med[label], med_dom[label] = float(np.median(ms)), float(np.median(dom))
                    tail = "; dominant kernel median %.3f ms" % med_dom[label]
                    if label == "fast maps pass":
                        tail += "; exact list %d, generic list %d" % (st.last_fallback_pixels, st.last_generic_pixels)
                    lines.append("%-19s %-68s %s; protocol %d%s" % (label, st.last_kernel_name, stats(ms), st.last_pass_protocol, tail))
                lines.append("fast maps / plain default = %.3f (one more 4-byte store per %d bytes read: %.4f); "
                             "fast maps / default = %.3f; column maps / fast maps = %.1f"
                             % (med["fast maps pass"] / med["plain default pass"], 4 * active, 1.0 + 1.0 / active,
                                med["fast maps pass"] / med["default pass"], med["column maps pass"] / med["fast maps pass"]))
                lines.append("dominant kernels, fast maps / plain default = %.3f; behind the dominant kernel: %.3f ms against %.3f ms"
                             % (med_dom["fast maps pass"] / med_dom["plain default pass"],
                                med["fast maps pass"] - med_dom["fast maps pass"],
                                med["plain default pass"] - med_dom["plain default pass"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "fastmaps_probe.txt"), "w") as f:
            f.write(text + "\n")


def linfit(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm, mode = 3, capi.ST_LINEAR_FIT
    lines = []
    try:
        import torch
        lines.append("device: %s" % torch.cuda.get_device_name(0))
    except Exception:
        pass
    lines.append("linear fit, frames of %d x %d resident, sigma %.2f / %.2f; %d runs after %d warm-up runs; GPU time of the whole pass"
                 % (a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    for n in [int(x) for x in a.linfit_frames.split(",")]:
        lines.append("-- %d frames" % n)
        try:
            st = nl.StackHandle(n, a.width, a.height)
        except capi.NlError as e:
            lines.append("no handle of %d frames: %s" % (n, e))
            continue
        with st:
            st.fill_synthetic(seed=7)

            def default_pass():
                st.run(mode, a.sigma, a.sigma, 0.0, fetch=False)
                return st.pass_times(0)

            def resident_maps_pass():
                capi.check(L.nl_stack_run_maps_resident(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                return st.pass_times(0)

            def column_maps_pass():
                capi.check(L.nl_stack_run_maps(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                return st.pass_times(0)

            med, med_dom = {}, {}
            for label, fn in (("default pass", default_pass), ("resident maps pass", resident_maps_pass),
                              ("default pass again", default_pass), ("column maps pass", column_maps_pass)):
                both = [fn() for _ in range(warm + a.reps)][warm:]
                ms, dom = [t[0] for t in both], [t[1] for t in both]
                med[label], med_dom[label] = float(np.median(ms)), float(np.median(dom))
                tail = "; dominant kernel median %.3f ms, min %.3f ms" % (med_dom[label], float(np.min(dom)))
                if label != "column maps pass":
                    tail += "; exact list %d, stages %r" % (st.last_fallback_pixels, st.linfit_stage_counts[:3])
                lines.append("%-19s %-44s %s; protocol %d%s" % (label, st.last_kernel_name, stats(ms), st.last_pass_protocol, tail))
            base = 0.5 * (med["default pass"] + med["default pass again"])
            lines.append("resident maps / default = %.4f (one more 4-byte store per %d bytes read: %.4f; default again / default = %.4f); "
                         "column maps / resident maps = %.1f"
                         % (med["resident maps pass"] / base, 4 * n, 1.0 + 1.0 / n, med["default pass again"] / med["default pass"],
                            med["column maps pass"] / med["resident maps pass"]))
            lines.append("dominant kernels, resident maps / default = %.4f; behind the dominant kernel: %.3f ms against %.3f ms"
                         % (med_dom["resident maps pass"] / (0.5 * (med_dom["default pass"] + med_dom["default pass again"])),
                            med["resident maps pass"] - med_dom["resident maps pass"], med["default pass"] - med_dom["default pass"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "linfitmaps_probe.txt"), "w") as f:
            f.write(text + "\n")


def deep(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm = 3
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "deepmaps_probe.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")

    try:
        import torch
        emit("device: %s" % torch.cuda.get_device_name(0))
    except Exception:
        pass
    emit("sigma %.2f / %.2f, frames resident; per workload %d interleaved repetitions after %d warm-up runs (column maps pass: "
         "%d after 1); GPU time of the whole pass" % (a.sigma, a.sigma, a.reps, warm, a.column_reps))
    for spec in a.deep_workloads.split(","):
        shape, mode = spec.split(":")
        n, width, height = (int(x) for x in shape.split("x"))
        mode = int(mode)
        emit("-- %d frames of %d x %d, mode %d" % (n, width, height, mode))
        try:
            st = nl.StackHandle(n, width, height)
        except capi.NlError as e:
            emit("no handle of %d frames: %s" % (n, e))
            continue
        with st:
            st.fill_synthetic(seed=7)

            def default_pass():
                st.run(mode, a.sigma, a.sigma, 0.0, fetch=False)
                return st.pass_times(0)

            def steady_default_pass():
                # (twice, the second one timed: behind a plain-protocol pass a fused pass first clears both scratch sets)
                default_pass()
                return default_pass()

            def plain_default_pass():
                st.set_dev_flags(1)
                try:
                    return default_pass()
                finally:
                    st.set_dev_flags(0)

            def deep_maps_pass():
                capi.check(L.nl_stack_run_maps_deep(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                return st.pass_times(0)

            def column_maps_pass():
                capi.check(L.nl_stack_run_maps(st._h, mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
                return st.pass_times(0)

            passes = (("default pass", steady_default_pass),("plain default pass", plain_default_pass),
                      ("deep maps pass", deep_maps_pass), ("column maps pass", column_maps_pass))
            times = {label: [] for label, _ in passes}
            facts = {}
            for r in range(-warm, a.reps):
                for label, fn in passes:
                    if label == "column maps pass" and not -1 <= r < a.column_reps:
                        continue
                    t = fn()
                    if r >= 0:
                        times[label].append(t)
                    tail = "; protocol %d" % st.last_pass_protocol
                    if label == "deep maps pass":
                        tail += "; exact list %d, generic list %d" % (st.last_fallback_pixels, st.last_generic_pixels)
                    facts[label] = (st.last_kernel_name, tail)
            med, med_dom = {}, {}
            for label, _ in passes:
                ms, dom = [t[0] for t in times[label]], [t[1] for t in times[label]]
                med[label], med_dom[label] = float(np.median(ms)), float(np.median(dom))
                emit("%-19s %-50s %s (%d runs)%s; dominant kernel median %.3f ms, min %.3f ms"
                     % (label, facts[label][0], stats(ms), len(ms), facts[label][1], med_dom[label], float(np.min(dom))))
            emit("deep maps / default = %.3f; deep maps / plain default = %.3f (one more 4-byte store per %d bytes read: %.4f); "
                 "column maps / deep maps = %.1f"
                 % (med["deep maps pass"] / med["default pass"], med["deep maps pass"] / med["plain default pass"], 4 * n,
                    1.0 + 1.0 / n, med["column maps pass"] / med["deep maps pass"]))
            emit("dominant kernels, deep maps / plain default = %.4f, deep maps / default = %.4f; behind the dominant kernel: "
                 "%.3f ms (deep maps), %.3f ms (plain default), %.3f ms (default)"
                 % (med_dom["deep maps pass"] / med_dom["plain default pass"], med_dom["deep maps pass"] / med_dom["default pass"],
                    med["deep maps pass"] - med_dom["deep maps pass"], med["plain default pass"] - med_dom["plain default pass"],
                    med["default pass"] - med_dom["default pass"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fastmaps", action="store_true")
    ap.add_argument("--linfit", action="store_true")
    ap.add_argument("--linfit-frames", default="128,32,256")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--deep-workloads", default="512x4096x4096:2,256x4096x4096:2,512x4096x512:3")
    ap.add_argument("--column-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.fastmaps:
        return fastmaps(a)
    if a.linfit:
        return linfit(a)
    if a.deep:
        return deep(a)
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm = 3
    lines = []
    try:
        import torch
        lines.append("device: %s" % torch.cuda.get_device_name(0))
    except Exception:
        pass
    lines.append("%d frames of %d x %d, mode %d, sigma %.2f / %.2f; %d runs after %d warm-up runs"
                 % (a.frames, a.width, a.height, a.mode, a.sigma, a.sigma, a.reps, warm))
    with nl.StackHandle(a.frames, a.width, a.height) as st:
        st.fill_synthetic(seed=7)
        cov = np.zeros(a.width * a.height, np.uint16)

        def default_pass():
            st.run(a.mode, a.sigma, a.sigma, 0.0, fetch=False)
            return st.pass_times(0)[0]

        def maps_pass():
            capi.check(L.nl_stack_run_maps(st._h, a.mode, a.sigma, a.sigma, 0.0, None, None, None, None, None))
            return st.pass_times(0)[0]

        def mean_pass():
            st.run(capi.ST_MEAN, a.sigma, a.sigma, 0.0, fetch=False)
            return st.pass_times(0)[0]

        def coverage():
            st.coverage(out=cov)
            return st.last_coverage_ms

        times = {}
        for label, fn in (("default pass", default_pass), ("maps pass", maps_pass), ("mean pass", mean_pass),
                          ("coverage", coverage)):
            ms = [fn() for _ in range(warm + a.reps)][warm:]
            times[label] = float(np.median(ms))
            kernel = "stack_coverage_kernel" if label == "coverage" else st.last_kernel_name
            lines.append("%-13s %-42s %s" % (label, kernel, stats(ms)))
        read = 4.0 * a.frames * a.width * a.height
        lines.append("coverage / mean pass = %.3f; coverage reads %.2f GB: %.2f TB/s; maps pass / default pass = %.1f"
                     % (times["coverage"] / times["mean pass"], read / 1e9, read / times["coverage"] / 1e9,
                        times["maps pass"] / times["default pass"]))
        lines.append("coverage: %d ... %d frames per pixel" % (int(cov.min()), int(cov.max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "maps_probe.txt"), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
