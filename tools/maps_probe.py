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

  python tools/maps_probe.py --mad [--mad-frames 32,128,256,512 --width 4096 --height 4096 --sigma 3 --mad-reps 10
                                    --median-frames 128 --out DIR]
      The full maps pass (include/nlstack_fullmaps.h) beside the passes it sits next to.  Per depth ONE handle, and on it
      3 warm-up runs and the median of --mad-reps, whole pass and dominant kernel, of MAD sigma through (the first two
      interleaved, the third in a block of its own behind them):
        the default pass          nl_stack_run (plain protocol already: its own yardstick)
        the full maps pass        nl_stack_run_maps_full, every host pointer NULL
        the column maps pass      nl_stack_run_maps, every host pointer NULL
      and, at --median-frames, the same three for the median.  DIR (default: profiles/) receives the lines as
      maps_probe_mad.txt, depth by depth as they finish.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return "median %.3f ms, min %.3f ms" % (float(np.median(ms)), float(np.min(ms)))


class Report:
    """the lines of one mode: printed as they come, and DIR/name rewritten with all of them so far"""

    def __init__(self, out, name):
        self.lines, self.out, self.name = [], out, name
        try:
            import torch
            self("device: %s" % torch.cuda.get_device_name(0))
        except Exception:
            pass

    def __call__(self, line):
        print(line, flush=True)
        self.lines.append(line)
        if self.out:
            os.makedirs(self.out, exist_ok=True)
            with open(os.path.join(self.out, self.name), "w") as f:
                f.write("\n".join(self.lines) + "\n")


class Timing:
    """the runs of one pass: whole-pass and dominant-kernel times, and what the handle said after the last of them"""

    def __init__(self):
        self.ms, self.dom = [], []
        self.kernel, self.protocol, self.exact_list, self.generic_list = "", 0, 0, 0

    med = property(lambda self: float(np.median(self.ms)))
    med_dom = property(lambda self: float(np.median(self.dom)))
    min_dom = property(lambda self: float(np.min(self.dom)))


def measure(st, passes, warm, reps, interleaved=False, fewer=None):
    """passes: (label, fn) or (label, fn, developer flags); fn() runs one pass and returns (whole pass ms, dominant kernel
    ms).  Block by block -- warm + reps runs of one pass, then the next -- or interleaved: one run of each per repetition.
    fewer: {label: (warm-up runs, runs)} of the passes that run less often.  Returns {label: Timing}."""
    passes = [(p + (0,))[:3] for p in passes]
    result = {label: Timing() for label, _, _ in passes}

    def run(label, fn, flags, keep):
        st.set_dev_flags(flags)
        try:
            t = fn()
        finally:
            st.set_dev_flags(0)
        r = result[label]
        if keep:
            r.ms.append(t[0])
            r.dom.append(t[1])
        r.kernel, r.protocol = st.last_kernel_name, st.last_pass_protocol
        r.exact_list, r.generic_list = st.last_fallback_pixels, st.last_generic_pixels

    def wanted(label, i):
        w, n = (fewer or {}).get(label, (warm, reps))
        return -w <= i < n

    if interleaved:
        for i in range(-warm, reps):
            for label, fn, flags in passes:
                if wanted(label, i):
                    run(label, fn, flags, i >= 0)
    else:
        for label, fn, flags in passes:
            for i in range(-warm, reps):
                if wanted(label, i):
                    run(label, fn, flags, i >= 0)
    return result


def pass_fns(st, L, mode, sigma):
    """(default pass, maps pass of an entry) on the handle: the result stays on the device, every host pointer NULL"""
    from nightlight_amd import capi

    def default_pass():
        st.run(mode, sigma, sigma, 0.0, fetch=False)
        return st.pass_times(0)

    def maps_pass(entry):
        def fn():
            capi.check(getattr(L, entry)(st._h, mode, sigma, sigma, 0.0, None, None, None, None, None))
            return st.pass_times(0)
        return fn

    return default_pass, maps_pass


def fastmaps(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm, n = 3, 128
    emit = Report(a.out, "fastmaps_probe.txt")
    emit("%d frames of %d x %d resident, sigma %.2f / %.2f; %d runs after %d warm-up runs; GPU time of the whole pass"
         % (n, a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    with nl.StackHandle(n, a.width, a.height) as st:
        st.fill_synthetic(seed=7)
        for active in (128, 24):
            st.set_active_frames(active)
            for mode in (capi.ST_SIGMA, capi.ST_WINSOR_SIGMA):
                default_pass, maps_pass = pass_fns(st, L, mode, a.sigma)
                emit("-- %d active frames, mode %d" % (active, mode))
                t = measure(st, (("default pass", default_pass), ("plain default pass", default_pass, 1),
                                 ("fast maps pass", maps_pass("nl_stack_run_maps_fast")),
                                 ("column maps pass", maps_pass("nl_stack_run_maps"))), warm, a.reps)
                for label, r in t.items():
                    tail = "; dominant kernel median %.3f ms" % r.med_dom
                    if label == "fast maps pass":
                        tail += "; exact list %d, generic list %d" % (r.exact_list, r.generic_list)
                    emit("%-19s %-68s %s; protocol %d%s" % (label, r.kernel, stats(r.ms), r.protocol, tail))
                fast, plain = t["fast maps pass"], t["plain default pass"]
                emit("fast maps / plain default = %.3f (one more 4-byte store per %d bytes read: %.4f); "
                     "fast maps / default = %.3f; column maps / fast maps = %.1f"
                     % (fast.med / plain.med, 4 * active, 1.0 + 1.0 / active, fast.med / t["default pass"].med,
                        t["column maps pass"].med / fast.med))
                emit("dominant kernels, fast maps / plain default = %.3f; behind the dominant kernel: %.3f ms against %.3f ms"
                     % (fast.med_dom / plain.med_dom, fast.med - fast.med_dom, plain.med - plain.med_dom))


def linfit(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm, mode = 3, capi.ST_LINEAR_FIT
    emit = Report(a.out, "linfitmaps_probe.txt")
    emit("linear fit, frames of %d x %d resident, sigma %.2f / %.2f; %d runs after %d warm-up runs; GPU time of the whole pass"
         % (a.width, a.height, a.sigma, a.sigma, a.reps, warm))
    for n in [int(x) for x in a.linfit_frames.split(",")]:
        emit("-- %d frames" % n)
        try:
            st = nl.StackHandle(n, a.width, a.height)
        except capi.NlError as e:
            emit("no handle of %d frames: %s" % (n, e))
            continue
        with st:
            st.fill_synthetic(seed=7)
            default_pass, maps_pass = pass_fns(st, L, mode, a.sigma)
            # (block by block, one at a time: the stage lengths are read behind each block)
            t = {}
            for label, fn in (("default pass", default_pass), ("resident maps pass", maps_pass("nl_stack_run_maps_resident")),
                              ("default pass again", default_pass), ("column maps pass", maps_pass("nl_stack_run_maps"))):
                r = t[label] = measure(st, ((label, fn),), warm, a.reps)[label]
                tail = "; dominant kernel median %.3f ms, min %.3f ms" % (r.med_dom, r.min_dom)
                if label != "column maps pass":
                    tail += "; exact list %d, stages %r" % (r.exact_list, st.linfit_stage_counts[:3])
                emit("%-19s %-44s %s; protocol %d%s" % (label, r.kernel, stats(r.ms), r.protocol, tail))
            first, again, res = t["default pass"], t["default pass again"], t["resident maps pass"]
            emit("resident maps / default = %.4f (one more 4-byte store per %d bytes read: %.4f; default again / default = %.4f); "
                 "column maps / resident maps = %.1f"
                 % (res.med / (0.5 * (first.med + again.med)), 4 * n, 1.0 + 1.0 / n, again.med / first.med,
                    t["column maps pass"].med / res.med))
            emit("dominant kernels, resident maps / default = %.4f; behind the dominant kernel: %.3f ms against %.3f ms"
                 % (res.med_dom / (0.5 * (first.med_dom + again.med_dom)), res.med - res.med_dom, first.med - first.med_dom))


def deep(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm = 3
    emit = Report(a.out, "deepmaps_probe.txt")
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
            default_pass, maps_pass = pass_fns(st, L, mode, a.sigma)

            def steady_default_pass():
                # (twice, the second one timed: behind a plain-protocol pass a fused pass first clears both scratch sets)
                default_pass()
                return default_pass()

            t = measure(st, (("default pass", steady_default_pass), ("plain default pass", default_pass, 1),
                             ("deep maps pass", maps_pass("nl_stack_run_maps_deep")),
                             ("column maps pass", maps_pass("nl_stack_run_maps"))), warm, a.reps, interleaved=True,
                        fewer={"column maps pass": (1, a.column_reps)})
            for label, r in t.items():
                tail = "; protocol %d" % r.protocol
                if label == "deep maps pass":
                    tail += "; exact list %d, generic list %d" % (r.exact_list, r.generic_list)
                emit("%-19s %-50s %s (%d runs)%s; dominant kernel median %.3f ms, min %.3f ms"
                     % (label, r.kernel, stats(r.ms), len(r.ms), tail, r.med_dom, r.min_dom))
            dm, plain, default = t["deep maps pass"], t["plain default pass"], t["default pass"]
            emit("deep maps / default = %.3f; deep maps / plain default = %.3f (one more 4-byte store per %d bytes read: %.4f); "
                 "column maps / deep maps = %.1f"
                 % (dm.med / default.med, dm.med / plain.med, 4 * n, 1.0 + 1.0 / n, t["column maps pass"].med / dm.med))
            emit("dominant kernels, deep maps / plain default = %.4f, deep maps / default = %.4f; behind the dominant kernel: "
                 "%.3f ms (deep maps), %.3f ms (plain default), %.3f ms (default)"
                 % (dm.med_dom / plain.med_dom, dm.med_dom / default.med_dom, dm.med - dm.med_dom, plain.med - plain.med_dom,
                    default.med - default.med_dom))


def mad(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm, reps = 3, a.mad_reps
    emit = Report(a.out or os.path.join(ROOT, "profiles"), "maps_probe_mad.txt")
    emit("MAD sigma %.2f / %.2f and the median, frames of %d x %d resident; per depth one handle, %d repetitions "
         "after %d warm-up runs, default and full maps pass interleaved; GPU time of the whole pass" % (a.sigma, a.sigma, a.width, a.height, reps, warm))
    for n in [int(x) for x in a.mad_frames.split(",")]:
        emit("-- %d frames" % n)
        try:
            st = nl.StackHandle(n, a.width, a.height)
        except capi.NlError as e:
            emit("no handle of %d frames: %s" % (n, e))
            continue
        with st:
            st.fill_synthetic(seed=7)
            default_pass, maps_pass = pass_fns(st, L, capi.ST_MAD_SIGMA, a.sigma)
            # (the default MAD pass runs the plain protocol already: it is its own yardstick)
            # (the pair that is compared runs interleaved; the column kernel, which holds the device for a hundred times
            # as long, in a block of its own behind them: in between it shifts the passes next to it by 10 ... 20 %, either way)
            t = measure(st, (("default pass", default_pass), ("full maps pass", maps_pass("nl_stack_run_maps_full"))),
                        warm, reps, interleaved=True)
            t.update(measure(st, (("column maps pass", maps_pass("nl_stack_run_maps")),), warm, reps))
            for label, r in t.items():
                tail = "; protocol %d" % r.protocol
                if label != "column maps pass":
                    tail += "; exact list %d, generic list %d" % (r.exact_list, r.generic_list)
                emit("%-17s %-36s %s (%d runs)%s; dominant kernel median %.3f ms, min %.3f ms"
                     % (label, r.kernel, stats(r.ms), len(r.ms), tail, r.med_dom, r.min_dom))
            fm, default = t["full maps pass"], t["default pass"]
            emit("full maps / default = %.4f (one more 4-byte store per %d bytes read: %.4f); column maps / full maps = %.1f"
                 % (fm.med / default.med, 4 * n, 1.0 + 1.0 / n, t["column maps pass"].med / fm.med))
            emit("dominant kernels, full maps / default = %.4f; behind the dominant kernel: %.3f ms (full maps), %.3f ms (default)"
                 % (fm.med_dom / default.med_dom, fm.med - fm.med_dom, default.med - default.med_dom))
            if n == a.median_frames:
                default_pass, maps_pass = pass_fns(st, L, capi.ST_MEDIAN, a.sigma)
                t = measure(st, (("default pass", default_pass), ("full maps pass", maps_pass("nl_stack_run_maps_full"))),
                            warm, reps, interleaved=True)
                t.update(measure(st, (("column maps pass", maps_pass("nl_stack_run_maps")),), warm, reps))
                emit("-- %d frames, the median" % n)
                for label, r in t.items():
                    emit("%-17s %-36s %s (%d runs); protocol %d" % (label, r.kernel, stats(r.ms), len(r.ms), r.protocol))
                emit("full maps / default = %.4f (one memset of %d bytes beside %d bytes read); column maps / full maps = %.1f"
                     % (t["full maps pass"].med / t["default pass"].med, 4 * a.width * a.height, 4 * n * a.width * a.height,
                        t["column maps pass"].med / t["full maps pass"].med))


def column(a):
    import nightlight_amd as nl
    from nightlight_amd import capi
    L = capi.load()
    warm = 3
    emit = Report(a.out, "maps_probe.txt")
    emit("%d frames of %d x %d, mode %d, sigma %.2f / %.2f; %d runs after %d warm-up runs"
         % (a.frames, a.width, a.height, a.mode, a.sigma, a.sigma, a.reps, warm))
    with nl.StackHandle(a.frames, a.width, a.height) as st:
        st.fill_synthetic(seed=7)
        cov = np.zeros(a.width * a.height, np.uint16)
        default_pass, maps_pass = pass_fns(st, L, a.mode, a.sigma)

        def mean_pass():
            st.run(capi.ST_MEAN, a.sigma, a.sigma, 0.0, fetch=False)
            return st.pass_times(0)

        def coverage():
            st.coverage(out=cov)
            return st.last_coverage_ms, st.last_coverage_ms

        t = measure(st, (("default pass", default_pass), ("maps pass", maps_pass("nl_stack_run_maps")), ("mean pass", mean_pass),
                         ("coverage", coverage)), warm, a.reps)
        for label, r in t.items():
            emit("%-13s %-42s %s" % (label, "stack_coverage_kernel" if label == "coverage" else r.kernel, stats(r.ms)))
        read = 4.0 * a.frames * a.width * a.height
        emit("coverage / mean pass = %.3f; coverage reads %.2f GB: %.2f TB/s; maps pass / default pass = %.1f"
             % (t["coverage"].med / t["mean pass"].med, read / 1e9, read / t["coverage"].med / 1e9,
                t["maps pass"].med / t["default pass"].med))
        emit("coverage: %d ... %d frames per pixel" % (int(cov.min()), int(cov.max())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fastmaps", action="store_true")
    ap.add_argument("--linfit", action="store_true")
    ap.add_argument("--linfit-frames", default="128,32,256")
    ap.add_argument("--deep", action="store_true")
    ap.add_argument("--deep-workloads", default="512x4096x4096:2,256x4096x4096:2,512x4096x512:3")
    ap.add_argument("--column-reps", type=int, default=3)
    ap.add_argument("--mad", action="store_true")
    ap.add_argument("--mad-frames", default="32,128,256,512")
    ap.add_argument("--mad-reps", type=int, default=10)
    ap.add_argument("--median-frames", type=int, default=128)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--width", type=int, default=4096)
    ap.add_argument("--height", type=int, default=4096)
    ap.add_argument("--mode", type=int, default=2)
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    return (fastmaps if a.fastmaps else linfit if a.linfit else deep if a.deep else mad if a.mad else column)(a)


if __name__ == "__main__":
    main()
