#!/usr/bin/env python3
"""Times of the colour steps of the rgb / lrgb command on the device (colour.hip).

  python tools/colour_probe.py --out DIR
      wall time per call (median of 10 after 2 warm-up calls; every call ends in a stream sync, the clamp with
      statistics also in three 48 KiB copies of the partials, the darkest block in the download of its block means, the
      exports in the download of their counts -- so this is device time plus launch, copy and sync overhead) on a
      resident 4096^2 three-slot handle: every new entry, and the one comparison there is: the parent's
      nl_stack_frame_affine followed by nl_stack_frame_stats per plane (six launches, no clamp) against
      nl_stack_rgb_scale_offset_clamp with statistics.
      Then the calls run once more under `rocprofv3 --kernel-trace --stats` (a child process with its own time limit)
      and every colour kernel's per-dispatch durations are printed with its rate against the bytes it must move -- 8 B
      per pixel and plane for the clamp, the combine and the chroma steps (12 for rotate-hues' two reads), 12 B read per
      pixel for the block means, 20 or 16 B per pixel for the export -- as a share of the MI355X's 8 TB/s HBM peak.
      DIR receives the summary (colour_probe.txt) and the trace.  Recorded, not gated: there is no earlier device form
      of these steps.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stars_probe import dispatches  # noqa: E402
from tone_probe import HBM_PEAK, H, N, W, median_ms  # noqa: E402

P = (0, 1, 2)


def stars(n=2000):
    import nightlight_amd as nl
    rng = np.random.default_rng(6)
    s = np.zeros(n, nl.capi.STAR_DTYPE)
    s["index"] = rng.integers(0, N, n).astype(np.int32)
    s["hfr"] = rng.uniform(1.0, 6.0, n).astype(np.float32)
    return s


def cases(nl, st, src):
    """(label, call): in place, so the planes drift from call to call; the work per call does not depend on the values"""
    one, zero, rgb = (0.999, 0.999, 0.999), (0.0005, 0.0005, 0.0005), (0.9, 0.9, 0.9)
    s = stars()
    out = [("combine_from", lambda: st.frame_combine_from(0, src, 0, 0.0005, 0.999)),
           ("clamp", lambda: st.rgb_scale_offset_clamp(P, one, zero)),
           ("clamp + stats", lambda: st.rgb_scale_offset_clamp(P, one, zero, stats=True)),
           ("3 x (affine, frame_stats)", lambda: [(st.frame_affine(c, 0.999, 0.0005), st.frame_stats(c, variance=False)) for c in P])]
    for block in (16, 64):
        out.append(("darkest block %d" % block, lambda block=block: st.rgb_darkest_block(P, block, 0.1)))
    out.append(("star intensity, 2000 stars", lambda: st.rgb_mean_star_intensity(P, s, 0.0, 0.75, rgb)))
    out.append(("balance", lambda: st.rgb_balance(P, s, 16, 0.1, 0.0, 0.75, (0.1, 0.1, 0.1), (0.9, 0.9, 0.9),
                                                  (0.4, 0.4, 0.4), (0.1, 0.1, 0.1))))
    for label, kind, p in (("chroma gamma", nl.CHROMA_GAMMA, (1.5, 0.1)), ("neutralize", nl.CHROMA_NEUTRALIZE, (0.05, 0.1)),
                           ("chroma for hues", nl.CHROMA_FOR_HUES, (0.8, 0.1, 0.5)), ("rotate hues", nl.ROTATE_HUES, (0.3, 0.6, 0.01, 0.1))):
        out.append((label, lambda kind=kind, p=p: st.rgb_chroma(P, kind, *p)))
    for bits in (16, 8):
        out.append(("export %d bits" % bits, lambda bits=bits: st.rgb_export(P, 0.0, 1.0, 1.0, bits)))
        out.append(("export %d bits, gamma 2.2" % bits, lambda bits=bits: st.rgb_export(P, 0.0, 1.0, 2.2, bits)))
    return out


def run_calls(reps):
    import nightlight_amd as nl
    lines = []
    rng = np.random.default_rng(5)
    with nl.StackHandle(3, W, H) as st, nl.StackHandle(1, W, H) as src:
        for c in P:
            st.upload_frame(c, rng.random(N, dtype=np.float32))
        src.upload_frame(0, rng.random(N, dtype=np.float32))
        for label, call in cases(nl, st, src):
            med, mn = median_ms(call, reps)
            lines.append("%-28s 4096^2: median %.3f ms, min %.3f ms per call" % (label, med, mn))
    return lines


def bytes_per_pixel(name):
    """what one dispatch of the kernel must move, per pixel of one plane (the clamp: of its three planes)"""
    if "export_rgb_kernel<16" in name:
        return 20
    if "export_rgb_kernel<8" in name:
        return 16
    if "block_means_kernel" in name:
        return 12
    if "rgb_clamp_kernel" in name:
        return 24
    if "chroma_kernel<3" in name:
        return 12
    if "min_sum_max" in name:
        return 4
    return 8


def kernel_stats(out_dir):
    trace = os.path.join(out_dir, "colour_rocprof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "run",
           "--", sys.executable, os.path.abspath(__file__), "--inner", "--out", out_dir]
    rc = subprocess.call(cmd, cwd=ROOT)
    if rc != 0:
        return ["rocprofv3 run failed with status %d" % rc]
    lines = ["rocprofv3 --kernel-trace: per kernel dispatches, min / median / max in us; share = algorithmic bytes / min / 8 TB/s",
             "(rgb_clamp_kernel<stats, vec>: three planes per dispatch; block_means_kernel<staged> with border 0.1: 0.64 of "
             "the frame is read, the share is against the whole frame; min_sum_max_kernel and affine_kernel: the parent's pair)"]
    keys = ("combine_kernel", "rgb_clamp_kernel", "block_means_kernel", "star_sums_kernel", "chroma_kernel",
            "export_rgb_kernel", "min_sum_max_kernel", "affine_kernel")
    for name, ns in sorted(dispatches(trace).items()):
        if not any(k in name for k in keys):
            continue
        bpp = bytes_per_pixel(name)
        lines.append("%-44s %3d %9.1f %9.1f %9.1f  %4.0f MB  %3.0f %%"
                     % (name[-44:], len(ns), min(ns) / 1e3, float(np.median(ns)) / 1e3, max(ns) / 1e3,
                        bpp * N / 1e6, 100.0 * bpp * N / (min(ns) * 1e-9) / HBM_PEAK))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", action="store_true", help="the calls only (the run under rocprofv3)")
    ap.add_argument("--out", required=True, help="directory for the summary and the rocprofv3 trace")
    a = ap.parse_args()
    if a.inner:
        run_calls(3)
        return
    os.makedirs(a.out, exist_ok=True)
    lines = run_calls(10) + [""] + kernel_stats(a.out)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "colour_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
