#!/usr/bin/env python3
"""Times of nl_stack_frame_location_scale on a resident 4096^2 frame against what it replaces: the download of the frame
plus the estimate on the host.

  python tools/locscale_probe.py --out DIR
      Per estimator (0 mean / stddev, 1 median / MAD, 3 sigma-clipped median / Qn with NL_LOCSCALE_SAMPLES, 4 histogram):
      the time of one call between two HIP events on the handle's stream, 3 warm-up calls, the median and minimum of 10
      (the calls read back a few bytes per sampling call, so this is device time plus launch, copy and sync overhead,
      which is what a caller waits for).  Then nl_stack_download_tile of the frame between the same events, and the
      wall time of tools/locscale_host.c (compiled here with cc -O2, one thread) for estimator 3 with the same seeds on
      the downloaded frame, whose result must equal the device's bits.  DIR receives locscale_probe.txt.  Recorded, not
      gated.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096
WARM, REPS = 3, 10


def sky():
    rng = np.random.default_rng(5)
    d = rng.normal(1000.0, 30.0, W * H)
    out = rng.random(W * H) < 0.01
    d[out] += rng.uniform(500.0, 20000.0, int(out.sum()))
    return d.astype(np.float32)


def load_hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    else:
        raise SystemExit("libamdhip64.so not found")
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def event_ms(hip, stream, fn):
    """(median, min) ms of fn() between two events on `stream`"""
    start, stop = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(start)) == 0 and hip.hipEventCreate(C.byref(stop)) == 0
    t = []
    for k in range(WARM + REPS):
        assert hip.hipEventRecord(start, stream) == 0
        fn()
        assert hip.hipEventRecord(stop, stream) == 0 and hip.hipEventSynchronize(stop) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), start, stop) == 0
        if k >= WARM:
            t.append(ms.value)
    hip.hipEventDestroy(start)
    hip.hipEventDestroy(stop)
    return float(np.median(t)), float(np.min(t))


def host_estimator(tmp):
    lib_path = os.path.join(tmp, "liblocscale_host.so")
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "locscale_host.c"),
                           "-o", lib_path, "-lm"])
    lib = C.CDLL(lib_path)
    lib.locscale_host.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_float,
                                  C.POINTER(C.c_float), C.POINTER(C.c_float)]
    return lib.locscale_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="directory for locscale_probe.txt")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import nightlight_amd as nl
    hip = load_hip()
    seeds = nl.locscale_seeds(2024)
    lines = []
    with nl.StackHandle(1, W, H) as st:
        st.upload_frame(0, sky())
        stream = C.c_void_p(st.stream_ptr)
        results = {}
        for label, estimator in (("0 mean / stddev", nl.LSE_MEAN_STDDEV), ("1 median / MAD", nl.LSE_MEDIAN_MAD),
                                 ("3 sc median / Qn", nl.LSE_SC_MEDIAN_QN), ("4 histogram", nl.LSE_HISTOGRAM)):
            def call(estimator=estimator):
                results[estimator] = st.frame_location_scale(0, estimator, seeds)
            med, mn = event_ms(hip, stream, call)
            loc, scale, info = results[estimator]
            lines.append("estimator %-18s 4096^2: median %.3f ms, min %.3f ms per estimate (location %.6g, scale %.6g, "
                         "%d iterations, %d sampling calls)" % (label, med, mn, loc, scale, info["iterations"],
                                                                 info["seeds_used"]))
        frames = {}
        med, mn = event_ms(hip, stream, lambda: frames.__setitem__(0, st.download_tile(0)))
        lines.append("download of the frame (64 MiB, pageable destination): median %.3f ms, min %.3f ms = %.1f GiB/s"
                     % (med, mn, 0.0625 / (mn * 1e-3)))
    frame = frames[0]
    loc3, scale3, info3 = results[nl.LSE_SC_MEDIAN_QN]
    with tempfile.TemporaryDirectory() as tmp:
        host = host_estimator(tmp)
        t = []
        for k in range(WARM + REPS):
            loc, scale = C.c_float(), C.c_float()
            t0 = time.perf_counter()
            iterations = host(frame.ctypes.data_as(C.POINTER(C.c_float)), frame.size, nl.LOCSCALE_SAMPLES,
                              seeds.ctypes.data_as(C.POINTER(C.c_uint32)), float(info3["epsilon"]), C.byref(loc),
                              C.byref(scale))
            if k >= WARM:
                t.append(1e3 * (time.perf_counter() - t0))
    same = (np.float32(loc.value).tobytes() == loc3.tobytes() and np.float32(scale.value).tobytes() == scale3.tobytes()
            and iterations == info3["iterations"])
    lines.append("estimator 3 on the host (tools/locscale_host.c, one thread of %d usable CPUs): median %.3f ms, min %.3f ms; "
                 "%s the device's bits" % (len(os.sched_getaffinity(0)), float(np.median(t)), float(np.min(t)),
                                           "equals" if same else "DIFFERS FROM"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "locscale_probe.txt"), "w") as f:
        f.write(text)
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
