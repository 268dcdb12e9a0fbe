"""The location / scale entries of the C ABI: include/nlstack_locscale.h (the part of the interface nlstack.h includes)
declares exactly capi.LOCSCALE_EXPORTS, the library exports them, and on a machine without a device every argument
check that runs in front of the device gives its code and message, in the order the header states: a characterisation
table in the form of tests/test_frame_entry_errors.py, whose rows state the header's contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"

W = H = 4
F = np.arange(W * H, dtype=np.float32)
SEEDS = np.arange(1, 26, dtype=np.uint32)         # 25 nonzero seeds
SEEDS_ZERO = np.array([1, 0] + [1] * 23, np.uint32)
f = capi.fptr
seeds = SEEDS.ctypes.data_as(C.POINTER(C.c_uint32))
seeds_zero = SEEDS_ZERO.ctypes.data_as(C.POINTER(C.c_uint32))


def _fl():
    return C.byref(C.c_float(0))


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nlstack_locscale.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.LOCSCALE_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS)
    assert '#include "nlstack_locscale.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the struct and the constants as the header spells them
    assert C.sizeof(capi.LocScale) == 4 * (3 + 25 + 3 + 3)
    for name, value in (("NL_LSE_MEAN_STDDEV", capi.LSE_MEAN_STDDEV), ("NL_LSE_MEDIAN_MAD", capi.LSE_MEDIAN_MAD),
                        ("NL_LSE_IKSS", capi.LSE_IKSS), ("NL_LSE_SC_MEDIAN_QN", capi.LSE_SC_MEDIAN_QN),
                        ("NL_LSE_HISTOGRAM", capi.LSE_HISTOGRAM)):
        assert re.search(r"\b%s = %d\b" % (name, value), text)
    assert re.search(r"#define NL_LOCSCALE_SAMPLES %d\b" % capi.LOCSCALE_SAMPLES, text)
    assert re.search(r"#define NL_LOCSCALE_MAX_SEEDS %d\b" % capi.LOCSCALE_MAX_SEEDS, text)


# (row id, entry, call(L) -> return code)
ROWS = [
    ("frame_location_scale/null-handle", "nl_stack_frame_location_scale",
     lambda L: L.nl_stack_frame_location_scale(None, 0, 4, 0, None, 0, None, _fl(), _fl(), None)),
    ("frame_location_scale/null-handle+ikss", "nl_stack_frame_location_scale",
     lambda L: L.nl_stack_frame_location_scale(None, 0, 2, 1000, seeds, 25, None, _fl(), _fl(), None)),
    ("location_scale/null-data", "nl_location_scale",
     lambda L: L.nl_location_scale(None, W, H, 3, 1000, seeds, 25, None, _fl(), _fl(), None, 0)),
    ("location_scale/null-output", "nl_location_scale",
     lambda L: L.nl_location_scale(f(F), W, H, 3, 1000, seeds, 25, None, None, _fl(), None, 0)),
    ("location_scale/samples-3", "nl_location_scale",
     lambda L: L.nl_location_scale(f(F), W, H, 3, 3, seeds, 25, None, _fl(), _fl(), None, 0)),
    ("location_scale/zero-seed", "nl_location_scale",
     lambda L: L.nl_location_scale(f(F), W, H, 3, 1000, seeds_zero, 25, None, _fl(), _fl(), None, 0)),
    ("location_scale/too-few-seeds", "nl_location_scale",
     lambda L: L.nl_location_scale(f(F), W, H, 1, 1000, seeds, 1, None, _fl(), _fl(), None, 0)),
    ("location_scale/valid", "nl_location_scale",
     lambda L: L.nl_location_scale(f(F), W, H, 3, 1000, seeds, 25, None, _fl(), _fl(), None, 0)),
    ("locscale_seeds/null-output", "nl_locscale_seeds", lambda L: L.nl_locscale_seeds(1, None, 3)),
    ("locscale_seeds/valid", "nl_locscale_seeds", lambda L: L.nl_locscale_seeds(1, seeds, 25)),
]

NO_DEVICE = (capi.ERR_NO_DEVICE,
             "no HIP device available (no ROCm-capable device is detected); libnlstack has no CPU path")
UNTOUCHED = (capi.OK, SENTINEL)           # the call succeeded and left the thread's error as it was

EXPECTED = {
    "frame_location_scale/null-handle": (-6, "null handle"),
    "frame_location_scale/null-handle+ikss": (-6, "frame_location_scale: estimator 2, LSEIKSS (stats.go:535-566), sorts the whole frame: not implemented on the device"),
    "location_scale/null-data": (-6, "location_scale: bad argument"),
    "location_scale/null-output": (-6, "location_scale: null output"),
    "location_scale/samples-3": (-6, "location_scale: 3 samples (4 .. 1048576)"),
    "location_scale/zero-seed": (-6, "location_scale: seed 1 is zero (fastrand would replace it by one from the clock)"),
    "location_scale/too-few-seeds": (-6, "location_scale: 1 seeds, estimator 1 reads 2"),
    "location_scale/valid": NO_DEVICE,
    "locscale_seeds/null-output": (-6, "locscale_seeds: 3 seeds with no output"),
    "locscale_seeds/valid": UNTOUCHED,
}


def run_row(L, call):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, np.float32)
    assert L.nl_weights_from_scalars(7, f(w), 1, f(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


def test_every_entry_has_a_row():
    assert {entry for _, entry, _ in ROWS} == set(capi.LOCSCALE_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    """With a device only the rows that end in front of it are compared (the others need a real frame to succeed)."""
    L = capi.load()
    has_device = capi.device_count() > 0
    got = {rid: run_row(L, call) for rid, _, call in ROWS if not (has_device and EXPECTED[rid] == NO_DEVICE)}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
