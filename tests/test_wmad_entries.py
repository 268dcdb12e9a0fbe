"""The entries of the weighted MAD-sigma pass whose weights follow their frames: include/nlstack_wmad.h (part of the
interface nlstack.h includes) declares exactly capi.WMAD_EXPORTS, the library exports them, every argument check that
ends in front of the device gives its code and message (a characterisation table in the form of
tests/test_wclip_entries.py), and no entry gives a result where no handle can be made.

The entries take no mode, so nothing but the handle can be wrong in front of the device.  "No weights" needs a handle:
tests/test_gpu_wmad.py has it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_wmad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.WMAD_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.FASTMAPS_EXPORTS +
                                   capi.RESIDENTMAPS_EXPORTS + capi.DEEPMAPS_EXPORTS + capi.WLINFIT_EXPORTS +
                                   capi.WCLIP_EXPORTS + capi.ALIGN_EXPORTS + capi.RESAMPLE_EXPORTS)
    assert '#include "nlstack_wmad.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is and carries the definition
    for word in ("EXTENSION", "Definition.", "num += v_k * w_k", "mad * 1.4826f", "never fused", "stack.go:185",
                 "A median that is not finite", "NL_ERR_WEIGHTED_MAD"):
        assert word in raw, word


def test_python_layer_has_the_methods():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert callable(cls.run_mad_weighted)
    assert callable(stack.StackHandle.run_mad_weighted_async)


def _i64():
    return C.byref(C.c_int64(0))


F32 = np.zeros(16, np.float32)
RUN, ASYNC, GROUP = "nl_stack_run_mad_weighted", "nl_stack_run_mad_weighted_async", "nl_group_run_mad_weighted"

# (row id, entry, call(L) -> return code)
ROWS = [
    ("run/null-handle", RUN, lambda L: L.nl_stack_run_mad_weighted(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run/null-handle+null-outputs", RUN, lambda L: L.nl_stack_run_mad_weighted(None, 2.0, 2.5, 0.0, None, None, None)),
    ("run_async/null-handle", ASYNC, lambda L: L.nl_stack_run_mad_weighted_async(None, 2.0, 2.5, 0.0)),
    ("group_run/null-group", GROUP, lambda L: L.nl_group_run_mad_weighted(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("group_run/null-group+null-outputs", GROUP, lambda L: L.nl_group_run_mad_weighted(None, 2.0, 2.5, 0.0, None, None, None)),
]
EXPECTED = {
    "run/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "run_async/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "group_run/null-group": (capi.ERR_INVALID_ARG, "null group"),
    "group_run/null-group+null-outputs": (capi.ERR_INVALID_ARG, "null group"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.WMAD_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_no_cpu_result_where_no_handle_can_be_made():
    """A pass needs a handle, and a handle needs a device: where none is visible making one fails ("no HIP device"),
    and the entries, left without a handle, end with NL_ERR_INVALID_ARG and their outputs untouched -- never with a
    result of the CPU."""
    import nightlight_amd as nl
    L = capi.load()
    if capi.device_count() == 0:
        with pytest.raises(capi.NlError) as e:
            nl.StackHandle(4, 8, 8)
        assert "no HIP device" in str(e.value) or "hipGetDeviceCount" in str(e.value)
    for entry in (RUN, GROUP):
        out = np.full(16, np.float32(-7.5))
        cl, ch = C.c_int64(-3), C.c_int64(-4)
        rc = getattr(L, entry)(None, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch))
        assert rc == capi.ERR_INVALID_ARG, entry
        assert np.all(out == np.float32(-7.5)) and (cl.value, ch.value) == (-3, -4), entry
