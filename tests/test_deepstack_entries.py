"""The entries of the deep pass -- the median and MAD sigma of 513 ... 2048 frames on register-resident engines:
include/nlstack_deepstack.h (part of the interface nlstack.h includes) declares exactly capi.DEEPSTACK_EXPORTS, the
library exports them, every argument check that ends in front of the device gives its code and message (a
characterisation table in the form of tests/test_wmad_entries.py), and no entry gives a result where no handle can be
made.

The mode is checked behind the handle, as nl_stack_run checks it: a null handle with a bad mode is a null handle.  What
needs a handle -- the weighted MAD refusal, the fall-throughs -- is in tests/test_gpu_deepstack.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr
OTHERS = ("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "RESIDENTMAPS_EXPORTS", "DEEPMAPS_EXPORTS",
          "FULLMAPS_EXPORTS", "WLINFIT_EXPORTS", "WCLIP_EXPORTS", "WMAD_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS")


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_deepstack.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.DEEPSTACK_EXPORTS)
    assert not set(declared) & set(sum((getattr(capi, name) for name in OTHERS), []))
    assert '#include "nlstack_deepstack.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the entries take nl_stack_run's / nl_group_run's arguments
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nlstack.h")).read(), flags=re.S)
    proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
    assert proto(text, "nl_stack_run_deepstack") == proto(main, "nl_stack_run")
    assert proto(text, "nl_stack_run_deepstack_async") == proto(main, "nl_stack_run_async")
    assert proto(text, "nl_group_run_deepstack") == proto(main, "nl_group_run")
    # the header says what it is, gives the definition per mode, names engines, kernels and fall-throughs
    for word in ("EXTENSION OF DEPTH, NOT OF SEMANTICS", "Definition per mode.", "NL_ST_MEDIAN", "NL_ST_MAD_SIGMA",
                 "BIT FOR BIT", "COUNT FOR COUNT", "mad * 1.4826f", "never fused", "Engines.", "Fall-throughs.",
                 "stack_median_ml_kernel<8>", "stack_median_ml_kernel<16>", "stack_mad_ml_kernel<8>",
                 "stack_mad_ml_kernel<16>", "nl_stack_set_exact", "nl_stack_set_active_frames", "NL_ERR_WEIGHTED_MAD",
                 "NL_ERR_INVALID_MODE", "nl_stack_last_fallback_pixels", "nl_stack_finish"):
        assert word in raw, word


def test_build_checks_the_list():
    import inspect

    import __graft_entry__ as entry
    assert "capi.DEEPSTACK_EXPORTS" in inspect.getsource(entry.build)


def test_python_layer_has_the_methods():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert callable(cls.run_deepstack)
    assert callable(stack.StackHandle.run_deepstack_async)


def _i64():
    return C.byref(C.c_int64(0))


F32 = np.zeros(16, np.float32)
RUN, ASYNC, GROUP = "nl_stack_run_deepstack", "nl_stack_run_deepstack_async", "nl_group_run_deepstack"

# (row id, entry, call(L) -> return code)
ROWS = [
    ("run/null-handle", RUN, lambda L: L.nl_stack_run_deepstack(None, 0, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run/null-handle+null-outputs", RUN, lambda L: L.nl_stack_run_deepstack(None, 4, 2.0, 2.5, 0.0, None, None, None)),
    ("run/null-handle+bad-mode", RUN, lambda L: L.nl_stack_run_deepstack(None, 9, 2.0, 2.5, 0.0, None, None, None)),
    ("run_async/null-handle", ASYNC, lambda L: L.nl_stack_run_deepstack_async(None, 0, 2.0, 2.5, 0.0)),
    ("run_async/null-handle+bad-mode", ASYNC, lambda L: L.nl_stack_run_deepstack_async(None, -1, 2.0, 2.5, 0.0)),
    ("group_run/null-group", GROUP, lambda L: L.nl_group_run_deepstack(None, 4, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("group_run/null-group+null-outputs", GROUP, lambda L: L.nl_group_run_deepstack(None, 0, 2.0, 2.5, 0.0, None, None, None)),
]
EXPECTED = {
    "run/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+bad-mode": (capi.ERR_INVALID_ARG, "null handle"),
    "run_async/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run_async/null-handle+bad-mode": (capi.ERR_INVALID_ARG, "null handle"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.DEEPSTACK_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # the stack entries answer a null handle as nl_stack_run does
    assert run_row(L, lambda L: L.nl_stack_run(None, 0, 2.0, 2.5, 0.0, None, None, None)) == EXPECTED["run/null-handle"]


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
        for mode in (capi.ST_MEDIAN, capi.ST_MAD_SIGMA):
            out = np.full(16, np.float32(-7.5))
            cl, ch = C.c_int64(-3), C.c_int64(-4)
            rc = getattr(L, entry)(None, mode, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch))
            assert rc == capi.ERR_INVALID_ARG, entry
            assert np.all(out == np.float32(-7.5)) and (cl.value, ch.value) == (-3, -4), entry
