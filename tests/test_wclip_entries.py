"""The entries of the weighted clip pass whose weights follow their frames: include/nlstack_wclip.h (part of the
interface nlstack.h includes) declares exactly capi.WCLIP_EXPORTS, the library exports them, every argument check that
ends in front of the device gives its code and message (a characterisation table in the form of
tests/test_maps_entries.py), no entry gives a result where no handle can be made, and the host operator's JSON
carries the switch only when it is set.

What can be told from the mode alone -- an id out of range, the median, the mean, MAD sigma, the linear fit -- is told in
front of the handle, so these rows need no device.  "No weights" needs a handle: tests/test_gpu_wclip.py has it."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from nightlight_amd import capi
from nightlight_amd import operator as host_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_wclip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.WCLIP_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.FASTMAPS_EXPORTS +
                                   capi.WLINFIT_EXPORTS + capi.ALIGN_EXPORTS + capi.RESAMPLE_EXPORTS)
    assert '#include "nlstack_wclip.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is and carries the definition
    for word in ("EXTENSION", "Definition.", "num += v_k * w_k", "AFTER the last removal sweep",
                 "order of summation only", "stack.go:487"):
        assert word in raw, word


def test_python_layer_has_the_methods():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert callable(cls.run_clip_weighted)
    assert callable(stack.StackHandle.run_clip_weighted_async)


def _i64():
    return C.byref(C.c_int64(0))


F32 = np.zeros(16, np.float32)
RUN, ASYNC, GROUP = "nl_stack_run_clip_weighted", "nl_stack_run_clip_weighted_async", "nl_group_run_clip_weighted"
NEITHER = "run_clip_weighted: mode %d is neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA"
GROUP_NEITHER = "run_clip_weighted: the mode is neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA"
OTHER_MODES = [("median", capi.ST_MEDIAN), ("mean", capi.ST_MEAN), ("mad", capi.ST_MAD_SIGMA), ("linear-fit", capi.ST_LINEAR_FIT)]

# (row id, entry, call(L) -> return code)
ROWS = [
    ("run/null-handle", RUN, lambda L: L.nl_stack_run_clip_weighted(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run/null-handle+winsor+null-outputs", RUN, lambda L: L.nl_stack_run_clip_weighted(None, 3, 2.0, 2.5, 0.0, None, None, None)),
    ("run/null-handle+auto", RUN, lambda L: L.nl_stack_run_clip_weighted(None, 6, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run_async/null-handle", ASYNC, lambda L: L.nl_stack_run_clip_weighted_async(None, 2, 2.0, 2.5, 0.0)),
    ("group_run/null-group", GROUP, lambda L: L.nl_group_run_clip_weighted(None, 3, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("group_run/null-group+auto", GROUP, lambda L: L.nl_group_run_clip_weighted(None, 6, 2.0, 2.5, 0.0, None, None, None)),
]
EXPECTED = {
    "run/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+winsor+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+auto": (capi.ERR_INVALID_ARG, "null handle"),
    "run_async/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "group_run/null-group": (capi.ERR_INVALID_ARG, "null group"),
    "group_run/null-group+auto": (capi.ERR_INVALID_ARG, "null group"),
}
for bad in (-1, 7, 9):
    ROWS += [("run/mode%d" % bad, RUN, lambda L, m=bad: L.nl_stack_run_clip_weighted(None, m, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
             ("run_async/mode%d" % bad, ASYNC, lambda L, m=bad: L.nl_stack_run_clip_weighted_async(None, m, 2.0, 2.5, 0.0)),
             ("group_run/mode%d" % bad, GROUP, lambda L, m=bad: L.nl_group_run_clip_weighted(None, m, 2.0, 2.5, 0.0, f(F32), _i64(), _i64()))]
    for e in ("run", "run_async", "group_run"):
        EXPECTED["%s/mode%d" % (e, bad)] = (capi.ERR_INVALID_MODE, "invalid stacking mode")
for name, mode in OTHER_MODES:
    ROWS += [("run/%s" % name, RUN, lambda L, m=mode: L.nl_stack_run_clip_weighted(None, m, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
             ("run_async/%s" % name, ASYNC, lambda L, m=mode: L.nl_stack_run_clip_weighted_async(None, m, 2.0, 2.5, 0.0)),
             ("group_run/%s" % name, GROUP, lambda L, m=mode: L.nl_group_run_clip_weighted(None, m, 2.0, 2.5, 0.0, f(F32), _i64(), _i64()))]
    EXPECTED["run/%s" % name] = EXPECTED["run_async/%s" % name] = (capi.ERR_INVALID_MODE, NEITHER % mode)
    EXPECTED["group_run/%s" % name] = (capi.ERR_INVALID_MODE, GROUP_NEITHER)


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
    assert {entry for _, entry, _ in ROWS} == set(capi.WCLIP_EXPORTS)
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
        with pytest.raises(capi.NlError):
            nl.StackGroup(4, 8, 8)
    for entry in (RUN, GROUP):
        out = np.full(16, np.float32(-7.5))
        cl, ch = C.c_int64(-3), C.c_int64(-4)
        rc = getattr(L, entry)(None, 2, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch))
        assert rc == capi.ERR_INVALID_ARG, entry
        assert np.all(out == np.float32(-7.5)) and (cl.value, ch.value) == (-3, -4), entry


def test_operator_json_carries_the_switch_only_when_set():
    plain = host_op.op_stack_roundtrip_json('{"type":"stack"}')
    assert plain == '{"type":"stack","mode":6,"weighting":0,"sigmaLow":2.75,"sigmaHigh":2.75}'       # exactly as before
    full = '{"type":"stack","mode":3,"weighting":2,"sigmaLow":2.75,"sigmaHigh":3}'
    assert host_op.op_stack_roundtrip_json(full) == full
    assert "weightsFollowFrames" not in host_op.op_stack_roundtrip_json('{"type":"stack","weightsFollowFrames":false}')
    on = host_op.op_stack_roundtrip_json('{"type":"stack","mode":3,"weighting":2,"weightsFollowFrames":true}')
    assert json.loads(on) == {"type": "stack", "mode": 3, "weighting": 2, "sigmaLow": 2.75, "sigmaHigh": 2.75,
                              "weightsFollowFrames": True}
    assert host_op.op_stack_roundtrip_json(on) == on
    both = host_op.op_stack_roundtrip_json('{"type":"stack","weightsFollowFrames":true,"weightedLinearFit":true}')
    assert json.loads(both)["weightsFollowFrames"] is True and json.loads(both)["weightedLinearFit"] is True
