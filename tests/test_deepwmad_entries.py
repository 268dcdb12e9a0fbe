"""The entries of the deep weighted MAD-sigma pass -- nl_stack_run_mad_weighted of 513 ... 2048 frames on the 8- / 16-lane
engine: include/nlstack_deepwmad.h (part of the interface nlstack.h includes) declares exactly capi.DEEPWMAD_EXPORTS, the
library exports them, they are no entry of another list, they take the arguments of the nl_stack_run_mad_weighted family,
every argument check that ends in front of the device gives that family's code and message, and no entry gives a result
where no handle can be made.  In the form of tests/test_deepstack_entries.py.  What needs a handle -- the refusal of a
handle without weights, the fall-throughs -- is in tests/test_gpu_deepwmad.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr
RUN, ASYNC, GROUP = ("nl_stack_run_mad_weighted_deepstack", "nl_stack_run_mad_weighted_deepstack_async",
                     "nl_group_run_mad_weighted_deepstack")
SIBLING = {RUN: "nl_stack_run_mad_weighted", ASYNC: "nl_stack_run_mad_weighted_async", GROUP: "nl_group_run_mad_weighted"}
OTHERS = ("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "RESIDENTMAPS_EXPORTS", "DEEPMAPS_EXPORTS",
          "FULLMAPS_EXPORTS", "WLINFIT_EXPORTS", "WCLIP_EXPORTS", "WMAD_EXPORTS", "DEEPSTACK_EXPORTS",
          "DEEPSTACKMAPS_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS")
WORDS = ("EXTENSION OF DEPTH, NOT OF SEMANTICS", "Definition.", "mad * 1.4826f", "never fused", "FRAME INDEX", "BIT FOR BIT",
         "COUNT FOR COUNT", "Engines.", "Fall-throughs.", "Errors.", "stack_mad_ml_kernel<8, true>",
         "stack_mad_ml_kernel<16, true>", "stack_clip_weighted_kernel<4, true>", "stack_exact_kernel<mad,follow>",
         "nl_stack_run_mad_weighted", "nl_stack_set_exact", "nl_stack_set_active_frames", "nl_stack_set_weights",
         "NL_ERR_INVALID_ARG", "nl_stack_last_fallback_pixels", "nl_stack_finish")


def _i64():
    return C.byref(C.c_int64(0))


F32 = np.zeros(16, np.float32)

# (row id, entry, call(L, entry name) -> return code): each row also runs on the entry's sibling of nlstack_wmad.h
ROWS = [
    ("run/null-handle", RUN, lambda L, e: getattr(L, e)(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run/null-handle+null-outputs", RUN, lambda L, e: getattr(L, e)(None, 2.0, 2.5, 0.0, None, None, None)),
    ("run_async/null-handle", ASYNC, lambda L, e: getattr(L, e)(None, 2.0, 2.5, 0.0)),
    ("group_run/null-group", GROUP, lambda L, e: getattr(L, e)(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("group_run/null-group+null-outputs", GROUP, lambda L, e: getattr(L, e)(None, 2.0, 2.5, 0.0, None, None, None)),
]
EXPECTED = {
    "run/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run/null-handle+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "run_async/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "group_run/null-group": (capi.ERR_INVALID_ARG, "null group"),
    "group_run/null-group+null-outputs": (capi.ERR_INVALID_ARG, "null group"),
}


def _uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, header)).read(), flags=re.S)


def test_header_exports_and_binding_agree():
    raw = open(os.path.join(INC, "nlstack_deepwmad.h")).read()
    text = _uncommented("nlstack_deepwmad.h")
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.DEEPWMAD_EXPORTS) == sorted([RUN, ASYNC, GROUP])
    assert not set(declared) & set(sum((getattr(capi, name) for name in OTHERS), []))
    assert '#include "nlstack_deepwmad.h"' in open(os.path.join(INC, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the entries take the arguments of their siblings
    wmad = _uncommented("nlstack_wmad.h")
    proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
    for entry, sibling in SIBLING.items():
        assert proto(text, entry) == proto(wmad, sibling), entry
    for word in WORDS:
        assert word in raw, word


def test_build_checks_the_list():
    import __graft_entry__ as entry
    assert "capi.DEEPWMAD_EXPORTS" in inspect.getsource(entry.build)


def test_python_layer_has_the_methods():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert inspect.signature(cls.run_mad_weighted_deepstack) == inspect.signature(cls.run_mad_weighted)
    assert (inspect.signature(stack.StackHandle.run_mad_weighted_deepstack_async) ==
            inspect.signature(stack.StackHandle.run_mad_weighted_async))
    L = capi.load()
    for entry, sibling in SIBLING.items():
        assert getattr(L, entry).argtypes == getattr(L, sibling).argtypes, entry


def run_row(L, call, entry):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, np.float32)
    assert L.nl_weights_from_scalars(7, f(w), 1, f(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L, entry)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


def test_every_entry_has_a_row():
    assert {entry for _, entry, _ in ROWS} == set(capi.DEEPWMAD_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call, entry) for rid, entry, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # ... which is what the sibling of nlstack_wmad.h gives for the same arguments
    assert {rid: run_row(L, call, SIBLING[entry]) for rid, entry, call in ROWS} == got


@pytest.mark.parametrize("entry", [RUN, GROUP])
def test_no_cpu_result_where_no_handle_can_be_made(entry):
    """A pass needs a handle, and a handle needs a device: where none is visible making one fails, and the entries, left
    without a handle, end with NL_ERR_INVALID_ARG and their outputs untouched -- never with a result of the CPU."""
    import nightlight_amd as nl
    L = capi.load()
    if capi.device_count() == 0:
        with pytest.raises(capi.NlError) as e:
            nl.StackHandle(4, 8, 8)
        assert "no HIP device" in str(e.value) or "hipGetDeviceCount" in str(e.value)
    out = np.full(16, np.float32(-7.5))
    cl, ch = C.c_int64(-3), C.c_int64(-4)
    rc = getattr(L, entry)(None, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch))
    assert rc == capi.ERR_INVALID_ARG, entry
    assert np.all(out == np.float32(-7.5)) and (cl.value, ch.value) == (-3, -4), entry
