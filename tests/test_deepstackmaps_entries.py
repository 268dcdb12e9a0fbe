"""The entries of the deep-stack maps pass -- the rejection maps of stacks beyond 512 frames at the speed of the pass:
include/nlstack_deepstackmaps.h (part of the interface nlstack.h includes) declares exactly capi.DEEPSTACKMAPS_EXPORTS, the
library exports them, they are no entry of another list, they take the arguments of nl_stack_run_maps_full /
nl_group_run_maps_full, every argument check that ends in front of the device gives that entry's code and message, and no
entry gives a result where no handle can be made.  In the form of tests/test_deepstack_entries.py and
tests/test_fullmaps_entries.py.  What needs a handle is in tests/test_gpu_deepstackmaps.py."""
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
STACK, GROUP = "nl_stack_run_maps_deepstack", "nl_group_run_maps_deepstack"
OTHERS = ("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "RESIDENTMAPS_EXPORTS", "DEEPMAPS_EXPORTS",
          "FULLMAPS_EXPORTS", "WLINFIT_EXPORTS", "WCLIP_EXPORTS", "WMAD_EXPORTS", "DEEPSTACK_EXPORTS", "DEEPWMAD_EXPORTS",
          "ALIGN_EXPORTS", "RESAMPLE_EXPORTS")
WORDS = ("Definition per mode.", "NL_ST_MAD_SIGMA", "NL_ST_MEDIAN", "NL_ST_SIGMA", "NL_ST_WINSOR_SIGMA", "BIT FOR BIT",
         "COUNT FOR COUNT", "Engines.", "Fall-throughs.", "Errors.", "stack_mad_ml_kernel<8, maps>",
         "stack_mad_ml_kernel<16, maps>", "stack_median_ml_kernel<8>", "stack_median_ml_kernel<16>",
         "stack_sigma_coop_kernel<", "stack_exact_kernel<mad,maps>", "nl_stack_run_maps_full", "nl_stack_run_deepstack",
         "nl_stack_set_exact", "nl_stack_set_active_frames", "NL_ERR_INVALID_MODE", "NL_ERR_WEIGHTED_MAD",
         "NL_ERR_TOO_MANY_FRAMES", "nl_stack_last_fallback_pixels", "linear fit")


def _i64():
    return C.byref(C.c_int64(0))


U16 = np.zeros(16, np.uint16)
u16 = U16.ctypes.data_as(C.POINTER(C.c_uint16))
F32 = np.zeros(16, np.float32)

# (row id, entry, the existing entry that gives the expected code and message, call(L, entry name) -> return code)
ROWS = [
    ("run_maps_deepstack/null-handle", STACK, "nl_stack_run_maps_full",
     lambda L, e: getattr(L, e)(None, 4, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_deepstack/null-handle+null-outputs", STACK, "nl_stack_run_maps_full",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("run_maps_deepstack/null-handle+bad-mode", STACK, "nl_stack_run_maps_full",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_deepstack/null-group", GROUP, "nl_group_run_maps_full",
     lambda L, e: getattr(L, e)(None, 4, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_deepstack/null-group+null-outputs", GROUP, "nl_group_run_maps_full",
     lambda L, e: getattr(L, e)(None, 0, 2.0, 2.5, 0.0, None, None, None, None, None)),
]
EXPECTED = {
    "run_maps_deepstack/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "run_maps_deepstack/null-handle+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "run_maps_deepstack/null-handle+bad-mode": (capi.ERR_INVALID_ARG, "null handle"),
    "group_run_maps_deepstack/null-group": (capi.ERR_INVALID_ARG, "null group"),
    "group_run_maps_deepstack/null-group+null-outputs": (capi.ERR_INVALID_ARG, "null group"),
}


def _uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, header)).read(), flags=re.S)


def test_header_exports_and_binding_agree():
    raw = open(os.path.join(INC, "nlstack_deepstackmaps.h")).read()
    text = _uncommented("nlstack_deepstackmaps.h")
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.DEEPSTACKMAPS_EXPORTS) == sorted([STACK, GROUP])
    assert not set(declared) & set(sum((getattr(capi, name) for name in OTHERS), []))
    assert '#include "nlstack_deepstackmaps.h"' in open(os.path.join(INC, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the maps are uint16, and the entries take the arguments of the entries they stand beside
    assert len(re.findall(r"uint16_t \*", text)) == 4
    full = _uncommented("nlstack_fullmaps.h")
    proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
    assert proto(text, STACK) == proto(full, "nl_stack_run_maps_full")
    assert proto(text, GROUP) == proto(full, "nl_group_run_maps_full")
    for word in WORDS:
        assert word in raw, word


def test_build_checks_the_list():
    import __graft_entry__ as entry
    assert "capi.DEEPSTACKMAPS_EXPORTS" in inspect.getsource(entry.build)


def test_python_layer_has_both_methods():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert inspect.signature(cls.run_maps_deepstack) == inspect.signature(cls.run_maps_full)
    L = capi.load()
    assert L.nl_stack_run_maps_deepstack.argtypes == L.nl_stack_run_maps_full.argtypes
    assert L.nl_group_run_maps_deepstack.argtypes == L.nl_group_run_maps_full.argtypes


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
    assert {r[1] for r in ROWS} == set(capi.DEEPSTACKMAPS_EXPORTS)
    ids = [r[0] for r in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call, entry) for rid, entry, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # ... which is what the entry it stands beside gives for the same arguments
    assert {rid: run_row(L, call, existing) for rid, _, existing, call in ROWS} == got


@pytest.mark.parametrize("entry", [STACK, GROUP])
@pytest.mark.parametrize("mode", [capi.ST_MEDIAN, capi.ST_SIGMA, capi.ST_WINSOR_SIGMA, capi.ST_MAD_SIGMA])
def test_no_cpu_result_where_no_handle_can_be_made(entry, mode):
    """as every maps entry: no handle, NL_ERR_INVALID_ARG, the outputs untouched -- never a result of the CPU"""
    import nightlight_amd as nl
    L = capi.load()
    if capi.device_count() == 0:
        with pytest.raises(capi.NlError) as e:
            nl.StackHandle(4, 8, 8)
        assert "no HIP device" in str(e.value) or "hipGetDeviceCount" in str(e.value)
    out = np.full(16, np.float32(-7.5))
    low, high = np.full(16, 0xABCD, np.uint16), np.full(16, 0x1234, np.uint16)
    cl, ch = C.c_int64(-3), C.c_int64(-4)
    rc = getattr(L, entry)(None, mode, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch),
                           low.ctypes.data_as(C.POINTER(C.c_uint16)), high.ctypes.data_as(C.POINTER(C.c_uint16)))
    assert rc == capi.ERR_INVALID_ARG, entry
    assert np.all(out == np.float32(-7.5)) and np.all(low == 0xABCD) and np.all(high == 0x1234), entry
    assert (cl.value, ch.value) == (-3, -4), entry
