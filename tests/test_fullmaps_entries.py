"""The entries of the full maps pass: include/nlstack_fullmaps.h (part of the interface nlstack.h includes) declares exactly
capi.FULLMAPS_EXPORTS, the library exports them, they are no entry of another list, they take the arguments of the entries
they stand beside (nl_stack_run_maps / nl_group_run_maps), every argument check that ends in front of the device gives
that entry's code and message, and no entry gives a result where no handle can be made.  In the form of
tests/test_maps_entries.py, whose recorded tables stay as they are."""
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
STACK, GROUP = "nl_stack_run_maps_full", "nl_group_run_maps_full"


def _i64():
    return C.byref(C.c_int64(0))


U16 = np.zeros(16, np.uint16)
u16 = U16.ctypes.data_as(C.POINTER(C.c_uint16))
F32 = np.zeros(16, np.float32)

# (row id, entry, the existing entry that gives the expected code and message, call(L, entry name) -> return code)
ROWS = [
    ("run_maps_full/null-handle", STACK, "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 4, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_full/null-handle+bad-mode", STACK, "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_full/null-group", GROUP, "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 4, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_full/null-group+null-outputs", GROUP, "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 0, 2.0, 2.5, 0.0, None, None, None, None, None)),
]
EXPECTED = {
    "run_maps_full/null-handle": (-6, "null handle"),
    "run_maps_full/null-handle+bad-mode": (-6, "null handle"),
    "group_run_maps_full/null-group": (-6, "null group"),
    "group_run_maps_full/null-group+null-outputs": (-6, "null group"),
}
WORDS = ("When the MAD engines run.", "Maps.", "Result.", "The median.", "Everything else.", "Kernel name.",
         "stack_mad_fast_kernel", "stack_mad_bitonic_kernel", "stack_mad_ml_kernel", "nl_stack_set_exact",
         "NL_ERR_INVALID_MODE", "NL_ERR_WEIGHTED_MAD", "NL_ERR_TOO_MANY_FRAMES", "1e-6")
OTHERS = ("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "RESIDENTMAPS_EXPORTS", "DEEPMAPS_EXPORTS",
          "WLINFIT_EXPORTS", "WCLIP_EXPORTS", "WMAD_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS")


def _uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, header)).read(), flags=re.S)


def test_header_exports_and_binding_agree():
    raw = open(os.path.join(INC, "nlstack_fullmaps.h")).read()
    text = _uncommented("nlstack_fullmaps.h")
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.FULLMAPS_EXPORTS) == sorted([STACK, GROUP])
    assert not set(declared) & set(sum((getattr(capi, name) for name in OTHERS), []))
    assert '#include "nlstack_fullmaps.h"' in open(os.path.join(INC, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the maps are uint16, and the entries take the arguments of the entries they stand beside
    assert len(re.findall(r"uint16_t \*", text)) == 4
    maps = _uncommented("nlstack_maps.h")
    proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
    for name in ("nl_stack_run_maps", "nl_group_run_maps"):
        assert proto(text, name + "_full") == proto(maps, name)
    for word in WORDS:
        assert word in raw, word


def test_build_checks_the_list():
    import __graft_entry__ as entry
    assert "capi.FULLMAPS_EXPORTS" in inspect.getsource(entry.build)


def test_python_layer_has_both_methods():
    from nightlight_amd import stack
    handle, group = inspect.signature(stack.StackHandle.run_maps_full), inspect.signature(stack.StackGroup.run_maps_full)
    assert list(handle.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc", "out", "reject_low", "reject_high"]
    assert list(group.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc"]
    L = capi.load()
    assert L.nl_stack_run_maps_full.argtypes == L.nl_stack_run_maps.argtypes
    assert L.nl_group_run_maps_full.argtypes == L.nl_group_run_maps.argtypes


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
    assert {r[1] for r in ROWS} == set(capi.FULLMAPS_EXPORTS)
    ids = [r[0] for r in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call, entry) for rid, entry, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # ... which is what the existing entry gives for the same arguments
    assert {rid: run_row(L, call, existing) for rid, _, existing, call in ROWS} == got


@pytest.mark.parametrize("entry", [STACK, GROUP])
def test_no_cpu_result_where_no_handle_can_be_made(entry):
    """as every maps entry: no handle, NL_ERR_INVALID_ARG, the outputs untouched -- never a result of the CPU"""
    L = capi.load()
    out = np.full(16, np.float32(-7.5))
    low, high = np.full(16, 0xABCD, np.uint16), np.full(16, 0x1234, np.uint16)
    cl, ch = C.c_int64(-3), C.c_int64(-4)
    rc = getattr(L, entry)(None, 4, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch),
                           low.ctypes.data_as(C.POINTER(C.c_uint16)), high.ctypes.data_as(C.POINTER(C.c_uint16)))
    assert rc == capi.ERR_INVALID_ARG, entry
    assert np.all(out == np.float32(-7.5)) and np.all(low == 0xABCD) and np.all(high == 0x1234), entry
    assert (cl.value, ch.value) == (-3, -4), entry
