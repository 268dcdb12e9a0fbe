"""The entries of the deep maps pass: include/nlstack_deepmaps.h (part of the interface nlstack.h includes) declares
exactly capi.DEEPMAPS_EXPORTS, the library exports them, they are no entry of another list, and every argument check
that ends in front of the device gives the code and message of the entry it stands beside (nl_stack_run_maps /
nl_group_run_maps): a characterisation table in the form of tests/test_deepmaps_entries.py."""
import ctypes as C
import inspect
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
    raw = open(os.path.join(inc, "nlstack_deepmaps.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.DEEPMAPS_EXPORTS) == ["nl_group_run_maps_deep", "nl_stack_run_maps_deep"]
    others = (capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.FASTMAPS_EXPORTS + capi.RESIDENTMAPS_EXPORTS +
              capi.WLINFIT_EXPORTS + capi.WCLIP_EXPORTS + capi.ALIGN_EXPORTS + capi.RESAMPLE_EXPORTS)
    assert not set(declared) & set(others)
    assert '#include "nlstack_deepmaps.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the arguments of the entries they stand beside, and the maps are uint16
    assert len(re.findall(r"uint16_t \*", text)) == 4
    maps = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nlstack_maps.h")).read(), flags=re.S)
    for name in ("nl_stack_run_maps", "nl_group_run_maps"):
        proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
        assert proto(text, name + "_deep") == proto(maps, name)
    # the contract is in the header's comment
    for word in ("When the deep engines run.", "Maps.", "Result.", "Everything else.", "Kernel name.",
                 "stack_sigma_mlz_kernel", "nl_stack_set_exact", "NL_ERR_INVALID_MODE", "NL_ERR_WEIGHTED_MAD",
                 "NL_ERR_TOO_MANY_FRAMES", "1e-6", "Out of scope"):
        assert word in raw, word


def test_python_layer_has_both_methods():
    from nightlight_amd import stack
    handle, group = inspect.signature(stack.StackHandle.run_maps_deep), inspect.signature(stack.StackGroup.run_maps_deep)
    assert list(handle.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc", "out", "reject_low", "reject_high"]
    assert list(group.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc"]
    # run_maps and its switch are what they were
    for cls in (stack.StackHandle, stack.StackGroup):
        assert inspect.signature(cls.run_maps).parameters["fast"].default is False
    # the binding gives both entries the argument types of the entries they stand beside
    L = capi.load()
    assert L.nl_stack_run_maps_deep.argtypes == L.nl_stack_run_maps.argtypes
    assert L.nl_group_run_maps_deep.argtypes == L.nl_group_run_maps.argtypes


def _i64():
    return C.byref(C.c_int64(0))


U16 = np.zeros(16, np.uint16)
u16 = U16.ctypes.data_as(C.POINTER(C.c_uint16))
F32 = np.zeros(16, np.float32)

# (row id, entry, call(L, entry name) -> return code, the existing entry that gives the expected code and message)
ROWS = [
    ("run_maps_deep/null-handle", "nl_stack_run_maps_deep", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_deep/null-handle+bad-mode", "nl_stack_run_maps_deep", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_deep/null-group", "nl_group_run_maps_deep", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_deep/null-group+null-outputs", "nl_group_run_maps_deep", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 3, 2.0, 2.5, 0.0, None, None, None, None, None)),
]

EXPECTED = {
    "run_maps_deep/null-handle": (-6, "null handle"),
    "run_maps_deep/null-handle+bad-mode": (-6, "null handle"),
    "group_run_maps_deep/null-group": (-6, "null group"),
    "group_run_maps_deep/null-group+null-outputs": (-6, "null group"),
}


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
    assert {entry for _, entry, _, _ in ROWS} == set(capi.DEEPMAPS_EXPORTS)
    ids = [rid for rid, _, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call, entry) for rid, entry, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # ... which is what the existing entry gives for the same arguments
    beside = {rid: run_row(L, call, existing) for rid, _, existing, call in ROWS}
    assert got == beside


def test_no_cpu_result_where_no_handle_can_be_made():
    """A pass needs a handle, and a handle needs a device: where none is visible the deep entries end as
    nl_stack_run_maps does -- no handle, NL_ERR_INVALID_ARG, the outputs untouched -- never with a result of the CPU."""
    import nightlight_amd as nl
    L = capi.load()
    if capi.device_count() == 0:
        with pytest.raises(capi.NlError) as e:
            nl.StackHandle(4, 8, 8)
        assert "no HIP device" in str(e.value) or "hipGetDeviceCount" in str(e.value)
        with pytest.raises(capi.NlError):
            nl.StackGroup(4, 8, 8)
    for entry in ("nl_stack_run_maps", "nl_stack_run_maps_deep", "nl_group_run_maps", "nl_group_run_maps_deep"):
        out = np.full(16, np.float32(-7.5))
        low, high = np.full(16, 0xABCD, np.uint16), np.full(16, 0x1234, np.uint16)
        cl, ch = C.c_int64(-3), C.c_int64(-4)
        rc = getattr(L, entry)(None, 2, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch),
                               low.ctypes.data_as(C.POINTER(C.c_uint16)), high.ctypes.data_as(C.POINTER(C.c_uint16)))
        assert rc == capi.ERR_INVALID_ARG, entry
        assert np.all(out == np.float32(-7.5)) and np.all(low == 0xABCD) and np.all(high == 0x1234), entry
        assert (cl.value, ch.value) == (-3, -4), entry
