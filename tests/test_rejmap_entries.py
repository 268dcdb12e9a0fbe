"""The map entries of the C ABI: include/nlstack_maps.h (the part of the interface nlstack.h includes) declares exactly
capi.MAPS_EXPORTS, the library exports them, and every argument check that ends in front of the device gives its code
and message: a characterisation table in the form of tests/test_locscale_entries.py."""
import ctypes as C
import os
import re

import numpy as np

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nlstack_maps.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.MAPS_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.ALIGN_EXPORTS)
    assert '#include "nlstack_maps.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the four entries the interface is about, and the maps are uint16
    assert {"nl_stack_run_maps", "nl_stack_coverage", "nl_group_run_maps", "nl_group_coverage"} <= set(declared)
    assert len(re.findall(r"uint16_t \*", text)) == 6


def _i64():
    return C.byref(C.c_int64(0))


U16 = np.zeros(16, np.uint16)
u16 = U16.ctypes.data_as(C.POINTER(C.c_uint16))
F32 = np.zeros(16, np.float32)

# (row id, entry, call(L) -> return code)
ROWS = [
    ("run_maps/null-handle", "nl_stack_run_maps",
     lambda L: L.nl_stack_run_maps(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps/null-handle+bad-mode", "nl_stack_run_maps",
     lambda L: L.nl_stack_run_maps(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("coverage/null-handle", "nl_stack_coverage", lambda L: L.nl_stack_coverage(None, u16)),
    ("coverage/null-handle+null-output", "nl_stack_coverage", lambda L: L.nl_stack_coverage(None, None)),
    ("last_coverage_ms/null-handle", "nl_stack_last_coverage_ms", lambda L: int(L.nl_stack_last_coverage_ms(None))),
    ("group_run_maps/null-group", "nl_group_run_maps",
     lambda L: L.nl_group_run_maps(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_coverage/null-group", "nl_group_coverage", lambda L: L.nl_group_coverage(None, u16)),
    ("group_coverage/null-group+null-output", "nl_group_coverage", lambda L: L.nl_group_coverage(None, None)),
]

EXPECTED = {
    "run_maps/null-handle": (-6, "null handle"),
    "run_maps/null-handle+bad-mode": (-6, "null handle"),
    "coverage/null-handle": (-6, "null handle"),
    "coverage/null-handle+null-output": (-6, "null handle"),
    "last_coverage_ms/null-handle": (-1, SENTINEL),          # no timing, and the thread's error stays as it was
    "group_run_maps/null-group": (-6, "null group"),
    "group_coverage/null-group": (-6, "null group"),
    "group_coverage/null-group+null-output": (-6, "null group"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.MAPS_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
