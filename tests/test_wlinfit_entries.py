"""The entries of the weighted linear-fit pass: include/nlstack_wlinfit.h (part of the interface nlstack.h includes)
declares exactly capi.WLINFIT_EXPORTS, the library exports them, every argument check that ends in front of the device
gives its code and message (a characterisation table in the form of tests/test_maps_entries.py), and the host
operator's JSON carries the switch only when it is set."""
import ctypes as C
import json
import os
import re

import numpy as np

from nightlight_amd import capi
from nightlight_amd import operator as host_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_wlinfit.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.WLINFIT_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.ALIGN_EXPORTS)
    assert '#include "nlstack_wlinfit.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is and carries the definition
    assert "EXTENSION" in raw and "Definition." in raw and "num += v_k * w_k" in raw


def _i64():
    return C.byref(C.c_int64(0))


F32 = np.zeros(16, np.float32)

# (row id, entry, call(L) -> return code)
ROWS = [
    ("run/null-handle", "nl_stack_run_linfit_weighted",
     lambda L: L.nl_stack_run_linfit_weighted(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("run/null-handle+null-outputs", "nl_stack_run_linfit_weighted",
     lambda L: L.nl_stack_run_linfit_weighted(None, 2.0, 2.5, 0.0, None, None, None)),
    ("run_async/null-handle", "nl_stack_run_linfit_weighted_async",
     lambda L: L.nl_stack_run_linfit_weighted_async(None, 2.0, 2.5, 0.0)),
    ("group_run/null-group", "nl_group_run_linfit_weighted",
     lambda L: L.nl_group_run_linfit_weighted(None, 2.0, 2.5, 0.0, f(F32), _i64(), _i64())),
    ("group_run/null-group+null-outputs", "nl_group_run_linfit_weighted",
     lambda L: L.nl_group_run_linfit_weighted(None, 2.0, 2.5, 0.0, None, None, None)),
]

EXPECTED = {
    "run/null-handle": (-6, "null handle"),
    "run/null-handle+null-outputs": (-6, "null handle"),
    "run_async/null-handle": (-6, "null handle"),
    "group_run/null-group": (-6, "null group"),
    "group_run/null-group+null-outputs": (-6, "null group"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.WLINFIT_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_operator_json_carries_the_switch_only_when_set():
    plain = host_op.op_stack_roundtrip_json('{"type":"stack"}')
    assert plain == '{"type":"stack","mode":6,"weighting":0,"sigmaLow":2.75,"sigmaHigh":2.75}'       # exactly as before
    full = '{"type":"stack","mode":5,"weighting":2,"sigmaLow":2.75,"sigmaHigh":3}'
    assert host_op.op_stack_roundtrip_json(full) == full
    assert "weightedLinearFit" not in host_op.op_stack_roundtrip_json('{"type":"stack","weightedLinearFit":false}')
    on = host_op.op_stack_roundtrip_json('{"type":"stack","mode":5,"weighting":2,"weightedLinearFit":true}')
    assert json.loads(on) == {"type": "stack", "mode": 5, "weighting": 2, "sigmaLow": 2.75, "sigmaHigh": 2.75,
                              "weightedLinearFit": True}
    assert host_op.op_stack_roundtrip_json(on) == on
