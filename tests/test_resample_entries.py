"""The entries of the bicubic / Lanczos-3 resampling: include/nlstack_resample.h (part of the interface nlstack.h
includes) declares exactly capi.RESAMPLE_EXPORTS, the library exports them, every argument check that ends in front of
the device gives its code and message (a characterisation table in the form of tests/test_wlinfit_entries.py), and the
table entry works without a device.

The _resample_from entries check what needs no handle -- the kernel's id, a null or singular transform -- in front of
their handles, so every row below runs on a machine without a device."""
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
    raw = open(os.path.join(inc, "nlstack_resample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.RESAMPLE_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.WLINFIT_EXPORTS +
                                   capi.ALIGN_EXPORTS)
    assert '#include "nlstack_resample.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is, carries the definition and the constants the binding repeats
    assert "EXTENSION" in raw and "Definition." in raw and "w1 = (1.5f*t - 2.5f)*t*t + 1" in raw
    consts = dict(re.findall(r"#define (NL_RS_[A-Z0-9]+) (\d+)", text))
    assert consts == {"NL_RS_BILINEAR": str(capi.RS_BILINEAR), "NL_RS_BICUBIC": str(capi.RS_BICUBIC),
                      "NL_RS_LANCZOS3": str(capi.RS_LANCZOS3), "NL_RS_PHASES": str(capi.RS_PHASES)}


def test_python_surface():
    import nightlight_amd as nl
    for cls in (nl.StackHandle, nl.StackGroup):
        assert callable(getattr(cls, "frame_resample_from", None))
    assert callable(getattr(nl.StackHandle, "resample_tile_paths", None)) and callable(nl.lanczos3_table)


def _i64():
    return C.byref(C.c_int64(0))


T6 = np.array([1, 0, 0.5, 0, 1, 0.25], np.float32)
T6_SINGULAR = np.array([1, 2, 0, 2, 4, 0], np.float32)
LANCZOS3 = capi.RS_LANCZOS3

# (row id, entry, call(L) -> return code); every handle is null: there is no device to make one on
ROWS = [
    ("table/null-table", "nl_resample_lanczos3_table", lambda L: L.nl_resample_lanczos3_table(None)),
    ("frame/null-handles", "nl_stack_frame_resample_from",
     lambda L: L.nl_stack_frame_resample_from(None, 0, None, 0, f(T6), 0.0, LANCZOS3, 0)),
    ("frame/null-transform", "nl_stack_frame_resample_from",
     lambda L: L.nl_stack_frame_resample_from(None, 0, None, 0, None, 0.0, LANCZOS3, 0)),
    ("frame/kernel-3", "nl_stack_frame_resample_from",
     lambda L: L.nl_stack_frame_resample_from(None, 0, None, 0, f(T6), 0.0, 3, 0)),
    ("frame/kernel--1", "nl_stack_frame_resample_from",
     lambda L: L.nl_stack_frame_resample_from(None, 0, None, 0, f(T6), 0.0, -1, 1)),
    ("frame/singular", "nl_stack_frame_resample_from",
     lambda L: L.nl_stack_frame_resample_from(None, 0, None, 0, f(T6_SINGULAR), 0.0, capi.RS_BICUBIC, 0)),
    ("group/null-group", "nl_group_frame_resample_from",
     lambda L: L.nl_group_frame_resample_from(None, 0, None, 0, f(T6), 0.0, LANCZOS3, 0)),
    ("group/null-transform", "nl_group_frame_resample_from",
     lambda L: L.nl_group_frame_resample_from(None, 0, None, 0, None, 0.0, LANCZOS3, 0)),
    ("group/kernel-7", "nl_group_frame_resample_from",
     lambda L: L.nl_group_frame_resample_from(None, 0, None, 0, f(T6), 0.0, 7, 0)),
    ("group/singular", "nl_group_frame_resample_from",
     lambda L: L.nl_group_frame_resample_from(None, 0, None, 0, f(T6_SINGULAR), 0.0, LANCZOS3, 1)),
    ("tile_paths/null-handles", "nl_stack_resample_tile_paths",
     lambda L: L.nl_stack_resample_tile_paths(None, None, 0, f(T6), LANCZOS3, _i64(), _i64())),
    ("tile_paths/null-transform+kernel-9", "nl_stack_resample_tile_paths",
     lambda L: L.nl_stack_resample_tile_paths(None, None, 0, None, 9, _i64(), _i64())),
]

KERNELS = "(NL_RS_BILINEAR 0, NL_RS_BICUBIC 1, NL_RS_LANCZOS3 2)"
EXPECTED = {
    "table/null-table": (-6, "resample_lanczos3_table: null table"),
    "frame/null-handles": (-6, "frame_resample_from: null handle"),
    "frame/null-transform": (-6, "frame_resample_from: null transform"),
    "frame/kernel-3": (-6, "frame_resample_from: unknown kernel 3 " + KERNELS),
    "frame/kernel--1": (-6, "frame_resample_from: unknown kernel -1 " + KERNELS),
    "frame/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "group/null-group": (-6, "group_frame_resample_from: null group"),
    "group/null-transform": (-6, "group_frame_resample_from: null transform"),
    "group/kernel-7": (-6, "group_frame_resample_from: unknown kernel 7 " + KERNELS),
    "group/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "tile_paths/null-handles": (-6, "resample_tile_paths: null argument"),
    "tile_paths/null-transform+kernel-9": (-6, "resample_tile_paths: null argument"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.RESAMPLE_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_the_table_needs_no_device():
    import nightlight_amd as nl
    a, b = nl.lanczos3_table(), nl.lanczos3_table()
    assert a.shape == (capi.RS_PHASES, 6) and a.dtype == np.float32 and np.array_equal(a, b)
    assert a[0].tolist() == [0, 0, 1, 0, 0, 0]
    half = a[capi.RS_PHASES // 2]
    assert np.array_equal(half, half[::-1]) and half[2] > 0.6 and half[1] < 0 < half[0]     # symmetric at phase 1/2
