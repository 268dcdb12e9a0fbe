"""The entries of the drizzle integration: include/nlstack_drizzle.h (part of the interface nlstack.h includes) declares
exactly capi.DRIZZLE_EXPORTS, the library exports them, every argument check that ends in front of the device gives its
code and message (a characterisation table in the form of tests/test_resample_entries.py), and the geometry entry,
which needs no device, equals the numpy double formula bit for bit after rounding.

nl_stack_frame_drizzle_from checks what needs no handle -- the transform, the kernel's id, the weight, the whole
geometry -- in front of its handles, and nl_stack_frame_reject_against its thresholds, so every row below runs on a
machine without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import drizzle_ref as ref
from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr
f32 = np.float32


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_drizzle.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.DRIZZLE_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.WLINFIT_EXPORTS +
                                   capi.ALIGN_EXPORTS + capi.RESAMPLE_EXPORTS)
    assert '#include "nlstack_drizzle.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is, carries the definition and the constants the binding repeats
    assert "EXTENSION" in raw and "Definition." in raw
    assert "R = (int)ceil( max((|Ga|+|Gb|)*reach, (|Gd|+|Ge|)*reach) + 0.5 + 1.0/64 )" in raw
    consts = dict(re.findall(r"#define (NL_DZ_[A-Z0-9_]+) (\d+)", text))
    assert consts == {"NL_DZ_TURBO": str(capi.DZ_TURBO), "NL_DZ_POINT": str(capi.DZ_POINT),
                      "NL_DZ_MAX_RADIUS": str(capi.DZ_MAX_RADIUS)}
    assert (ref.TURBO, ref.POINT, ref.MAX_RADIUS) == (capi.DZ_TURBO, capi.DZ_POINT, capi.DZ_MAX_RADIUS)
    # out of scope, said where a caller reads it
    assert "nl_group_" in raw and "rotated-square" in raw and "Go shim" in raw


def test_python_surface():
    import nightlight_amd as nl
    for name in ("frame_drizzle_from", "drizzle_finalize", "frame_reject_against", "drizzle_tile_paths"):
        assert callable(getattr(nl.StackHandle, name, None)), name
    assert callable(nl.drizzle_geometry)
    assert (nl.DZ_TURBO, nl.DZ_POINT, nl.DZ_MAX_RADIUS) == (0, 1, 3)


def _i64():
    return C.byref(C.c_int64(0))


T6 = np.array([1, 0, 0.5, 0, 1, 0.25], f32)
T6_SINGULAR = np.array([1, 2, 0, 2, 4, 0], f32)
T6_NAN = np.array([1, 0, np.nan, 0, 1, 0], f32)
T6_HUGE = np.array([1e30, 0, 0, 0, 1e30, 0], f32)                       # S * a overflows fp32 at S = 1e30
T6_R4 = ref.R4[1](67, 35)
NAN, INF = float("nan"), float("inf")


def _geometry(trans, scale, pixfrac, null=None):
    def call(L):
        F, G, hw, R = np.zeros(6, f32), np.zeros(6, f32), C.c_float(0), C.c_int(0)
        args = [None if trans is None else f(trans), scale, pixfrac, f(F), f(G), C.byref(hw), C.byref(R)]
        if null is not None:
            args[null] = None
        return L.nl_drizzle_geometry(*args)
    return call


def _from(trans, scale=2.0, pixfrac=1.0, weight=1.0, kernel=capi.DZ_TURBO):
    return lambda L: L.nl_stack_frame_drizzle_from(None, 0, 1, None, 0, None if trans is None else f(trans), scale,
                                                   pixfrac, weight, 1, kernel)


# (row id, entry, call(L) -> return code); every handle is null: there is no device to make one on
ROWS = [
    ("geometry/null-transform", "nl_drizzle_geometry", _geometry(None, 2.0, 1.0)),
    ("geometry/null-radius", "nl_drizzle_geometry", _geometry(T6, 2.0, 1.0, null=6)),
    ("geometry/null-half-width", "nl_drizzle_geometry", _geometry(T6, 2.0, 1.0, null=5)),
    ("geometry/scale-0", "nl_drizzle_geometry", _geometry(T6, 0.0, 1.0)),
    ("geometry/scale-negative", "nl_drizzle_geometry", _geometry(T6, -2.0, 1.0)),
    ("geometry/scale-inf", "nl_drizzle_geometry", _geometry(T6, INF, 1.0)),
    ("geometry/scale-nan", "nl_drizzle_geometry", _geometry(T6, NAN, 1.0)),
    ("geometry/pixfrac-0", "nl_drizzle_geometry", _geometry(T6, 2.0, 0.0)),
    ("geometry/pixfrac-above-1", "nl_drizzle_geometry", _geometry(T6, 2.0, 1.5)),
    ("geometry/pixfrac-nan", "nl_drizzle_geometry", _geometry(T6, 2.0, NAN)),
    ("geometry/singular", "nl_drizzle_geometry", _geometry(T6_SINGULAR, 2.0, 1.0)),
    ("geometry/nan-coefficient", "nl_drizzle_geometry", _geometry(T6_NAN, 2.0, 1.0)),
    ("geometry/overflow", "nl_drizzle_geometry", _geometry(T6_HUGE, 1e30, 1.0)),
    ("geometry/radius-4", "nl_drizzle_geometry", _geometry(T6_R4, 1.0, 1.0)),
    ("from/null-transform", "nl_stack_frame_drizzle_from", _from(None)),
    ("from/kernel-2", "nl_stack_frame_drizzle_from", _from(T6, kernel=2)),
    ("from/kernel--1", "nl_stack_frame_drizzle_from", _from(T6, kernel=-1)),
    ("from/weight-0", "nl_stack_frame_drizzle_from", _from(T6, weight=0.0)),
    ("from/weight-negative", "nl_stack_frame_drizzle_from", _from(T6, weight=-1.0)),
    ("from/weight-inf", "nl_stack_frame_drizzle_from", _from(T6, weight=INF)),
    ("from/weight-nan", "nl_stack_frame_drizzle_from", _from(T6, weight=NAN)),
    ("from/scale-0", "nl_stack_frame_drizzle_from", _from(T6, scale=0.0)),
    ("from/pixfrac-2", "nl_stack_frame_drizzle_from", _from(T6, pixfrac=2.0)),
    ("from/singular", "nl_stack_frame_drizzle_from", _from(T6_SINGULAR)),
    ("from/nan-coefficient", "nl_stack_frame_drizzle_from", _from(T6_NAN)),
    ("from/radius-4", "nl_stack_frame_drizzle_from", _from(T6_R4, scale=1.0)),
    ("from/null-handles", "nl_stack_frame_drizzle_from", _from(T6)),
    ("finalize/null-handle", "nl_stack_drizzle_finalize", lambda L: L.nl_stack_drizzle_finalize(None, 0, 1, 2, 0.0, NAN)),
    ("reject/low-negative", "nl_stack_frame_reject_against",
     lambda L: L.nl_stack_frame_reject_against(None, 0, 1, -1.0, 1.0, _i64(), _i64())),
    ("reject/high-nan", "nl_stack_frame_reject_against",
     lambda L: L.nl_stack_frame_reject_against(None, 0, 1, 1.0, NAN, _i64(), _i64())),
    ("reject/null-handle", "nl_stack_frame_reject_against",
     lambda L: L.nl_stack_frame_reject_against(None, 0, 1, 1.0, 1.0, _i64(), _i64())),
    ("tile_paths/null-handles", "nl_stack_drizzle_tile_paths",
     lambda L: L.nl_stack_drizzle_tile_paths(None, None, 0, f(T6), 2.0, 1.0, _i64(), _i64())),
    ("tile_paths/null-transform", "nl_stack_drizzle_tile_paths",
     lambda L: L.nl_stack_drizzle_tile_paths(None, None, 0, None, 2.0, 1.0, _i64(), _i64())),
]

KERNELS = "(NL_DZ_TURBO 0, NL_DZ_POINT 1)"
RADIUS_4 = ": window radius 4 beyond NL_DZ_MAX_RADIUS 3 (the output grid is too coarse for this frame)"
EXPECTED = {
    "geometry/null-transform": (-6, "drizzle_geometry: null argument"),
    "geometry/null-radius": (-6, "drizzle_geometry: null argument"),
    "geometry/null-half-width": (-6, "drizzle_geometry: null argument"),
    "geometry/scale-0": (-6, "drizzle_geometry: scale 0 (a finite number > 0)"),
    "geometry/scale-negative": (-6, "drizzle_geometry: scale -2 (a finite number > 0)"),
    "geometry/scale-inf": (-6, "drizzle_geometry: scale inf (a finite number > 0)"),
    "geometry/scale-nan": (-6, "drizzle_geometry: scale nan (a finite number > 0)"),
    "geometry/pixfrac-0": (-6, "drizzle_geometry: pixfrac 0 (0 < pixfrac <= 1)"),
    "geometry/pixfrac-above-1": (-6, "drizzle_geometry: pixfrac 1.5 (0 < pixfrac <= 1)"),
    "geometry/pixfrac-nan": (-6, "drizzle_geometry: pixfrac nan (0 < pixfrac <= 1)"),
    "geometry/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "geometry/nan-coefficient": (-6, "drizzle_geometry: a coefficient of the geometry is not finite"),
    "geometry/overflow": (-6, "drizzle_geometry: a coefficient of the geometry is not finite"),
    "geometry/radius-4": (-6, "drizzle_geometry" + RADIUS_4),
    "from/null-transform": (-6, "frame_drizzle_from: null transform"),
    "from/kernel-2": (-6, "frame_drizzle_from: unknown kernel 2 " + KERNELS),
    "from/kernel--1": (-6, "frame_drizzle_from: unknown kernel -1 " + KERNELS),
    "from/weight-0": (-6, "frame_drizzle_from: weight 0 (a finite number > 0)"),
    "from/weight-negative": (-6, "frame_drizzle_from: weight -1 (a finite number > 0)"),
    "from/weight-inf": (-6, "frame_drizzle_from: weight inf (a finite number > 0)"),
    "from/weight-nan": (-6, "frame_drizzle_from: weight nan (a finite number > 0)"),
    "from/scale-0": (-6, "frame_drizzle_from: scale 0 (a finite number > 0)"),
    "from/pixfrac-2": (-6, "frame_drizzle_from: pixfrac 2 (0 < pixfrac <= 1)"),
    "from/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "from/nan-coefficient": (-6, "frame_drizzle_from: a coefficient of the geometry is not finite"),
    "from/radius-4": (-6, "frame_drizzle_from" + RADIUS_4),
    "from/null-handles": (-6, "frame_drizzle_from: null handle"),
    "finalize/null-handle": (-6, "null handle"),
    "reject/low-negative": (-6, "frame_reject_against: low -1, high 1 (absolute thresholds >= 0)"),
    "reject/high-nan": (-6, "frame_reject_against: low 1, high nan (absolute thresholds >= 0)"),
    "reject/null-handle": (-6, "null handle"),
    "tile_paths/null-handles": (-6, "drizzle_tile_paths: null argument"),
    "tile_paths/null-transform": (-6, "drizzle_tile_paths: null argument"),
}


def run_row(L, call):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, f32)
    assert L.nl_weights_from_scalars(7, f(w), 1, f(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


def test_every_entry_has_a_row():
    assert {entry for _, entry, _ in ROWS} == set(capi.DRIZZLE_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def _all_transforms():
    out = []
    for (w, h), _, S in ref.SHAPES:
        for name, make in ref.TRANSFORMS.items():
            for p in (0.5, 0.7, 0.9, 1.0):
                out.append((make(w, h), S, p))
    out.append((ref.R3[1](67, 35), ref.R3[2], ref.R3[3]))
    out.append((ref.R1[1](67, 35), ref.R1[2], ref.R1[3]))
    for deg in (0, 13, 30, 45, 90, 180):
        for mag in (0.97, 1.0, 1.02):
            for S in (1.0, 1.5, 2.0, 3.0):
                out.append((ref.rotation(23, 17, deg, mag, 0.31, -0.17), S, 0.7))
    return out


def test_the_geometry_equals_the_double_formula_bit_for_bit():
    import nightlight_amd as nl
    radii = set()
    for trans, S, p in _all_transforms():
        F, G, hw, R = nl.drizzle_geometry(trans, S, p)
        Fd, Gd, hwd, span = ref.geometry_double(trans, S, p)
        assert F.dtype == f32 and G.dtype == f32
        assert np.array_equal(F.view(np.uint32), Fd.astype(f32).view(np.uint32))
        assert np.array_equal(G.view(np.uint32), Gd.astype(f32).view(np.uint32))
        assert f32(hw).view(np.uint32) == f32(hwd).view(np.uint32) and R == math.ceil(span)
        rF, rG, rhw, rR = ref.geometry(trans, S, p)
        assert np.array_equal(rF, F) and np.array_equal(rG, G) and rhw == hw and rR == R
        radii.add(R)
    assert radii == {1, 2, 3}


def test_the_geometry_errors_of_the_restatement_are_the_entry_s():
    import nightlight_amd as nl
    for trans, S, p in ((T6_SINGULAR, 2.0, 1.0), (T6_NAN, 2.0, 1.0), (T6_HUGE, 1e30, 1.0), (T6_R4, 1.0, 1.0),
                        (T6, 0.0, 1.0), (T6, INF, 1.0), (T6, 2.0, 0.0), (T6, 2.0, 1.5), (T6, 2.0, NAN)):
        with pytest.raises(ref.GeometryError):
            ref.geometry(trans, S, p)
        with pytest.raises(nl.NlError) as e:
            nl.drizzle_geometry(trans, S, p)
        assert e.value.code == capi.ERR_INVALID_ARG
