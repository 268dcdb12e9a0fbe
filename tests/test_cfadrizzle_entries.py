"""The entries of the CFA drizzle: include/nlstack_cfadrizzle.h (part of the interface nlstack.h includes) declares
exactly capi.CFADRIZZLE_EXPORTS, the library exports them, every argument check that ends in front of the device gives
its code and message (the form of tests/test_drizzle_entries.py), and the transform entry, which needs no device, equals
the double formula bit for bit after its one rounding.

nl_stack_frame_drizzle_cfa_from runs the mono entry's checks in its order under its own name, with the channel and the
CFA directly behind the kernel and the weight; nl_stack_frame_reject_against_cfa checks its thresholds and names in
front of its handle.  nl_stack_frame_badpixel_cfa asks for the device first, as nl_stack_upload_frame_cfa does: without
one it is NL_ERR_NO_DEVICE, with one its null handle is refused."""
import ctypes as C
import os
import re

import numpy as np

import cfadrizzle_ref as cref
import drizzle_ref as ref
from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"
f = capi.fptr
f32 = np.float32


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    raw = open(os.path.join(inc, "nlstack_cfadrizzle.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.CFADRIZZLE_EXPORTS)
    others = (capi.EXPORTS + capi.LOCSCALE_EXPORTS + capi.MAPS_EXPORTS + capi.FASTMAPS_EXPORTS +
              capi.RESIDENTMAPS_EXPORTS + capi.DEEPMAPS_EXPORTS + capi.FULLMAPS_EXPORTS + capi.WLINFIT_EXPORTS +
              capi.WCLIP_EXPORTS + capi.WMAD_EXPORTS + capi.DEEPSTACK_EXPORTS + capi.DEEPSTACKMAPS_EXPORTS +
              capi.DEEPWMAD_EXPORTS + capi.ALIGN_EXPORTS + capi.RESAMPLE_EXPORTS + capi.DRIZZLE_EXPORTS)
    assert not set(declared) & set(others)
    top = open(os.path.join(inc, "nlstack.h")).read()
    assert '#include "nlstack_cfadrizzle.h"' in top
    assert top.index('#include "nlstack_drizzle.h"') < top.index('#include "nlstack_cfadrizzle.h"')
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the header says what it is and carries the definition, its consequence and what is out of scope
    assert "EXTENSION" in raw and "Definition." in raw
    for words in ("(i - xo) and (j - yo) are both even", "(i - xo) and (j - yo) are both odd", "(i - xo) + (j - yo) is odd",
                  "is skipped, as a NaN pixel is skipped", "whose other pixels are NaN",
                  "c' = c - a*xo - b*yo", "f' = f - d*xo - e*yo", "nl_group_", "pixfrac > 1", "Go shim"):
        assert words in raw, words


def test_python_surface():
    import nightlight_amd as nl
    for name in ("frame_drizzle_cfa_from", "frame_reject_against_cfa", "frame_badpixel_cfa"):
        assert callable(getattr(nl.StackHandle, name, None)), name
    assert callable(nl.drizzle_cfa_transform)


def _i64():
    return C.byref(C.c_int64(0))


T6 = np.array([1, 0, 0.5, 0, 1, 0.25], f32)
T6_SINGULAR = np.array([1, 2, 0, 2, 4, 0], f32)
T6_NAN = np.array([1, 0, np.nan, 0, 1, 0], f32)
T6_OVERFLOW = np.array([3e38, 3e38, -3e38, 0, 1, 0], f32)                    # c - a*xo - b*yo leaves fp32 for BGGR
T6_R4 = ref.R4[1](67, 35)
NAN, INF = float("nan"), float("inf")


def _transform(trans, cfa, null_out=False):
    def call(L):
        out = np.zeros(6, f32)
        return L.nl_drizzle_cfa_transform(None if trans is None else f(trans), cfa, None if null_out else f(out))
    return call


def _from(trans, scale=2.0, pixfrac=1.0, weight=1.0, kernel=capi.DZ_TURBO, channel=b"R", cfa=b"RGGB"):
    return lambda L: L.nl_stack_frame_drizzle_cfa_from(None, 0, 1, None, 0, None if trans is None else f(trans), scale,
                                                       pixfrac, weight, 1, kernel, channel, cfa)


def _reject(low=1.0, high=1.0, channel=b"R", cfa=b"RGGB"):
    return lambda L: L.nl_stack_frame_reject_against_cfa(None, 0, 1, channel, cfa, low, high, _i64(), _i64())


# (row id, entry, call(L) -> return code); every handle is null: there is no device to make one on
ROWS = [
    ("transform/null-in", "nl_drizzle_cfa_transform", _transform(None, b"RGGB")),
    ("transform/null-out", "nl_drizzle_cfa_transform", _transform(T6, b"RGGB", null_out=True)),
    ("transform/null-cfa", "nl_drizzle_cfa_transform", _transform(T6, None)),
    ("transform/empty-cfa", "nl_drizzle_cfa_transform", _transform(T6, b"")),
    ("transform/unknown-cfa", "nl_drizzle_cfa_transform", _transform(T6, b"RGBG")),
    ("transform/nan-in", "nl_drizzle_cfa_transform", _transform(T6_NAN, b"RGGB")),
    ("transform/overflow-out", "nl_drizzle_cfa_transform", _transform(T6_OVERFLOW, b"BGGR")),
    ("from/null-transform", "nl_stack_frame_drizzle_cfa_from", _from(None)),
    ("from/kernel-2", "nl_stack_frame_drizzle_cfa_from", _from(T6, kernel=2)),
    ("from/weight-0", "nl_stack_frame_drizzle_cfa_from", _from(T6, weight=0.0)),
    ("from/weight-nan", "nl_stack_frame_drizzle_cfa_from", _from(T6, weight=NAN)),
    ("from/null-channel", "nl_stack_frame_drizzle_cfa_from", _from(T6, channel=None)),
    ("from/empty-cfa", "nl_stack_frame_drizzle_cfa_from", _from(T6, cfa=b"")),
    ("from/unknown-cfa-and-channel", "nl_stack_frame_drizzle_cfa_from", _from(T6, channel=b"L", cfa=b"XTRANS")),
    ("from/unknown-channel", "nl_stack_frame_drizzle_cfa_from", _from(T6, channel=b"L", cfa=b"grbg")),
    ("from/names-before-geometry", "nl_stack_frame_drizzle_cfa_from", _from(T6, scale=0.0, cfa=b"RGBG")),
    ("from/weight-before-names", "nl_stack_frame_drizzle_cfa_from", _from(T6, weight=-1.0, cfa=b"RGBG")),
    ("from/scale-0", "nl_stack_frame_drizzle_cfa_from", _from(T6, scale=0.0)),
    ("from/pixfrac-2", "nl_stack_frame_drizzle_cfa_from", _from(T6, pixfrac=2.0)),
    ("from/singular", "nl_stack_frame_drizzle_cfa_from", _from(T6_SINGULAR)),
    ("from/nan-coefficient", "nl_stack_frame_drizzle_cfa_from", _from(T6_NAN)),
    ("from/radius-4", "nl_stack_frame_drizzle_cfa_from", _from(T6_R4, scale=1.0)),
    ("from/null-handles", "nl_stack_frame_drizzle_cfa_from", _from(T6, channel=b"b", cfa=b"bggr")),
    ("reject/low-negative", "nl_stack_frame_reject_against_cfa", _reject(low=-1.0)),
    ("reject/high-nan", "nl_stack_frame_reject_against_cfa", _reject(high=NAN)),
    ("reject/thresholds-before-names", "nl_stack_frame_reject_against_cfa", _reject(high=NAN, cfa=b"RGBG")),
    ("reject/null-cfa", "nl_stack_frame_reject_against_cfa", _reject(cfa=None)),
    ("reject/unknown-cfa", "nl_stack_frame_reject_against_cfa", _reject(cfa=b"RGBG")),
    ("reject/unknown-channel", "nl_stack_frame_reject_against_cfa", _reject(channel=b"RG")),
    ("reject/null-handle", "nl_stack_frame_reject_against_cfa", _reject()),
    ("badpixel/null-handle", "nl_stack_frame_badpixel_cfa",
     lambda L: L.nl_stack_frame_badpixel_cfa(None, 0, b"R", b"RGGB", 3.0, 5.0, _i64(), None)),
]

KERNELS = "(NL_DZ_TURBO 0, NL_DZ_POINT 1)"
WHO = "frame_drizzle_cfa_from"
EXPECTED = {
    "transform/null-in": (-6, "drizzle_cfa_transform: null argument"),
    "transform/null-out": (-6, "drizzle_cfa_transform: null argument"),
    "transform/null-cfa": (-6, "drizzle_cfa_transform: null argument"),
    "transform/empty-cfa": (-6, "drizzle_cfa_transform: null argument"),
    "transform/unknown-cfa": (-6, "Unknown CFA value RGBG"),
    "transform/nan-in": (-6, "drizzle_cfa_transform: a coefficient is not finite"),
    "transform/overflow-out": (-6, "drizzle_cfa_transform: a coefficient is not finite"),
    "from/null-transform": (-6, WHO + ": null transform"),
    "from/kernel-2": (-6, WHO + ": unknown kernel 2 " + KERNELS),
    "from/weight-0": (-6, WHO + ": weight 0 (a finite number > 0)"),
    "from/weight-nan": (-6, WHO + ": weight nan (a finite number > 0)"),
    "from/null-channel": (-6, WHO + " needs a channel and a CFA"),
    "from/empty-cfa": (-6, WHO + " needs a channel and a CFA"),
    "from/unknown-cfa-and-channel": (-6, "Unknown CFA value XTRANS"),
    "from/unknown-channel": (-6, "Unknown debayering value L"),
    "from/names-before-geometry": (-6, "Unknown CFA value RGBG"),
    "from/weight-before-names": (-6, WHO + ": weight -1 (a finite number > 0)"),
    "from/scale-0": (-6, WHO + ": scale 0 (a finite number > 0)"),
    "from/pixfrac-2": (-6, WHO + ": pixfrac 2 (0 < pixfrac <= 1)"),
    "from/singular": (-6, "Matrix has no inverse, epsilon=0"),
    "from/nan-coefficient": (-6, WHO + ": a coefficient of the geometry is not finite"),
    "from/radius-4": (-6, WHO + ": window radius 4 beyond NL_DZ_MAX_RADIUS 3 (the output grid is too coarse for this frame)"),
    "from/null-handles": (-6, WHO + ": null handle"),
    "reject/low-negative": (-6, "frame_reject_against_cfa: low -1, high 1 (absolute thresholds >= 0)"),
    "reject/high-nan": (-6, "frame_reject_against_cfa: low 1, high nan (absolute thresholds >= 0)"),
    "reject/thresholds-before-names": (-6, "frame_reject_against_cfa: low 1, high nan (absolute thresholds >= 0)"),
    "reject/null-cfa": (-6, "frame_reject_against_cfa needs a channel and a CFA"),
    "reject/unknown-cfa": (-6, "Unknown CFA value RGBG"),
    "reject/unknown-channel": (-6, "Unknown debayering value RG"),
    "reject/null-handle": (-6, "null handle"),
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
    assert {entry for _, entry, _ in ROWS} == set(capi.CFADRIZZLE_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED) | {"badpixel/null-handle"}


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, _, call in ROWS}
    # the bad-pixel step asks for the device first: NL_ERR_NO_DEVICE without one, else its null handle is refused
    code, msg = got.pop("badpixel/null-handle")
    if capi.device_count() == 0:
        assert code == capi.ERR_NO_DEVICE and msg != SENTINEL, (code, msg)
    else:
        assert (code, msg) == (-6, "null handle")
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_the_transform_equals_the_double_formula_bit_for_bit():
    import nightlight_amd as nl
    transforms = [make(67, 35) for make in ref.TRANSFORMS.values()] + [ref.R3[1](67, 35), T6]
    transforms += [ref.rotation(23, 17, deg, mag, 0.31, -0.17) for deg in (13, 30, 45, 180) for mag in (0.97, 1.02)]
    moved = 0
    for cfa in cref.CFAS + [c.lower() for c in cref.CFAS]:
        for trans in transforms:
            got = nl.drizzle_cfa_transform(trans, cfa)
            want = cref.cfa_transform_double(trans, cfa).astype(f32)
            assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cfa, trans)
            assert np.array_equal(got[[0, 1, 3, 4]].view(np.uint32), np.asarray(trans, f32)[[0, 1, 3, 4]].view(np.uint32))
            moved += int(not np.array_equal(got, np.asarray(trans, f32)))
    assert moved == 6 * len(transforms)                                       # every CFA but RGGB moves the origin
    assert np.array_equal(nl.drizzle_cfa_transform(T6, "RGGB"), T6)
