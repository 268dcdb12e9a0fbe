"""Return codes and nl_last_error() strings of the two goal-seek entries where no handle or group is given: rows in the
form of tests/test_frame_entry_errors.py, for nl_stack_find_sigmas (nlstack_pass.hip) and nl_group_find_sigmas
(nlstack_group.hip), which share one driver (goal_seek.hpp) but check their arguments each in its own way.

A characterisation table: EXPECTED was recorded from the library as it was before the two drivers became one and must not
be regenerated from the code under test.  Every row first sets a known error from another unit (SENTINEL), so a call that
leaves the thread's message alone shows it.  (The group does not check the mode itself: that row needs a device and is
in tests/test_gpu_group_goal_seek.py.)"""
import ctypes as C

import numpy as np

from nightlight_amd import capi

SENTINEL = "Invalid weighting mode 7"
f = capi.fptr
OUT = np.zeros(16, np.float32)
NO_REDUCER = C.cast(None, capi.REDUCE_FN)


def _i():
    return C.byref(C.c_int(0))


def _i64():
    return C.byref(C.c_int64(0))


def _fl():
    return C.byref(C.c_float(0))


def _stack(L, mode, full=True):
    if full:
        return L.nl_stack_find_sigmas(None, mode, 0.0, 1.0, 1.0, NO_REDUCER, None, f(OUT), _i64(), _i64(), _fl(), _fl(), _i())
    return L.nl_stack_find_sigmas(None, mode, 0.0, 1.0, 1.0, NO_REDUCER, None, None, None, None, None, None, None)


def _group(L, mode, full=True):
    if full:
        return L.nl_group_find_sigmas(None, mode, 0.0, 1.0, 1.0, f(OUT), _i64(), _i64(), _fl(), _fl(), _i())
    return L.nl_group_find_sigmas(None, mode, 0.0, 1.0, 1.0, None, None, None, None, None, None)


# (row id, call(L) -> return code)
ROWS = [
    ("stack/null-handle", lambda L: _stack(L, capi.ST_SIGMA)),
    ("stack/null-handle+null-outputs", lambda L: _stack(L, capi.ST_SIGMA, full=False)),
    ("stack/null-handle+auto", lambda L: _stack(L, capi.ST_AUTO)),
    ("stack/null-handle+mode9", lambda L: _stack(L, 9)),                 # the handle is checked in front of the mode
    ("group/null-group", lambda L: _group(L, capi.ST_SIGMA)),
    ("group/null-group+null-outputs", lambda L: _group(L, capi.ST_SIGMA, full=False)),
    ("group/null-group+auto", lambda L: _group(L, capi.ST_AUTO)),
    ("group/null-group+mode9", lambda L: _group(L, 9)),
]
EXPECTED = {
    "stack/null-handle": (capi.ERR_INVALID_ARG, "null handle"),
    "stack/null-handle+null-outputs": (capi.ERR_INVALID_ARG, "null handle"),
    "stack/null-handle+auto": (capi.ERR_INVALID_ARG, "null handle"),
    "stack/null-handle+mode9": (capi.ERR_INVALID_ARG, "null handle"),
    # the group gives its code and leaves the thread's message alone, as nl_group_run and the setters do
    "group/null-group": (capi.ERR_INVALID_ARG, SENTINEL),
    "group/null-group+null-outputs": (capi.ERR_INVALID_ARG, SENTINEL),
    "group/null-group+auto": (capi.ERR_INVALID_ARG, SENTINEL),
    "group/null-group+mode9": (capi.ERR_INVALID_ARG, SENTINEL),
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


def test_every_row_has_its_expectation():
    ids = [rid for rid, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    L = capi.load()
    got = {rid: run_row(L, call) for rid, call in ROWS}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong


def test_nothing_is_written_without_a_handle():
    L = capi.load()
    for call in (lambda *a: L.nl_stack_find_sigmas(None, capi.ST_SIGMA, 0.0, 1.0, 1.0, NO_REDUCER, None, *a),
                 lambda *a: L.nl_group_find_sigmas(None, capi.ST_SIGMA, 0.0, 1.0, 1.0, *a)):
        out = np.full(16, np.float32(-7.5))
        cl, ch, sl, sh, passes = C.c_int64(-3), C.c_int64(-4), C.c_float(-1.5), C.c_float(-2.5), C.c_int(-9)
        rc = call(f(out), C.byref(cl), C.byref(ch), C.byref(sl), C.byref(sh), C.byref(passes))
        assert rc == capi.ERR_INVALID_ARG
        assert np.all(out == np.float32(-7.5))
        assert (cl.value, ch.value, sl.value, sh.value, passes.value) == (-3, -4, -1.5, -2.5, -9)
