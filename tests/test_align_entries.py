"""The alignment entries of the C ABI: include/nlstack_align.h (a part of the interface nlstack.h includes) declares
exactly capi.ALIGN_EXPORTS, the library exports them, the structs have the sizes the header spells, and on a machine
without a device every argument check that runs in front of the device gives its code and message: a
characterisation table in the form of tests/test_locscale_entries.py, whose rows state the header's contract."""
import ctypes as C
import os
import re

import numpy as np

from nightlight_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = "Invalid weighting mode 7"

STARS = np.zeros(4, capi.STAR_DTYPE)
STARS["x"], STARS["y"] = [0.0, 6.0, 24.0, 0.0], [0.0, 8.0, 7.0, 40.0]
stars = STARS.ctypes.data_as(C.c_void_p)
CANDS = np.zeros(8, capi.CANDIDATE_DTYPE)
cands = CANDS.ctypes.data_as(C.c_void_p)
REF_INDEX = np.zeros(8 * 4, np.int32)
ref_index = REF_INDEX.ctypes.data_as(C.POINTER(C.c_int32))
TRANS = np.array([1, 0, 0, 0, 1, 0], np.float32)
# the entries behind create need an aligner, which takes a device to make: none of them reads it in front of the
# device check, where the rows that pass this one end
FAKE = C.c_void_p(0x1000)


def test_header_exports_and_binding_agree():
    inc = os.path.join(ROOT, "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nlstack_align.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(capi.ALIGN_EXPORTS)
    assert not set(declared) & set(capi.EXPORTS) and not set(declared) & set(capi.LOCSCALE_EXPORTS)
    assert '#include "nlstack_align.h"' in open(os.path.join(inc, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the structs and the constant as the header spells them
    assert re.search(r"#define NL_ALIGN_MAX_K %d\b" % capi.ALIGN_MAX_K, text)
    assert re.search(r"sizeof\(nl_align_triangle_t\) == %d && sizeof\(nl_align_candidate_t\) == %d\b"
                     % (capi.TRIANGLE_DTYPE.itemsize, capi.CANDIDATE_DTYPE.itemsize), text)
    assert C.sizeof(capi.AlignInfo) == 3 * 8 + 4 * 4 + 4 * capi.ALIGN_MAX_K
    assert capi.AlignInfo.picked.offset == 40 and capi.AlignInfo.tri_capacity.offset == 24
    assert [capi.CANDIDATE_DTYPE.fields[n][1] for n in ("trans", "trans_ok", "enough")] == [36, 60, 68]


def _create(L, *a):
    """nl_aligner_create reports through NULL and nl_last_error(): the code its message belongs to"""
    if L.nl_aligner_create(*a):
        return capi.OK
    return capi.ERR_NO_DEVICE if L.nl_last_error().decode().startswith("no HIP device") else capi.ERR_INVALID_ARG


def _n():
    return C.byref(C.c_int(0))


# (row id, entry, call(L) -> return code)
ROWS = [
    ("aligner_create/null-stars", "nl_aligner_create", lambda L: _create(L, 0, 100, 100, None, 4, 3)),
    ("aligner_create/k-0", "nl_aligner_create", lambda L: _create(L, 0, 100, 100, stars, 4, 0)),
    ("aligner_create/k-129", "nl_aligner_create", lambda L: _create(L, 0, 100, 100, stars, 4, 129)),
    ("aligner_create/no-stars", "nl_aligner_create", lambda L: _create(L, 0, 100, 100, stars, 0, 3)),
    ("aligner_create/no-height", "nl_aligner_create", lambda L: _create(L, 0, 100, 0, stars, 4, 3)),
    ("aligner_create/valid", "nl_aligner_create", lambda L: _create(L, 0, 100, 100, stars, 4, 3)),
    ("aligner_destroy/null", "nl_aligner_destroy", lambda L: L.nl_aligner_destroy(None) or capi.OK),
    ("aligner_info/null", "nl_aligner_info", lambda L: L.nl_aligner_info(None, None, 0, _n(), _n(), None, 0)),
    ("aligner_match/null-aligner", "nl_aligner_match",
     lambda L: L.nl_aligner_match(None, 100, stars, 4, cands, 8, _n(), ref_index, None)),
    ("aligner_match/null-stars", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 100, None, 4, cands, 8, _n(), ref_index, None)),
    ("aligner_match/no-stars", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 100, stars, 0, cands, 8, _n(), ref_index, None)),
    ("aligner_match/null-output", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 100, stars, 4, cands, 8, _n(), None, None)),
    ("aligner_match/width-0", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 0, stars, 4, cands, 8, _n(), ref_index, None)),
    ("aligner_match/capacity-0", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 100, stars, 4, cands, 0, _n(), ref_index, None)),
    ("aligner_match/valid", "nl_aligner_match",
     lambda L: L.nl_aligner_match(FAKE, 100, stars, 4, cands, 8, _n(), ref_index, None)),
    ("aligner_match_stars/null-aligner", "nl_aligner_match_stars",
     lambda L: L.nl_aligner_match_stars(None, capi.fptr(TRANS), 1, stars, 4, ref_index, ref_index)),
    ("aligner_match_stars/no-stars", "nl_aligner_match_stars",
     lambda L: L.nl_aligner_match_stars(FAKE, capi.fptr(TRANS), 1, stars, -1, ref_index, ref_index)),
    ("aligner_match_stars/null-transforms", "nl_aligner_match_stars",
     lambda L: L.nl_aligner_match_stars(FAKE, None, 1, stars, 4, ref_index, ref_index)),
    ("aligner_match_stars/129-transforms", "nl_aligner_match_stars",
     lambda L: L.nl_aligner_match_stars(FAKE, capi.fptr(TRANS), 129, stars, 4, ref_index, ref_index)),
    ("aligner_match_stars/valid", "nl_aligner_match_stars",
     lambda L: L.nl_aligner_match_stars(FAKE, capi.fptr(TRANS), 1, stars, 4, ref_index, ref_index)),
]

NO_DEVICE = (capi.ERR_NO_DEVICE,
             "no HIP device available (no ROCm-capable device is detected); libnlstack has no CPU path")
UNTOUCHED = (capi.OK, SENTINEL)           # the call succeeded and left the thread's error as it was

EXPECTED = {
    "aligner_create/null-stars": (-6, "aligner_create: null reference stars"),
    "aligner_create/k-0": (-6, "aligner_create: k 0 (1 .. 128)"),
    "aligner_create/k-129": (-6, "aligner_create: k 129 (1 .. 128)"),
    "aligner_create/no-stars": (-6, "aligner_create: Unable to align without star detections in reference frame (postprocess.go:203)"),
    "aligner_create/no-height": (-6, "aligner_create: reference frame of 100 x 0"),
    "aligner_create/valid": NO_DEVICE,
    "aligner_destroy/null": UNTOUCHED,
    "aligner_info/null": (-6, "aligner_info: null aligner"),
    "aligner_match/null-aligner": (-6, "aligner_match: null aligner"),
    "aligner_match/null-stars": (-6, "aligner_match: null stars"),
    "aligner_match/no-stars": (-6, "aligner_match: 0 stars"),
    "aligner_match/null-output": (-6, "aligner_match: null output"),
    "aligner_match/width-0": (-6, "aligner_match: frame width 0"),
    "aligner_match/capacity-0": (-6, "aligner_match: room for 0 candidates"),
    "aligner_match/valid": NO_DEVICE,
    "aligner_match_stars/null-aligner": (-6, "aligner_match_stars: null aligner"),
    "aligner_match_stars/no-stars": (-6, "aligner_match_stars: -1 stars"),
    "aligner_match_stars/null-transforms": (-6, "aligner_match_stars: null transforms or output"),
    "aligner_match_stars/129-transforms": (-6, "aligner_match_stars: 129 transforms (1 .. 128)"),
    "aligner_match_stars/valid": NO_DEVICE,
}


def run_row(L, call):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, np.float32)
    assert L.nl_weights_from_scalars(7, capi.fptr(w), 1, capi.fptr(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


def test_every_entry_has_a_row():
    assert {entry for _, entry, _ in ROWS} == set(capi.ALIGN_EXPORTS)
    ids = [rid for rid, _, _ in ROWS]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)


def test_codes_and_messages_in_front_of_the_device():
    """With a device the rows that end at the device check are left out (there they need a real aligner, which
    tests/test_gpu_align.py covers)."""
    L = capi.load()
    has_device = capi.device_count() > 0
    got = {rid: run_row(L, call) for rid, _, call in ROWS if not (has_device and EXPECTED[rid] == NO_DEVICE)}
    wrong = {rid: (got[rid], EXPECTED[rid]) for rid in got if got[rid] != EXPECTED[rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
