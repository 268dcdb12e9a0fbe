"""The entries of the maps passes, one table row per public header: include/nlstack_maps.h and, beside it,
include/nlstack_fastmaps.h, nlstack_residentmaps.h and nlstack_deepmaps.h (all part of the interface nlstack.h includes).
Each header declares exactly its export list of capi, the library exports them, they are no entry of another list, and
every argument check that ends in front of the device gives its code and message -- for the three later headers those
of the entry it stands beside (nl_stack_run_maps / nl_group_run_maps): characterisation tables in the form of
tests/test_locscale_entries.py."""
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


def _i64():
    return C.byref(C.c_int64(0))


U16 = np.zeros(16, np.uint16)
u16 = U16.ctypes.data_as(C.POINTER(C.c_uint16))
F32 = np.zeros(16, np.float32)

# nlstack_maps.h -- (row id, entry, call(L) -> return code)
MAPS_ROWS = [
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

MAPS_EXPECTED = {
    "run_maps/null-handle": (-6, "null handle"),
    "run_maps/null-handle+bad-mode": (-6, "null handle"),
    "coverage/null-handle": (-6, "null handle"),
    "coverage/null-handle+null-output": (-6, "null handle"),
    "last_coverage_ms/null-handle": (-1, SENTINEL),          # no timing, and the thread's error stays as it was
    "group_run_maps/null-group": (-6, "null group"),
    "group_coverage/null-group": (-6, "null group"),
    "group_coverage/null-group+null-output": (-6, "null group"),
}

# the later headers -- (row id, entry, the existing entry that gives the expected code and message, call(L, entry name) -> return code)
FAST_ROWS = [
    ("run_maps_fast/null-handle", "nl_stack_run_maps_fast", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_fast/null-handle+bad-mode", "nl_stack_run_maps_fast", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_fast/null-group", "nl_group_run_maps_fast", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_fast/null-group+null-outputs", "nl_group_run_maps_fast", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 3, 2.0, 2.5, 0.0, None, None, None, None, None)),
]

FAST_EXPECTED = {
    "run_maps_fast/null-handle": (-6, "null handle"),
    "run_maps_fast/null-handle+bad-mode": (-6, "null handle"),
    "group_run_maps_fast/null-group": (-6, "null group"),
    "group_run_maps_fast/null-group+null-outputs": (-6, "null group"),
}

RESIDENT_ROWS = [
    ("run_maps_resident/null-handle", "nl_stack_run_maps_resident", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_resident/null-handle+bad-mode", "nl_stack_run_maps_resident", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_resident/null-group", "nl_group_run_maps_resident", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_resident/null-group+null-outputs", "nl_group_run_maps_resident", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 3, 2.0, 2.5, 0.0, None, None, None, None, None)),
]

RESIDENT_EXPECTED = {
    "run_maps_resident/null-handle": (-6, "null handle"),
    "run_maps_resident/null-handle+bad-mode": (-6, "null handle"),
    "group_run_maps_resident/null-group": (-6, "null group"),
    "group_run_maps_resident/null-group+null-outputs": (-6, "null group"),
}

DEEP_ROWS = [
    ("run_maps_deep/null-handle", "nl_stack_run_maps_deep", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("run_maps_deep/null-handle+bad-mode", "nl_stack_run_maps_deep", "nl_stack_run_maps",
     lambda L, e: getattr(L, e)(None, 9, 2.0, 2.5, 0.0, None, None, None, None, None)),
    ("group_run_maps_deep/null-group", "nl_group_run_maps_deep", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 2, 2.0, 2.5, 0.0, f(F32), _i64(), _i64(), u16, u16)),
    ("group_run_maps_deep/null-group+null-outputs", "nl_group_run_maps_deep", "nl_group_run_maps",
     lambda L, e: getattr(L, e)(None, 3, 2.0, 2.5, 0.0, None, None, None, None, None)),
]

DEEP_EXPECTED = {
    "run_maps_deep/null-handle": (-6, "null handle"),
    "run_maps_deep/null-handle+bad-mode": (-6, "null handle"),
    "group_run_maps_deep/null-group": (-6, "null group"),
    "group_run_maps_deep/null-group+null-outputs": (-6, "null group"),
}

# One row per header.  suffix: what its two pass entries add to nl_stack_run_maps / nl_group_run_maps (None: the header that
# declares those two, which stands beside nothing).  others: the export lists it must share no entry with.  uint16: how
# many `uint16_t *` its declarations hold.  words: what the header's comment must say.  must_declare: entries the
# interface is about.
TABLE = {
    "maps": dict(header="nlstack_maps.h", exports="MAPS_EXPORTS", suffix=None, uint16=6, words=(),
                 others=("EXPORTS", "LOCSCALE_EXPORTS", "ALIGN_EXPORTS"),
                 must_declare={"nl_stack_run_maps", "nl_stack_coverage", "nl_group_run_maps", "nl_group_coverage"},
                 rows=MAPS_ROWS, expected=MAPS_EXPECTED),
    "fast": dict(header="nlstack_fastmaps.h", exports="FASTMAPS_EXPORTS", suffix="_fast", uint16=4,
                 words=("When the fast engines run", "Maps.", "Result.", "Everything else.", "Kernel name.",
                        "stack_sigma_fast_kernel", "nl_stack_set_exact"),
                 others=("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "WLINFIT_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS"),
                 must_declare={"nl_group_run_maps_fast", "nl_stack_run_maps_fast"},
                 rows=FAST_ROWS, expected=FAST_EXPECTED),
    "resident": dict(header="nlstack_residentmaps.h", exports="RESIDENTMAPS_EXPORTS", suffix="_resident", uint16=4,
                     words=("When the resident engines run.", "Maps.", "Result.", "Everything else.", "Kernel name.",
                            "stack_linfit_fast_kernel", "stack_linfit_ml_kernel", "nl_stack_set_exact",
                            "bit-exact, not merely within 1e-6"),
                     others=("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "WLINFIT_EXPORTS",
                             "WCLIP_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS"),
                     must_declare={"nl_group_run_maps_resident", "nl_stack_run_maps_resident"},
                     rows=RESIDENT_ROWS, expected=RESIDENT_EXPECTED),
    "deep": dict(header="nlstack_deepmaps.h", exports="DEEPMAPS_EXPORTS", suffix="_deep", uint16=4,
                 words=("When the deep engines run.", "Maps.", "Result.", "Everything else.", "Kernel name.",
                        "stack_sigma_mlz_kernel", "nl_stack_set_exact", "NL_ERR_INVALID_MODE", "NL_ERR_WEIGHTED_MAD",
                        "NL_ERR_TOO_MANY_FRAMES", "1e-6", "Out of scope"),
                 others=("EXPORTS", "LOCSCALE_EXPORTS", "MAPS_EXPORTS", "FASTMAPS_EXPORTS", "RESIDENTMAPS_EXPORTS",
                         "WLINFIT_EXPORTS", "WCLIP_EXPORTS", "ALIGN_EXPORTS", "RESAMPLE_EXPORTS"),
                 must_declare={"nl_group_run_maps_deep", "nl_stack_run_maps_deep"},
                 rows=DEEP_ROWS, expected=DEEP_EXPECTED),
}
BESIDE = [k for k, row in TABLE.items() if row["suffix"]]      # the headers whose entries stand beside nlstack_maps.h's
PASS_ENTRIES = [base + (TABLE[k]["suffix"] or "") for k in TABLE for base in ("nl_stack_run_maps", "nl_group_run_maps")]


def _uncommented(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, header)).read(), flags=re.S)


def _rows(row):
    """the row's ROWS as (row id, entry, entry it stands beside or None, call(L, entry name))"""
    if row["suffix"] is None:
        return [(rid, entry, None, (lambda L, e, call=call: call(L))) for rid, entry, call in row["rows"]]
    return row["rows"]


@pytest.mark.parametrize("key", TABLE)
def test_header_exports_and_binding_agree(key):
    row = TABLE[key]
    raw = open(os.path.join(INC, row["header"])).read()
    text = _uncommented(row["header"])
    declared = sorted(set(re.findall(r"\b(nl_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(getattr(capi, row["exports"]))
    assert row["must_declare"] <= set(declared)
    if row["suffix"]:
        assert set(declared) == row["must_declare"]
    others = sum((getattr(capi, name) for name in row["others"]), [])
    assert not set(declared) & set(others)
    assert '#include "%s"' % row["header"] in open(os.path.join(INC, "nlstack.h")).read()
    lib = C.CDLL(capi.LIB_PATH)
    assert all(hasattr(lib, s) for s in declared)
    # the maps are uint16, and a later header's entries take the arguments of the entries they stand beside
    assert len(re.findall(r"uint16_t \*", text)) == row["uint16"]
    if row["suffix"]:
        maps = _uncommented("nlstack_maps.h")
        for name in ("nl_stack_run_maps", "nl_group_run_maps"):
            proto = lambda t, n: re.sub(r"\s+", " ", re.search(r"\b%s\s*\(([^)]*)\)" % n, t).group(1))
            assert proto(text, name + row["suffix"]) == proto(maps, name)
    # the contract is in the header's comment
    for word in row["words"]:
        assert word in raw, word


def test_python_layer_takes_the_switch():
    from nightlight_amd import stack
    for cls in (stack.StackHandle, stack.StackGroup):
        assert inspect.signature(cls.run_maps).parameters["fast"].default is False


@pytest.mark.parametrize("method", ["run_maps_resident", "run_maps_deep"])
def test_python_layer_has_both_methods(method):
    from nightlight_amd import stack
    handle, group = inspect.signature(getattr(stack.StackHandle, method)), inspect.signature(getattr(stack.StackGroup, method))
    assert list(handle.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc", "out", "reject_low", "reject_high"]
    assert list(group.parameters) == ["self", "mode", "sigma_low", "sigma_high", "ref_loc"]
    # run_maps and its switch are what they were
    for cls in (stack.StackHandle, stack.StackGroup):
        assert inspect.signature(cls.run_maps).parameters["fast"].default is False
    # the binding gives both entries the argument types of the entries they stand beside
    L = capi.load()
    assert getattr(L, "nl_stack_" + method).argtypes == L.nl_stack_run_maps.argtypes
    assert getattr(L, "nl_group_" + method).argtypes == L.nl_group_run_maps.argtypes


def run_row(L, call, entry):
    """(return code, nl_last_error()) of one row, after the sentinel error"""
    bad = C.c_int(-1)
    w = np.zeros(1, np.float32)
    assert L.nl_weights_from_scalars(7, f(w), 1, f(w), C.byref(bad)) == capi.ERR_INVALID_WEIGHTING
    assert L.nl_last_error().decode().startswith(SENTINEL)
    rc = call(L, entry)
    msg = L.nl_last_error().decode("utf-8", "replace")
    return rc, (SENTINEL if msg.startswith(SENTINEL) else msg)


@pytest.mark.parametrize("key", TABLE)
def test_every_entry_has_a_row(key):
    row = TABLE[key]
    assert {r[1] for r in row["rows"]} == set(getattr(capi, row["exports"]))
    ids = [r[0] for r in row["rows"]]
    assert len(set(ids)) == len(ids) and set(ids) == set(row["expected"])


@pytest.mark.parametrize("key", TABLE)
def test_codes_and_messages_in_front_of_the_device(key):
    row = TABLE[key]
    L = capi.load()
    got = {rid: run_row(L, call, entry) for rid, entry, _, call in _rows(row)}
    wrong = {rid: (got[rid], row["expected"][rid]) for rid in got if got[rid] != row["expected"][rid]}
    assert not wrong, "(got, expected) per row: %r" % wrong
    # ... which is what the existing entry gives for the same arguments
    beside = {rid: run_row(L, call, existing) for rid, _, existing, call in _rows(row) if existing}
    assert beside == (got if row["suffix"] else {})


@pytest.mark.parametrize("entry", PASS_ENTRIES)
def test_no_cpu_result_where_no_handle_can_be_made(entry):
    """A pass needs a handle, and a handle needs a device: where none is visible every maps entry ends as
    nl_stack_run_maps does -- no handle, NL_ERR_INVALID_ARG, the outputs untouched -- never with a result of the CPU."""
    import nightlight_amd as nl
    L = capi.load()
    if capi.device_count() == 0:
        with pytest.raises(capi.NlError) as e:
            nl.StackHandle(4, 8, 8)
        assert "no HIP device" in str(e.value) or "hipGetDeviceCount" in str(e.value)
        with pytest.raises(capi.NlError):
            nl.StackGroup(4, 8, 8)
    out = np.full(16, np.float32(-7.5))
    low, high = np.full(16, 0xABCD, np.uint16), np.full(16, 0x1234, np.uint16)
    cl, ch = C.c_int64(-3), C.c_int64(-4)
    rc = getattr(L, entry)(None, 2, 2.0, 2.5, 0.0, f(out), C.byref(cl), C.byref(ch),
                           low.ctypes.data_as(C.POINTER(C.c_uint16)), high.ctypes.data_as(C.POINTER(C.c_uint16)))
    assert rc == capi.ERR_INVALID_ARG, entry
    assert np.all(out == np.float32(-7.5)) and np.all(low == 0xABCD) and np.all(high == 0x1234), entry
    assert (cl.value, ch.value) == (-3, -4), entry
