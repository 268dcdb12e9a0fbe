"""GPU parity of background extraction -- OpBackExtract through nl_back_extract and nl_stack_frame_back_extract --
against the CPU restatement in background_ref.py.

Bar: the bits of the smoothed cells, of every info field, of the subtracted frame and of the rendered background equal
the restatement's; any NaN equals any NaN, and zeros compare sign-blind (deviation 4).  Where the restatement panics
or hangs, the library returns NL_ERR_INVALID_ARG.  Everything runs in this one pytest process.
"""
import threading

import numpy as np
import pytest

import background_ref as ref
from test_gpu_stars import field, loc_scale

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    if a.shape != b.shape:
        return False
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))
    return bool(ok.all())


def first_diff(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))
    bad = np.flatnonzero(~ok)
    return "%d differ, first %d: %r vs %r" % (bad.size, bad[0], a[bad[0]], b[bad[0]]) if bad.size else "none"


def check(got, want):
    g_out, g_bg, g_cells, g_info = got
    w_out, w_bg, w_cells, w_info = want
    assert same(g_cells, w_cells), "cells: " + first_diff(g_cells, w_cells)
    for k, v in w_info.items():
        assert same([g_info[k]], [v]) if isinstance(v, np.floating) else g_info[k] == v, (k, g_info[k], v)
    if g_out is not None:
        assert same(g_out, w_out), "frame: " + first_diff(g_out, w_out)
    if g_bg is not None:
        assert same(g_bg, w_bg), "background: " + first_diff(g_bg, w_bg)


@pytest.fixture(scope="module")
def star_fields(nl):
    """(data, stars) per (shape, kind): find_stars on a star field with NaN blocks, and on an integer-valued one."""
    cache = {}

    def get(w, h, kind):
        if (w, h, kind) not in cache:
            data = field(w, h, 11, nan_blocks=(kind == "nan"), integer=(kind == "int"))
            loc, scale = loc_scale(data)
            stars, _, _ = nl.find_stars(data, w, h, loc, scale, radius=16)
            cache[(w, h, kind)] = (data, stars)
        return cache[(w, h, kind)]
    return get


def run_both(nl, oracle, data, w, h, stars, g, clip=0, render=False, hfr_factor=4.0, sigma=1.5):
    try:
        want = ref.back_extract(data, w, h, stars, g, oracle, hfr_factor, sigma, clip)
    except ref.GoPanic as e:
        print("reference panics: %s" % e)
        with pytest.raises(nl.NlError) as err:
            nl.back_extract(data, w, h, stars, g, hfr_factor, sigma, clip, render)
        assert err.value.code == nl.capi.ERR_INVALID_ARG, str(e)
        return None
    got = nl.back_extract(data, w, h, stars, g, hfr_factor, sigma, clip, render)
    if not render:
        want = (want[0], None, want[2], want[3])
    check(got, want)
    return got


OUTCOMES = {}
CASES = [((67, 29), 7, 0), ((67, 29), 7, 3), ((67, 29), 32, 0), ((1080, 1920), 7, 0), ((1080, 1920), 32, 3),
         ((1080, 1920), 100, "q"), ((4096, 4096), 64, 0), ((4096, 4096), 32, 3), ((4096, 4096), 256, "q"),
         ((6000, 4000), 64, 3), ((6000, 4000), 512, 0), ((6000, 4000), 256, 0)]


@pytest.mark.parametrize("kind", ["nan", "int"])
@pytest.mark.parametrize("shape,g,clip", CASES)
def test_parity(nl, oracle, star_fields, shape, g, clip, kind):
    w, h = shape
    data, stars = star_fields(w, h, kind)
    q = clip == "q"
    if q:
        clip = max(1, ((w + g // 2) // g) * ((h + g // 2) // g) // 4)
    got = run_both(nl, oracle, data, w, h, stars, g, clip, render=(g in (32, 256)))
    OUTCOMES[(shape, g, q, kind)] = got is not None


def test_parity_compared_frames():
    # the parity cases above must compare frames, not only agree on rejections
    print(sorted(OUTCOMES.items()))
    assert sum(OUTCOMES.values()) >= len(OUTCOMES) // 2


def test_render_equals_subtract(nl, star_fields):
    data, stars = star_fields(1080, 1920, "int")
    a = nl.back_extract(data, 1080, 1920, stars, 64)
    b = nl.back_extract(data, 1080, 1920, stars, 64, render=True)
    assert a[1] is None and b[1] is not None
    assert same(a[0], b[0]) and same(a[2], b[2]) and a[3] == b[3]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_handmade_stars(nl, oracle):
    w, h = 640, 480
    rng = np.random.default_rng(5)
    data = (500.0 + 3.0 * rng.standard_normal((h, w))).astype(np.float32).reshape(-1)
    st = np.zeros(6, nl.capi.STAR_DTYPE)
    st["x"] = [100.5, -30.0, 700.0, 320.0, 5.0, 320.0]
    st["y"] = [100.0, -12.0, 500.0, 240.0, 470.0, 240.0]
    st["hfr"] = [2.0, 3.0, 4.0, 1e9, np.nan, 1.5]
    st["mass"] = 1.0
    for g, clip in ((64, 0), (100, 2), (7, 0)):
        run_both(nl, oracle, data, w, h, st, g, clip)
    # a star of moderate size masking most of a cell, and one whose disc reaches the neighbours
    st2 = st[[0, 3]].copy()
    st2["hfr"] = [8.0, 3.0]
    run_both(nl, oracle, data, w, h, st2, 64, 0, render=True)


def test_nan_cells_take_the_host_path(nl, oracle):
    # one NaN far from the pivot of the first partition: the literal select returns, and the device must defer
    w, h = 64, 64
    data = np.arange(w * h, dtype=np.float32) % 97 + 100
    data[5] = np.nan
    got = run_both(nl, oracle, data, w, h, None, 32)
    assert got is not None


def test_resident_equals_host(nl, oracle, star_fields):
    w, h = 1080, 1920
    data, stars = star_fields(w, h, "int")
    host = nl.back_extract(data, w, h, stars, 64, clip=3, render=True)
    with nl.StackHandle(2, w, h, device=0) as st:
        st.upload_frame(1, data)
        res = st.frame_back_extract(1, stars, 64, clip=3, render=True)
        out = st.download_tile(1)
    assert res[0] is None
    assert np.array_equal(out.view(np.uint32), host[0].view(np.uint32))
    assert np.array_equal(res[1].view(np.uint32), host[1].view(np.uint32))
    assert np.array_equal(res[2].view(np.uint32), host[2].view(np.uint32)) and res[3] == host[3]


def test_grid_zero_leaves_the_slot(nl, star_fields):
    w, h = 67, 29
    data, stars = star_fields(w, h, "nan")
    with nl.StackHandle(1, w, h, device=0) as st:
        st.upload_frame(0, data)
        res = st.frame_back_extract(0, stars, 0)
        out = st.download_tile(0)
    assert np.array_equal(out.view(np.uint32), data.view(np.uint32))
    assert res[2].size == 0 and res[3]["cells_x"] == 0
    out2, bg, cells, info = nl.back_extract(data, w, h, stars, -5)
    assert out2 is None and bg is None and cells.size == 0


def test_row_tile_rejected(nl):
    w, h = 256, 256
    with nl.StackHandle(1, w, h, row0=0, rows=128, device=0) as st:
        with pytest.raises(nl.NlError) as e:
            st.frame_back_extract(0, None, 32)
    assert e.value.code == nl.capi.ERR_INVALID_ARG and "whole-image" in str(e.value)


def test_deviations(nl, oracle):
    rng = np.random.default_rng(9)
    img = (100 + rng.standard_normal(96 * 64)).astype(np.float32)
    cases = [
        (img, 96, 64, None, 200, 0),             # deviation 2: fewer than half a cell
        (img, 96, 64, None, 64, 0),              # one cell tall: Subtract indexes Cells[-1]
        (np.full(96 * 64, 7, np.float32), 96, 64, None, 32, 0),   # flat plateau: mad 0, empty trimmed set
        (img, 96, 64, None, 16, 24),             # clip = every cell: the endless interpolation
    ]
    st = np.zeros(1, nl.capi.STAR_DTYPE)
    st["x"], st["y"], st["hfr"] = 16.0, 16.0, 100.0
    cases.append((img, 96, 64, st, 32, 0))      # a cell with no sample left after masking
    for data, w, h, stars, g, clip in cases:
        with pytest.raises(ref.GoPanic):
            ref.back_extract(data, w, h, stars, g, oracle, clip_n=clip)
        with pytest.raises(nl.NlError) as e:
            nl.back_extract(data, w, h, stars, g, clip=clip)
        assert e.value.code == nl.capi.ERR_INVALID_ARG
        assert "background.go" in str(e.value) or "qsort.go" in str(e.value)


def test_four_threads(nl, star_fields):
    w, h = 1080, 1920
    data, stars = star_fields(w, h, "int")
    want = nl.back_extract(data, w, h, stars, 64, clip=3)
    results, errors = [None] * 4, []

    def work(i):
        try:
            results[i] = nl.back_extract(data, w, h, stars, 64, clip=3)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    for r in results:
        assert np.array_equal(r[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(r[2].view(np.uint32), want[2].view(np.uint32))


def test_resident_chain_into_a_stack_pass(nl, oracle):
    """calibrate-free chain on resident slots: badpixel -> find_stars -> back_extract -> mean stack, against
    the same chain through the restatement (background) and the oracle (stack)."""
    w, h, n = 512, 384, 4
    frames = [field(w, h, 20 + i, nan_blocks=False, integer=True) for i in range(n)]
    with nl.StackHandle(n, w, h, device=0) as st:
        want = []
        for i, f in enumerate(frames):
            st.upload_frame(i, f)
            st.frame_badpixel(i, 3.0, 5.0)
            pre = st.download_tile(i)
            loc, scale = loc_scale(pre)
            stars, _, _ = st.frame_find_stars(i, loc, scale)
            out, _, _, _ = ref.back_extract(pre, w, h, stars, 64, oracle)
            st.frame_back_extract(i, stars, 64)
            got = st.download_tile(i)
            assert same(got, out), "frame %d: %s" % (i, first_diff(got, out))
            want.append(out)
        res, _, _ = st.run(nl.ST_MEAN, 3.0, 3.0)
    rc, exp, _, _, _ = oracle.stack_apply(nl.ST_MEAN, np.stack(want), None, 3.0, 3.0)
    assert rc == 0 and same(res, exp)
