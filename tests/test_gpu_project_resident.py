"""GPU parity of OpAlign's projection from a resident frame (nl_stack_frame_project_from, nl_group_frame_project_from;
fits/project.go:26-76 through the inverted Transform2D, coord.go:141-199) against the CPU oracle: bit equality, any
NaN equals any NaN.

The kernel (project.hip) makes 256 x 16 tiles of the destination; a tile either stages its source box in LDS or taps
global memory.  The shapes have a ragged last tile in both directions, 530 -> 521 is wider than one tile; the cases
meant for each tile path are named at DIRECT_CASES / STAGED_FAMILIES and checked through nl_stack_project_tile_paths.
"""
import numpy as np
import pytest

from util import same_values

pytestmark = pytest.mark.gpu

# source shape -> destination shape
SHAPES = {"131x77": (131, 77, 140, 70), "67x29": (67, 29, 67, 29), "530x80": (530, 80, 521, 75), "5x3": (5, 3, 9, 2)}

# the six of test_gpu_ingest.py::test_project_is_bit_exact, an integer shift (taps exactly on pixels, xr = 0), a
# 180 degree turn, a 0.5x and a 2x scale, a shear
TRANSFORMS = {
    "subpixel": [1, 0, 0.5, 0, 1, 0.25],
    "small_rot": [0.999, 0.03, -3.2, -0.03, 0.999, 4.7],
    "aniso": [1.02, 0, 0, 0, 0.98, 0],
    "rot90": [0, -1, 60, 1, 0, 0],
    "all_oob": [1, 0, 1e6, 0, 1, 0],            # deliberately everything out of bounds
    "identity": [1, 0, 0, 0, 1, 0],
    "int_shift": [1, 0, 3, 0, 1, -2],
    "rot180": [-1, 0, 0, 0, -1, 0],
    "half": [0.5, 0, 0, 0, 0.5, 0],             # the destination samples the source 2 pixels apart: large footprint
    "double": [2, 0, 0, 0, 2, 0],
    "shear": [1, 0.5, 0, 0, 1, 0],
}

# Offsets moved (the linear part and the offset's fractional part kept) where the literal transform leaves less than a
# quarter of the destination in bounds at a shape; found with the oracle alone.
MOVED = {
    ("131x77", "rot180"): [-1, 0, 132, 0, -1, 72],
    ("67x29", "rot180"): [-1, 0, 64, 0, -1, 28],
    ("530x80", "rot180"): [-1, 0, 520, 0, -1, 76],
    ("5x3", "rot180"): [-1, 0, 3, 0, -1, 1],
    ("5x3", "subpixel"): [1, 0, -0.5, 0, 1, -0.75],
    ("5x3", "small_rot"): [0.999, 0.03, -0.2, -0.03, 0.999, -0.3],
    ("5x3", "int_shift"): [1, 0, 1, 0, 1, 0],
    ("530x80", "rot90"): [0, -1, 80, 1, 0, -152],
    ("5x3", "rot90"): [0, -1, 1, 1, 0, -2],
}

# No offset reaches a quarter here, by arithmetic: a pixel in bounds has xl + 1 < src_w and yl + 1 < src_h, so a 0.5x
# scale fills at most floor((src_w - 1) / 2) x floor((src_h - 1) / 2) destination pixels (33 x 14 of 67 x 29, 2 x 1 of
# 9 x 2), and a quarter turn at most src_h - 1 destination columns (79 of 521, 2 of 9).  These cases assert that most
# instead, which the offset above reaches.
BEST_POSSIBLE = {("67x29", "half"): 33 * 14, ("5x3", "half"): 2 * 1, ("530x80", "rot90"): 79 * 75, ("5x3", "rot90"): 2 * 2}

# Meant for the direct-tap path: whole 256-column tiles whose box is 512 source columns wide.  (all_oob tiles have no
# box and take it too, without a tap.)  Meant for the staged path: every tile of the alignment-like families.
DIRECT_CASES = {("530x80", "half")}
STAGED_FAMILIES = ("subpixel", "identity", "int_shift")

OOB_VALUES = (np.nan, 123.5)              # OOBModeNaN; a finite location, as OOBModeRefLocation passes


def transform(shape, name):
    return MOVED.get((shape, name), TRANSFORMS[name])


def sources(sw, sh, seed):
    """Gaussian; Gaussian with NaN blocks and +-Inf pixels."""
    rng = np.random.default_rng(seed)
    plain = rng.standard_normal(sw * sh).astype(np.float32)
    holes = plain.copy().reshape(sh, sw)
    holes[sh // 3:sh // 3 + 2, sw // 4:sw // 4 + 3] = np.nan
    holes[0, 0] = np.nan
    holes[sh - 1, sw - 1] = np.inf
    holes[sh // 2, sw // 2] = -np.inf
    holes[sh // 2, (sw // 2 + 2) % sw] = np.inf
    return plain, holes.reshape(-1)


@pytest.fixture(scope="module")
def wanted(oracle):
    """oracle.project_bilinear of every case, computed once: (shape, transform, kind, oob index) -> array."""
    out = {}
    for shape, (sw, sh, dw, dh) in SHAPES.items():
        for kind, src in enumerate(sources(sw, sh, 4)):
            for name in TRANSFORMS:
                for o, oob in enumerate(OOB_VALUES):
                    rc, want = oracle.project_bilinear(src, sw, sh, dw, dh, transform(shape, name), oob)
                    assert rc == 0
                    out[shape, name, kind, o] = want
    return out


@pytest.mark.parametrize("name", list(TRANSFORMS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_project_from_matches_the_oracle(nl, wanted, shape, name):
    sw, sh, dw, dh = SHAPES[shape]
    trans = transform(shape, name)
    in_bounds = int((~np.isnan(wanted[shape, name, 0, 0])).sum())      # Gaussian source, NaN outside
    if name == "all_oob":
        assert in_bounds == 0
    elif (shape, name) in BEST_POSSIBLE:
        assert in_bounds == BEST_POSSIBLE[shape, name]
    else:
        assert 4 * in_bounds >= dw * dh
    with nl.StackHandle(2, sw, sh) as src, nl.StackHandle(2, dw, dh) as dst:
        for kind, data in enumerate(sources(sw, sh, 4)):
            src.upload_frame(kind, data)
        staged, direct = dst.project_tile_paths(src, 0, trans)
        print("%s %s: %d of %d in bounds, tiles staged %d direct %d" % (shape, name, in_bounds, dw * dh, staged, direct))
        assert staged + direct == -(-dw // 256) * -(-dh // 16)
        if (shape, name) in DIRECT_CASES:
            assert direct > 0
        if name in STAGED_FAMILIES:
            assert direct == 0
        if name == "all_oob":
            assert staged == 0
        for kind in (0, 1):
            for o, oob in enumerate(OOB_VALUES):
                dst.frame_project_from(1 - kind, src, kind, trans, oob)
                assert same_values(dst.download_tile(1 - kind), wanted[shape, name, kind, o]), (kind, oob)


@pytest.mark.parametrize("flags", [32768, 65536, 32768 | 65536])
def test_developer_switches_change_no_bit(nl, wanted, flags):
    # 32768: every tile taps global memory (the direct path on every transform); 65536: plain result stores
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]
    with nl.StackHandle(1, sw, sh) as src, nl.StackHandle(1, dw, dh) as dst:
        src.upload_frame(0, sources(sw, sh, 4)[1])
        dst.set_dev_flags(flags)
        for name in TRANSFORMS:
            trans = transform(shape, name)
            staged, direct = dst.project_tile_paths(src, 0, trans)
            assert staged == 0 or not flags & 32768
            dst.frame_project_from(0, src, 0, trans, np.nan)
            assert same_values(dst.download_tile(0), wanted[shape, name, 1, 0]), name


def test_row_tiles_concatenate_to_the_whole_image(nl, wanted):
    import ctypes as C
    from nightlight_amd import capi
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]

    def tile_rows(t):
        r0, nr = C.c_int(), C.c_int()
        capi.load().nl_group_tile_rows(dh, 3, t, C.byref(r0), C.byref(nr))
        return r0.value, nr.value

    with nl.StackHandle(1, sw, sh) as src:
        src.upload_frame(0, sources(sw, sh, 4)[1])
        for name in ("small_rot", "half", "shear"):
            parts = []
            for t in range(3):
                row0, rows = tile_rows(t)
                assert t == 0 or row0 > 0
                with nl.StackHandle(1, dw, dh, row0=row0, rows=rows) as dst:
                    dst.frame_project_from(0, src, 0, transform(shape, name), np.nan)
                    parts.append(dst.download_tile(0))
            assert same_values(np.concatenate(parts), wanted[shape, name, 1, 0]), name


def test_group_projects_its_tiles_from_the_resident_slot(nl, wanted):
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]
    with nl.StackHandle(2, sw, sh) as src, nl.StackGroup(2, dw, dh, devices=[0, 0, 0]) as g:
        src.upload_frame(1, sources(sw, sh, 4)[1])
        for name in ("small_rot", "rot180"):
            g.frame_project_from(1, src, 1, transform(shape, name), 123.5)
            got = np.concatenate([g.tile(t).download_tile(1) for t in range(g.size)])
            assert same_values(got, wanted[shape, name, 1, 1]), name


def test_group_tile_on_another_device_receives_its_rows_peer_to_peer(nl, wanted):
    if nl.device_count() <= 1:
        pytest.skip("nl.device_count() <= 1: the cross-device branch needs a second device")
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]
    with nl.StackHandle(1, sw, sh, device=0) as src, nl.StackGroup(1, dw, dh, devices=[1, 0, 1]) as g:
        src.upload_frame(0, sources(sw, sh, 4)[1])
        for name in ("small_rot", "rot90", "half"):
            g.frame_project_from(0, src, 0, transform(shape, name), np.nan)
            got = np.concatenate([g.tile(t).download_tile(0) for t in range(g.size)])
            assert same_values(got, wanted[shape, name, 1, 0]), name


def test_resident_chain_affine_project_stack(nl, oracle):
    # MatchHistogram (frame_affine) before Align (frame_project_from), the reference's order; one staging slot
    sw = sh = 80
    width, height, n = 72, 64, 9
    rng = np.random.default_rng(6)
    srcs = [(1000 + 30 * rng.standard_normal(sw * sh)).astype(np.float32) for _ in range(n)]
    transs = [[1, 0.01 * (k - 4), 2.0 * k - 6.5, -0.01 * (k - 4), 1, 1.5 * k - 5.25] for k in range(n)]
    ms = rng.uniform(0.95, 1.05, n).astype(np.float32)
    os_ = rng.uniform(-5, 5, n).astype(np.float32)
    matched = [oracle.affine(srcs[k], ms[k], os_[k]) for k in range(n)]
    aligned = []
    for k in range(n):
        rc, a = oracle.project_bilinear(matched[k], sw, sh, width, height, transs[k], np.nan)
        assert rc == 0
        aligned.append(a)
    rc, want, wl, wh, _ = oracle.stack_apply(2, np.stack(aligned), None, 2.5, 2.5)
    assert rc == 0 and np.isnan(np.stack(aligned)).any()
    out = np.zeros(width * height, np.float32)
    tl = th = 0
    tiles = ((0, 40), (40, 24))
    with nl.StackHandle(1, sw, sh) as staging:
        handles = [nl.StackHandle(n, width, height, row0=row0, rows=rows) for row0, rows in tiles]
        try:
            for k in range(n):
                staging.upload_frame(0, srcs[k])
                staging.frame_affine(0, ms[k], os_[k])
                for st, (row0, rows) in zip(handles, tiles):
                    st.frame_project_from(k, staging, 0, transs[k], np.nan)
                    assert same_values(st.download_tile(k), aligned[k][row0 * width:(row0 + rows) * width])
                assert same_values(staging.download_tile(0), matched[k])          # the staging slot is only read
            for st in handles:
                st.set_exact(True)
                _, cl, ch = st.run(2, 2.5, 2.5, out=out)
                tl += cl
                th += ch
        finally:
            for st in handles:
                st.close()
    assert same_values(out, want) and (tl, th) == (wl, wh)


def test_errors_leave_the_destination_as_it_was(nl):
    from nightlight_amd import capi
    w, h = 40, 24
    rng = np.random.default_rng(9)
    before = rng.standard_normal(w * h).astype(np.float32)
    ident = [1, 0, 0, 0, 1, 0]
    with nl.StackHandle(2, w, h) as src, nl.StackHandle(2, w, h) as dst, \
            nl.StackHandle(1, w, h, row0=8, rows=8) as tile, nl.StackHandle(2, w, h) as lender:
        src.upload_frame(0, before)
        src.upload_frame(1, before)
        dst.upload_frame(0, before)
        tile.upload_frame(0, before)

        def refused(call, words):
            with pytest.raises(capi.NlError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG and words in str(e.value), str(e.value)
            assert same_values(dst.download_tile(0), before)

        refused(lambda: dst.frame_project_from(0, src, 0, [1, 2, 0, 2, 4, 0]), "Matrix has no inverse")
        refused(lambda: src.frame_project_from(1, src, 1, ident), "frame_project_from")     # same slot, same handle
        assert same_values(src.download_tile(1), before)
        refused(lambda: dst.frame_project_from(0, tile, 0, ident), "whole-image")           # a row-tile source
        refused(lambda: dst.frame_project_from(0, src, 2, ident), "bad index 2")
        refused(lambda: dst.frame_project_from(0, src, -1, ident), "bad index -1")
        dst.attach_device_frames(lender.frames_device_ptr(), lender.frame_stride())
        try:
            with pytest.raises(capi.NlError) as e:
                dst.frame_project_from(0, src, 0, ident)
            assert e.value.code == capi.ERR_INVALID_ARG and "attached" in str(e.value)
        finally:
            dst.attach_device_frames(None)
        assert same_values(dst.download_tile(0), before)
        src.frame_project_from(1, src, 0, [1, 0, 2, 0, 1, 1])                                # two slots of one handle: fine
        assert same_values(src.download_tile(0), before)


@pytest.mark.parametrize("name", ["small_rot", "half", "rot90"])
def test_same_bits_as_the_projected_upload(nl, name):
    shape = "131x77"
    sw, sh, dw, dh = SHAPES[shape]
    data = sources(sw, sh, 11)[1]
    trans = transform(shape, name)
    with nl.StackHandle(1, sw, sh) as src, nl.StackHandle(2, dw, dh) as dst:
        src.upload_frame(0, data)
        dst.frame_project_from(0, src, 0, trans, np.nan)
        dst.upload_frame_projected(1, data, sw, sh, trans, np.nan, 1.0, 0.0)
        a, b = dst.download_tile(0), dst.download_tile(1)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
