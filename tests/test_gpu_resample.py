"""GPU: the bicubic / Lanczos-3 resampling of the resident projection (nl_stack_frame_resample_from,
nl_group_frame_resample_from; include/nlstack_resample.h, an extension) against the fp32 restatement of its definition
(tests/resample_ref.py, which tests/test_resample_ref.py pins), fed with the library's own Lanczos-3 table: bit
equality, any NaN equals any NaN.

The kernels (resample.hip) make 256 x 16 tiles of the destination, as project.hip does; a tile either stages its
source box, grown by the kernel's radius - 1, in LDS or taps global memory.  The shapes and transforms are those of
tests/test_gpu_project_resident.py plus 7x7 (the smallest shape with wide pixels for both kernels); what each tile
path is meant for is checked through nl_stack_resample_tile_paths."""
import functools

import numpy as np
import pytest

import resample_ref as rr
from test_gpu_project_resident import DIRECT_CASES, OOB_VALUES, STAGED_FAMILIES, sources
from util import same_values

pytestmark = pytest.mark.gpu

SHAPES, transform, TRANSFORMS, BEST_POSSIBLE = rr.cases()
WIDE = (rr.BICUBIC, rr.LANCZOS3)


@functools.lru_cache(maxsize=None)
def table():
    import nightlight_amd as nl
    t = nl.lanczos3_table()
    t.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def source(shape, kind):
    sw, sh, _, _ = SHAPES[shape]
    data = sources(sw, sh, 4)[kind]
    data.flags.writeable = False
    return data


@functools.lru_cache(maxsize=None)
def truth(shape, name, kind, kernel, clamp):
    """the checker's Result with NaN out of bounds, computed once per process"""
    sw, sh, dw, dh = SHAPES[shape]
    return rr.resample(source(shape, kind), sw, sh, dw, dh, transform(shape, name), np.nan, kernel, clamp, table())


def wanted(shape, name, kind, kernel, clamp, oob):
    t = truth(shape, name, kind, kernel, clamp)
    return np.where(t.ok, t.out, np.float32(oob))


def n_tiles(dw, dh):
    return -(-dw // 256) * -(-dh // 16)


@pytest.mark.parametrize("name", list(TRANSFORMS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_resample_from_matches_the_checker(nl, shape, name):
    sw, sh, dw, dh = SHAPES[shape]
    trans = transform(shape, name)
    in_bounds = int(truth(shape, name, 0, rr.BILINEAR, False).ok.sum())
    if name == "all_oob":
        assert in_bounds == 0
    elif (shape, name) in BEST_POSSIBLE:
        assert in_bounds == BEST_POSSIBLE[shape, name]
    else:
        assert 4 * in_bounds >= dw * dh
    with nl.StackHandle(2, sw, sh) as src, nl.StackHandle(2, dw, dh) as dst:
        for kind in (0, 1):
            src.upload_frame(kind, source(shape, kind))
        for kernel in WIDE:
            staged, direct = dst.resample_tile_paths(src, 0, trans, kernel)
            print("%s %s kernel %d: %d of %d in bounds, %d wide, tiles staged %d direct %d"
                  % (shape, name, kernel, in_bounds, dw * dh, int(truth(shape, name, 0, kernel, False).wide.sum()), staged, direct))
            assert staged + direct == n_tiles(dw, dh)
            if (shape, name) in DIRECT_CASES:
                assert direct > 0
            if name in STAGED_FAMILIES:
                assert direct == 0
            if name == "all_oob":
                assert staged == 0
            for clamp in (False, True):
                for kind in (0, 1):
                    for oob in OOB_VALUES:
                        dst.frame_resample_from(1 - kind, src, kind, trans, oob, kernel, clamp)
                        assert same_values(dst.download_tile(1 - kind), wanted(shape, name, kind, kernel, clamp, oob)), \
                            (kernel, clamp, kind, oob)
        # NL_RS_BILINEAR is frame_project_from, bit for bit, and its tile paths are project_tile_paths
        assert dst.resample_tile_paths(src, 1, trans, rr.BILINEAR) == dst.project_tile_paths(src, 1, trans)
        for clamp in (False, True):
            dst.frame_project_from(0, src, 1, trans, 123.5)
            dst.frame_resample_from(1, src, 1, trans, 123.5, rr.BILINEAR, clamp)
            a, b = dst.download_tile(0), dst.download_tile(1)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert same_values(b, wanted(shape, name, 1, rr.BILINEAR, False, 123.5))


@pytest.mark.parametrize("flags", [32768, 65536, 32768 | 65536])
def test_developer_switches_change_no_bit(nl, flags):
    # 32768: every tile taps global memory (the direct path on every transform); 65536: plain result stores
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]
    with nl.StackHandle(1, sw, sh) as src, nl.StackHandle(1, dw, dh) as dst:
        src.upload_frame(0, source(shape, 1))
        dst.set_dev_flags(flags)
        for name in TRANSFORMS:
            trans = transform(shape, name)
            for kernel in WIDE:
                staged, direct = dst.resample_tile_paths(src, 0, trans, kernel)
                assert staged + direct == n_tiles(dw, dh) and (staged == 0 or not flags & 32768)
                dst.frame_resample_from(0, src, 0, trans, np.nan, kernel, kernel == rr.LANCZOS3)
                assert same_values(dst.download_tile(0), wanted(shape, name, 1, kernel, kernel == rr.LANCZOS3, np.nan)), \
                    (name, kernel)


def test_group_resamples_its_tiles_from_the_resident_slot(nl):
    shape = "530x80"
    sw, sh, dw, dh = SHAPES[shape]
    with nl.StackHandle(2, sw, sh) as src, nl.StackGroup(2, dw, dh, devices=[0, 0, 0]) as g, \
            nl.StackHandle(1, dw, dh) as single:
        assert g.size == 3
        src.upload_frame(1, source(shape, 1))
        for name in ("small_rot", "rot180", "subpixel"):
            for kernel in WIDE:
                trans = transform(shape, name)
                g.frame_resample_from(1, src, 1, trans, 123.5, kernel, True)
                single.frame_resample_from(0, src, 1, trans, 123.5, kernel, True)
                got = np.concatenate([g.tile(t).download_tile(1) for t in range(g.size)])
                assert np.array_equal(got.view(np.uint32), single.download_tile(0).view(np.uint32)), (name, kernel)
                assert same_values(got, wanted(shape, name, 1, kernel, True, 123.5)), (name, kernel)


def test_errors_leave_the_destination_as_it_was(nl):
    from nightlight_amd import capi
    w, h = 40, 24
    rng = np.random.default_rng(9)
    before = rng.standard_normal(w * h).astype(np.float32)
    ident = [1, 0, 0, 0, 1, 0]
    with nl.StackHandle(2, w, h) as src, nl.StackHandle(2, w, h) as dst, \
            nl.StackHandle(1, w, h, row0=8, rows=8) as tile:
        src.upload_frame(0, before)
        src.upload_frame(1, before)
        dst.upload_frame(0, before)
        tile.upload_frame(0, before)

        def refused(call, words):
            with pytest.raises(capi.NlError) as e:
                call()
            assert e.value.code == capi.ERR_INVALID_ARG and words in str(e.value), str(e.value)
            assert same_values(dst.download_tile(0), before)

        for kernel in WIDE:
            refused(lambda: dst.frame_resample_from(0, src, 0, [1, 2, 0, 2, 4, 0], np.nan, kernel), "Matrix has no inverse")
            refused(lambda: src.frame_resample_from(1, src, 1, ident, np.nan, kernel),
                    "frame_resample_from: slot 1 of one handle is source and destination")
            assert same_values(src.download_tile(1), before)
            refused(lambda: dst.frame_resample_from(0, tile, 0, ident, np.nan, kernel),
                    "frame_resample_from (source) needs a whole-image handle")
            refused(lambda: dst.frame_resample_from(0, src, 2, ident, np.nan, kernel), "frame_resample_from (source): bad index 2")
            refused(lambda: dst.frame_resample_from(0, src, -1, ident, np.nan, kernel), "bad index -1")
            refused(lambda: dst.resample_tile_paths(src, 2, ident, kernel), "resample_tile_paths: bad index 2")
        refused(lambda: dst.frame_resample_from(0, src, 0, ident, np.nan, 3), "frame_resample_from: unknown kernel 3")
        refused(lambda: dst.resample_tile_paths(src, 0, ident, 3), "resample_tile_paths: unknown kernel 3")
        src.frame_resample_from(1, src, 0, [1, 0, 2, 0, 1, 1], np.nan, rr.LANCZOS3)             # two slots of one handle: fine
        assert same_values(src.download_tile(0), before)


def test_a_resample_between_two_projections_changes_neither(nl):
    shape = "131x77"
    sw, sh, dw, dh = SHAPES[shape]
    trans = transform(shape, "small_rot")
    with nl.StackHandle(1, sw, sh) as src, nl.StackHandle(3, dw, dh) as dst:
        src.upload_frame(0, source(shape, 1))
        dst.frame_project_from(0, src, 0, trans, np.nan)
        dst.frame_resample_from(1, src, 0, trans, np.nan, rr.LANCZOS3, True)
        dst.frame_project_from(2, src, 0, trans, np.nan)
        first, between, second = (dst.download_tile(k) for k in range(3))
        assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
        assert same_values(first, wanted(shape, "small_rot", 1, rr.BILINEAR, False, np.nan))
        assert same_values(between, wanted(shape, "small_rot", 1, rr.LANCZOS3, True, np.nan))
