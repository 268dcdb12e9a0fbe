"""The checker of the rejection maps checks itself (CPU): tests/rejmap_ref.py takes a pixel's two clip counts from an
oracle call on that pixel alone.  That is the truth only if the reference treats pixels independently -- so for every
case of the GPU tests the per-pixel counts must sum to the totals of ONE oracle call on the whole image, and the
per-pixel results must be that call's result bit for bit.  The inputs must also be worth the name: every clipping mode
rejects on both sides at many pixels, and the special pixels are what they claim to be."""
import numpy as np
import pytest

import rejmap_ref as ref


@pytest.mark.parametrize("case", ref.CASES, ids=[c.name for c in ref.CASES])
def test_per_pixel_counts_are_the_whole_image_call(oracle, case):
    frames = ref.make_frames(case.frames, case.width, case.height)
    weights = ref.weights_of(case.frames) if case.weighted else None
    rc, want, wl, wh, _ = oracle.stack_apply(case.mode, np.ascontiguousarray(frames), weights, ref.SIGMA_LOW,
                                             ref.SIGMA_HIGH, ref.REF_LOC)
    assert rc == 0
    t = ref.truth(oracle, case)
    assert (t.clip_low, t.clip_high) == (wl, wh)
    assert (int(t.reject_low.astype(np.int64).sum()), int(t.reject_high.astype(np.int64).sum())) == (wl, wh)
    assert np.array_equal(t.result.view(np.uint32), want.view(np.uint32))
    assert np.all(t.reject_low.astype(np.int64) + t.reject_high <= t.coverage)
    if case.mode < 2:
        assert wl == 0 and wh == 0 and not t.reject_low.any() and not t.reject_high.any()


@pytest.mark.parametrize("case", ref.CLIPPING, ids=[c.name for c in ref.CLIPPING])
def test_inputs_clip_on_both_sides(oracle, case):
    """at 41 x 23 more than 100 pixels on either side; the small images of the deep stacks: more than a tenth of them"""
    t = ref.truth(oracle, case)
    least = 100 if case.width * case.height >= 900 else case.width * case.height // 10
    assert np.count_nonzero(t.reject_low) > least and np.count_nonzero(t.reject_high) > least


def test_special_pixels():
    case = ref.CASES[0]
    f = ref.make_frames(case.frames, case.width, case.height)
    cov = (~np.isnan(f)).sum(0)
    p = case.width * case.height
    assert cov[3] == 0 and cov[p - 2] == 1 and cov[case.width + 1] == case.frames
    assert np.all(f[:, case.width + 1] == f[0, case.width + 1])
    assert np.all(f.reshape(case.frames, case.height, case.width)[:, :, 5] == 1.0)
    assert 0 < cov.min() + 1 and cov.max() == case.frames and (cov < case.frames).sum() > p // 2


def test_truth_of_fewer_active_frames_is_its_own(oracle):
    case = ref.CASES[2]
    full, part = ref.truth(oracle, case), ref.truth(oracle, case, 17)
    assert part.coverage.max() == 17 and full.coverage.max() == case.frames
    assert not np.array_equal(part.reject_high, full.reject_high)
