"""The cases the alignment tests share (tests/test_align_ref.py, tests/test_gpu_align.py): frames from
align_ref.make_case, each the smallest at which a stage of the device path can go wrong, and the computed references,
each computed once.  Every generated case is free of ties -- no two reference points at one minimum distance, no equal
distances reaching into the shortlist -- so that the reference's outcome does not depend on Go's unstable sort; the
seeds are chosen so, and tests/test_align_ref.py asserts it of every case."""
import functools

import numpy as np

import align_ref

WIDTH, HEIGHT = 1200, 900                  # minLength = 45

# name: (k, arguments of align_ref.make_case)
CASES = {
    # exactly 3 usable stars: one triangle on either side, n_cands = 1 < K
    "k3-three-stars": (3, dict(seed=11, n_ref=3, drop=0.0, add=0.0)),
    "k8-12-stars": (8, dict(seed=12, n_ref=12)),
    "k50-60-stars": (50, dict(seed=13, n_ref=60)),             # fewer than K picked: close pairs drop out
    "k50-300-stars": (50, dict(seed=14, n_ref=300)),           # 19 600 triangles: 39 LDS tiles in 13 chunks
    "fewer-stars-than-k": (20, dict(seed=15, n_ref=10)),
    "close-stars-skipped": (10, dict(seed=16, n_ref=30, close=6)),
    "binned-frame": (12, dict(seed=17, n_ref=40, frame_width=WIDTH // 2)),      # scale factor 2
    # reference triangles on either side of the LDS tile of 512: C(15, 3) = 455, C(16, 3) = 560 (two chunks)
    "k15-455-triangles": (15, dict(seed=18, n_ref=40)),
    "k16-560-triangles": (16, dict(seed=19, n_ref=40)),
    # reference stars on either side of a wave and of the LDS tile of 1024
    "63-ref-stars": (8, dict(seed=20, n_ref=63)),
    "64-ref-stars": (8, dict(seed=21, n_ref=64)),
    "65-ref-stars": (8, dict(seed=22, n_ref=65)),
    "1025-ref-stars": (8, dict(seed=23, n_ref=1025, drop=0.5, add=0.0)),
    "rotated-scaled": (10, dict(seed=24, n_ref=50, angle=-0.04, shift=(-31.0, 18.5), scale=1.01)),
}


@functools.lru_cache(maxsize=None)
def frames(name):
    """(ref_x, ref_y, x, y, frame_width) of a case"""
    return align_ref.make_case(width=WIDTH, height=HEIGHT, **CASES[name][1])


@functools.lru_cache(maxsize=None)
def aligner(name):
    ref_x, ref_y = frames(name)[:2]
    return align_ref.RefAligner(WIDTH, HEIGHT, ref_x, ref_y, CASES[name][0])


@functools.lru_cache(maxsize=None)
def reference(name, path="kdtree"):
    """align_ref's result for a case, computed once: treat it as read-only"""
    _, _, x, y, frame_width = frames(name)
    return aligner(name).align(frame_width, x, y, path)


# ---- the 8-pixel boundary: reference stars on an integer lattice, the identity, offsets with exact squares ----------
LATTICE_STEP = 40.0
ROOT_14 = np.float32(3.7416575)            # 49 + fl(ROOT_14 * ROOT_14) == 63 exactly in fp32
# (offset, matched): dsq = 64 exactly is not a match (strict <, align.go:200), 63 is
LATTICE_OFFSETS = [((0.0, 0.0), True), ((8.0, 0.0), False), ((0.0, -8.0), False), ((7.0, ROOT_14), True),
                   ((6.0, 5.0), True), ((8.0, 1.0), False), ((-5.0, -6.0), True), ((20.0, 20.0), False)]


def lattice_case():
    """(ref_x, ref_y, x, y, expected ref_index): star i sits at lattice point i (the first at the origin, so that its
    offset survives the subtraction exactly) plus offset i"""
    side = 4
    gy, gx = np.divmod(np.arange(side * side), side)
    ref_x, ref_y = (gx * LATTICE_STEP).astype(np.float32), (gy * LATTICE_STEP).astype(np.float32)
    order = [5, 10, 15, 0, 3, 6, 9, 12]           # (7, ROOT_14) at the origin
    x = np.array([ref_x[i] + np.float32(o[0]) for i, (o, _) in zip(order, LATTICE_OFFSETS)], np.float32)
    y = np.array([ref_y[i] + np.float32(o[1]) for i, (o, _) in zip(order, LATTICE_OFFSETS)], np.float32)
    want = np.array([i if hit else -1 for i, (_, hit) in zip(order, LATTICE_OFFSETS)], np.int32)
    return ref_x, ref_y, x, y, want
