"""A restatement in fp32 of the reference's star aligner up to the minimiser: internal/star/align.go:58-206 with
kdtree2.go, kdtree3p.go and the parts of coord.go they use.  numpy float32 arithmetic is IEEE and never fused, so
every expression below has the bits of the Go expression it cites, operation for operation and left to right.

Two paths to the nearest neighbours:
  "kdtree"  the reference's pointerless kd-trees.  Make sorts stably (Go's sort.Slice under the reference's non-strict
            <= comparator leaves an unspecified order among equal keys; a stable sort is one of the orders it may
            leave).  The searches are the reference's mutually recursive NearestNeighbor / nearestNeighborY (/ Z),
            branch for branch, run for a batch of query points at once: at every node the batch splits by the
            reference's own conditions, so each query visits the nodes, in the order, the scalar code visits.
  "brute"   every distance, the minimum, and the documented tie rules: the lowest index wins among equal distances,
            and the shortlist is ordered by (dist, lowest triangle index).
The two agree in every bit wherever no two distinct points tie at a minimum; ties() counts those places."""
import numpy as np

F = np.float32
MIN_DISTANCE_FOR_ALIGNMENT_STARS = F(1.0) / F(20.0)            # align.go:55
DIST_SQUARED_LIMIT = F(8.0 * 8.0)                              # align.go:164


def dist2d_squared(ax, ay, bx, by):
    """coord.go:85-88"""
    dx, dy = ax - bx, ay - by
    return dx * dx + dy * dy


def dist2d(ax, ay, bx, by):
    """coord.go:79-82: float32(math.Sqrt(float64(dSquared)))"""
    return np.sqrt(np.asarray(dist2d_squared(ax, ay, bx, by), F).astype(np.float64)).astype(F)


def dist3d_squared(p, q):
    """coord.go:105-108; p, q: (..., 3)"""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    return dx * dx + dy * dy + dz * dz


def new_transform_2d(p1, p2, p3, p1p, p2p, p3p):
    """coord.go:118-137 on (x, y) pairs of float32: (six float32, ok); ok False is "divide by zero"."""
    (p1x, p1y), (p2x, p2y), (p3x, p3y) = [(F(p[0]), F(p[1])) for p in (p1, p2, p3)]
    (q1x, q1y), (q2x, q2y), (q3x, q3y) = [(F(p[0]), F(p[1])) for p in (p1p, p2p, p3p)]
    with np.errstate(all="ignore"):
        a = ((q3x - q1x) * (p2y - p1y) - (q2x - q1x) * (p3y - p1y)) / \
            ((p2y - p1y) * (p3x - p1x) - (p2x - p1x) * (p3y - p1y))
        b = ((q2x - q1x) - a * (p2x - p1x)) / (p2y - p1y)
        c = q1x - a * p1x - b * p1y
        d = ((q3y - q1y) * (p2y - p1y) - (q2y - q1y) * (p3y - p1y)) / \
            ((p2y - p1y) * (p3x - p1x) - (p2x - p1x) * (p3y - p1y))
        e = ((q2y - q1y) - d * (p2x - p1x)) / (p2y - p1y)
        f = q1y - d * p1x - e * p1y
    if np.isinf(a) or np.isinf(b) or np.isinf(d) or np.isinf(e):
        return np.zeros(6, F), False
    return np.array([a, b, c, d, e, f], F), True


def apply_transform(t, x, y):
    """coord.go:141-145"""
    with np.errstate(all="ignore"):
        return t[0] * x + t[1] * y + t[2], t[3] * x + t[4] * y + t[5]


def pick_brightest_distant(x, y, min_length, k):
    """align.go:86-104"""
    indices = []
    for s in range(len(x)):
        if len(indices) >= k:
            break
        picked = np.array(indices, np.int64)
        # the inner loop continues with the next star at the first picked one closer than minLength
        if picked.size and np.any(dist2d(x[s], y[s], x[picked], y[picked]) < min_length):
            continue
        indices.append(s)
    return np.array(indices, np.int32)


def generate_triangles(x, y, indices, scale_factor):
    """align.go:108-130: (dist (n, 3) float32 = dAB dAC dBC, abc (n, 3) int32) in the order of the three loops"""
    idx = np.asarray(indices, np.int64)
    m = idx.size
    sx, sy = x[idx] * F(scale_factor), y[idx] * F(scale_factor)
    d = dist2d(sx[:, None], sy[:, None], sx[None, :], sy[None, :]) if m else np.zeros((0, 0), F)   # d[i, j] = Dist2D(i, j)
    r = np.arange(m)
    a, b, c = r[:, None, None], r[None, :, None], r[None, None, :]
    dab, dac, dbc = d[:, :, None], d[:, None, :], d[None, :, :]
    keep = (a != b) & (a != c) & (b != c) & (dab < dac) & (dac < dbc)
    ia, ib, ic = np.nonzero(keep)                              # row-major: a outermost, c innermost
    dist = np.stack([d[ia, ib], d[ia, ic], d[ib, ic]], axis=1).astype(F).reshape(-1, 3)
    abc = np.stack([idx[ia], idx[ib], idx[ic]], axis=1).astype(np.int32).reshape(-1, 3)
    return dist, abc


class KDTree:
    """kdtree2.go (dims = 2) and kdtree3p.go (dims = 3): the points re-sorted in place into a pointerless tree, each
    with its payload -- for kdtree3p the triangle's index as there (align.go:67), for kdtree2 the star's index, which
    the reference does not keep (it returns the point; the index names it)."""

    def __init__(self, points):
        self.pts = np.array(points, F).reshape(len(points), -1) if len(points) else np.zeros((0, 1), F)
        self.dims = self.pts.shape[1] if len(points) else 0
        self.payload = np.arange(len(self.pts), dtype=np.int64)
        # Make, makeY (, makeZ): the same body on the next axis
        self._make_fns = [self._make_at(axis) for axis in range(self.dims)]
        self._nn_fns = [self._nearest_at(axis) for axis in range(self.dims)]
        if len(self.pts):
            self._make_fns[0](0, len(self.pts))

    def _make_at(self, axis):
        def make(lo, hi):                                      # kdtree2.go:31-43 / :47-59, kdtree3p.go:31-75
            order = np.argsort(self.pts[lo:hi, axis], kind="stable")
            self.pts[lo:hi] = self.pts[lo:hi][order]
            self.payload[lo:hi] = self.payload[lo:hi][order]
            n = hi - lo
            descend = self._make_fns[(axis + 1) % self.dims]
            if n > 1:                                          # descend left
                descend(lo, lo + n // 2)
                if n > 2:                                      # descend right
                    descend(lo + n // 2 + 1, hi)
        return make

    def _dsq(self, p, node):
        if self.dims == 2:
            return dist2d_squared(p[:, 0], p[:, 1], self.pts[node, 0], self.pts[node, 1])
        return dist3d_squared(p, self.pts[node])

    def _nearest_at(self, axis):
        def nearest(lo, hi, p):
            """kdtree2.go:63-93 / :95-125, kdtree3p.go:80-175 on the slice [lo, hi) for the queries p (n, dims):
            (closest node, closestDsq) per query"""
            n = hi - lo
            mid = lo + n // 2
            closest = np.full(len(p), mid, np.int64)
            closest_dsq = self._dsq(p, mid)
            descend = self._nn_fns[(axis + 1) % self.dims]
            left, right = (lo, mid), (mid + 1, hi)

            def visit(which, child):
                if which.size == 0:
                    return
                pt, dsq = descend(child[0], child[1], p[which])
                closer = dsq < closest_dsq[which]
                closest[which[closer]] = pt[closer]
                closest_dsq[which[closer]] = dsq[closer]

            def visit_behind_plane(which, child):
                dist_to_plane = p[which, axis] - self.pts[mid, axis]
                visit(which[dist_to_plane * dist_to_plane <= closest_dsq[which]], child)

            le = p[:, axis] <= self.pts[mid, axis]
            first, second = np.flatnonzero(le), np.flatnonzero(~le)
            # if p.X <= midpoint.X
            if n > 1:                                          # descend left
                visit(first, left)
                if n > 2:                                      # descend right
                    visit_behind_plane(first, right)
            # else
            if n > 2:                                          # descend right
                visit(second, right)
            if n > 1:                                          # descend left
                visit_behind_plane(second, left)
            return closest, closest_dsq
        return nearest

    def nearest_neighbor_recursive(self, p):
        """(payload, point, closestDsq) per row of p, by the recursive functions above"""
        p = np.asarray(p, F).reshape(-1, self.dims)
        with np.errstate(all="ignore"):
            node, dsq = self._nn_fns[0](0, len(self.pts), p)
        return self.payload[node], self.pts[node], dsq.astype(F)

    def nearest_neighbor(self, p):
        """The same searches with every query's recursion kept on a stack of its own and all queries stepped
        together (the recursive form starts a numpy call per node and batch: ten seconds for 19 600 queries).  Per
        query a frame is (lo, hi, phase, closestPt, closestDsq); phase 0 enters the function, 1 is back from the
        first child, 2 back from the second.  tests/test_align_ref.py holds it equal to the recursive form."""
        p = np.asarray(p, F).reshape(-1, self.dims)
        nq, depth = len(p), len(self.pts).bit_length() + 2
        lo_s, hi_s = np.zeros((nq, depth), np.int64), np.zeros((nq, depth), np.int64)
        phase_s, best_s, dsq_s = np.zeros((nq, depth), np.int8), np.zeros((nq, depth), np.int64), np.zeros((nq, depth), F)
        hi_s[:, 0] = len(self.pts)
        sp = np.zeros(nq, np.int64)
        ret_pt, ret_dsq = np.zeros(nq, np.int64), np.zeros(nq, F)
        with np.errstate(all="ignore"):
            while True:
                act = np.flatnonzero(sp >= 0)
                if act.size == 0:
                    break
                d = sp[act]
                lo, hi, phase = lo_s[act, d], hi_s[act, d], phase_s[act, d]
                n = hi - lo
                mid = lo + n // 2
                axis = d % self.dims
                pa, ma = p[act, axis], self.pts[mid, axis]
                le = pa <= ma                                  # if p.X <= midpoint.X
                closest, closest_dsq = best_s[act, d], dsq_s[act, d]
                enter = phase == 0                             # closestPt, closestDsq = midpoint, Dist(p, midpoint)
                closest[enter] = mid[enter]
                closest_dsq[enter] = self._dsq(p[act[enter]], mid[enter])
                closer = ~enter & (ret_dsq[act] < closest_dsq)   # if dsq < closestDsq { closestPt, closestDsq = pt, dsq }
                closest[closer] = ret_pt[act][closer]
                closest_dsq[closer] = ret_dsq[act][closer]
                has_first = np.where(le, n > 1, n > 2)         # left behind <=, else right
                has_second = np.where(le, n > 2, n > 1)
                to_first = enter & has_first
                dist_to_plane = pa - ma
                to_second = ((enter & ~has_first) | (phase == 1)) & has_second & \
                    (dist_to_plane * dist_to_plane <= closest_dsq)
                best_s[act, d], dsq_s[act, d] = closest, closest_dsq
                for go, next_phase, is_left in ((to_first, 1, le), (to_second, 2, ~le)):
                    g = np.flatnonzero(go)
                    a, dd, left = act[g], d[g], is_left[g]
                    phase_s[a, dd] = next_phase
                    lo_s[a, dd + 1] = np.where(left, lo[g], mid[g] + 1)
                    hi_s[a, dd + 1] = np.where(left, mid[g], hi[g])
                    phase_s[a, dd + 1] = 0
                    sp[a] = dd + 1
                r = np.flatnonzero(~(to_first | to_second))    # return closestPt, closestDsq
                ret_pt[act[r]], ret_dsq[act[r]], sp[act[r]] = closest[r], closest_dsq[r], d[r] - 1
        return self.payload[ret_pt], self.pts[ret_pt], ret_dsq


def brute_nearest(points, p, chunk=128):
    """(lowest index at the minimum, minimum dsq, number of points at the minimum) per row of p"""
    points, p = np.asarray(points, F), np.asarray(p, F)
    dims = points.shape[1]
    index = np.zeros(len(p), np.int64)
    best = np.zeros(len(p), F)
    count = np.zeros(len(p), np.int64)
    with np.errstate(all="ignore"):
        for s in range(0, len(p), chunk):
            q = p[s:s + chunk, None, :]
            if dims == 2:
                dsq = dist2d_squared(q[..., 0], q[..., 1], points[None, :, 0], points[None, :, 1])
            else:
                dsq = dist3d_squared(q, points[None, :, :])
            # a NaN never replaces the running minimum (dsq < closestDsq is false): it counts as +Inf
            key = np.where(np.isnan(dsq), F(np.inf), dsq)
            lo = key.min(axis=1)
            index[s:s + chunk] = np.argmax(key == lo[:, None], axis=1)
            count[s:s + chunk] = (key == lo[:, None]).sum(axis=1)
            best[s:s + chunk] = lo
    return index, best, count


class RefAligner:
    """NewAligner (align.go:58-71)"""

    def __init__(self, ref_width, ref_height, x, y, k):
        self.naxisn = (int(ref_width), int(ref_height))
        self.x, self.y = np.asarray(x, F), np.asarray(y, F)
        self.k = int(k)
        self.stars_2dt = KDTree(np.stack([self.x, self.y], axis=1))
        self.min_length = F(self.naxisn[1]) * MIN_DISTANCE_FOR_ALIGNMENT_STARS
        self.picked = pick_brightest_distant(self.x, self.y, self.min_length, self.k)
        self.tri_dist, self.tri_abc = generate_triangles(self.x, self.y, self.picked, F(1.0))
        self.ref_tri_3dt = KDTree(self.tri_dist)

    def nearest_stars(self, px, py, path):
        """(index of the reference star or -1, dsq, ties) per projected star (align.go:199-205)"""
        p = np.stack([px, py], axis=1).astype(F)
        if path == "kdtree":
            index, _, dsq = self.stars_2dt.nearest_neighbor(p)
            ties = 0
        else:
            index, dsq, count = brute_nearest(np.stack([self.x, self.y], axis=1), p)   # (a NaN dsq comes as +Inf)
            ties = int(((count > 1) & (dsq < DIST_SQUARED_LIMIT)).sum())
        with np.errstate(all="ignore"):
            matched = dsq < DIST_SQUARED_LIMIT
        return np.where(matched, index, -1).astype(np.int32), dsq, ties

    def match_stars(self, transforms, x, y, path="kdtree"):
        """align.go:194-206 per transform: (ref_index (n, stars), num_matches (n,), ties)"""
        x, y = np.asarray(x, F), np.asarray(y, F)
        rows, ties = [], 0
        for t in np.asarray(transforms, F).reshape(-1, 6):
            px, py = apply_transform(t, x, y)
            index, _, n = self.nearest_stars(px, py, path)
            rows.append(index)
            ties += n
        ref_index = np.array(rows, np.int32).reshape(len(rows), len(x))
        return ref_index, (ref_index >= 0).sum(axis=1).astype(np.int32), ties

    def align(self, frame_width, x, y, path="kdtree"):
        """Align (align.go:74-83) up to the minimiser, every candidate evaluated.  A dict of arrays: picked,
        scale_factor, triangles (tri_dist (n, 3), tri_abc (n, 3)), the matches in front of the sort (match_dist,
        match_ref), and per shortlisted candidate dist, tri_index, ref_tri_index, abc, ref_abc, trans, trans_ok,
        num_matches, enough, ref_index; ties = the places where the reference's outcome depends on Go's sort."""
        x, y = np.asarray(x, F), np.asarray(y, F)
        out = {}
        scale_factor = F(self.naxisn[0]) / F(int(frame_width))                       # :78
        picked = pick_brightest_distant(x, y, self.min_length, self.k)               # :75-76
        tri_dist, tri_abc = generate_triangles(x, y, picked, scale_factor)
        out.update(picked=picked, scale_factor=scale_factor, tri_dist=tri_dist, tri_abc=tri_abc)
        n_stars, n_tris, ties = len(x), len(tri_dist), 0
        empty = dict(match_dist=np.zeros(0, F), match_ref=np.zeros(0, np.int32), dist=np.zeros(0, F),
                     tri_index=np.zeros(0, np.int32), ref_tri_index=np.zeros(0, np.int32),
                     abc=np.zeros((0, 3), np.int32), ref_abc=np.zeros((0, 3), np.int32), trans=np.zeros((0, 6), F),
                     trans_ok=np.zeros(0, np.int32), num_matches=np.zeros(0, np.int32), enough=np.zeros(0, np.int32),
                     ref_index=np.zeros((0, n_stars), np.int32), ties=0)
        if n_tris == 0:                                        # no match: the zero transform and MaxFloat32
            out.update(empty)
            return out
        if len(self.tri_dist) == 0:
            raise IndexError("index out of range [0] with length 0 (kdtree3p.go:82)")

        # closestTriangleMatches (:133-156)
        if path == "kdtree":
            match_ref, _, match_dist = self.ref_tri_3dt.nearest_neighbor(tri_dist)
            order = np.argsort(match_dist, kind="stable")      # sort.Slice by Dist, taken as stable
        else:
            match_ref, match_dist, count = brute_nearest(self.tri_dist, tri_dist)
            ties += int((count > 1).sum())
            order = np.lexsort((np.arange(n_tris), match_dist))                       # (dist, lowest tri index)
        k = min(self.k, n_tris)                                # :148-149
        # equal distances that reach into the shortlist: their order is sort.Slice's
        head = match_dist[order][:k + 1]
        ties += int((head[1:] == head[:-1]).sum())
        shortlist = order[:k]
        out.update(match_dist=match_dist.astype(F), match_ref=match_ref.astype(np.int32))

        # findBestMatch (:159-212) in front of the minimiser
        res = {key: [] for key in ("dist", "tri_index", "ref_tri_index", "abc", "ref_abc", "trans", "trans_ok",
                                   "num_matches", "enough", "ref_index")}
        for ti in shortlist:
            abc, ref_abc = tri_abc[ti], self.tri_abc[match_ref[ti]]
            p = [(x[i], y[i]) for i in abc]
            pp = [(self.x[i], self.y[i]) for i in ref_abc]
            trans, ok = new_transform_2d(p[0], p[1], p[2], pp[0], pp[1], pp[2])
            if ok:
                px, py = apply_transform(trans, x, y)
                ref_index, _, n = self.nearest_stars(px, py, path)
                ties += n
            else:                                              # err != nil: continue
                ref_index = np.full(n_stars, -1, np.int32)
            num_matches = int((ref_index >= 0).sum())
            for key, value in (("dist", match_dist[ti]), ("tri_index", ti), ("ref_tri_index", match_ref[ti]),
                               ("abc", abc), ("ref_abc", ref_abc), ("trans", trans), ("trans_ok", int(ok)),
                               ("num_matches", num_matches),
                               ("enough", int(ok and num_matches >= n_stars // 3)),  # :210
                               ("ref_index", ref_index)):
                res[key].append(value)
        for key, value in res.items():
            out[key] = np.array(value, empty[key].dtype).reshape((len(shortlist),) + empty[key].shape[1:])
        out["ties"] = ties
        return out


def _bits(v):
    v = np.asarray(v)
    return v.view(np.uint32) if v.dtype == F else v


def compare(a, b):
    """The keys in which two results of align() differ in any bit"""
    return [key for key in a if key != "ties" and not np.array_equal(_bits(a[key]), _bits(b[key]))]


def make_case(seed, n_ref, width=1200, height=900, angle=0.01, shift=(7.3, -4.6), scale=1.0, drop=0.1, add=0.1,
              frame_width=None, jitter=0.2, close=0):
    """A reference frame of n_ref stars at random non-integer fp32 positions (brightest first: the order they come in)
    and a light frame made from it by a small rotation, shift and scale about the centre, with a fraction of the
    stars dropped, as many random ones added at random ranks, and every position jittered.  frame_width: the light
    frame's width where it is binned against the reference (coordinates shrink with it).
    Returns (ref_x, ref_y, x, y, frame_width)."""
    rng = np.random.RandomState(seed)
    ref_x = (rng.uniform(0.0, width, n_ref)).astype(F)
    ref_y = (rng.uniform(0.0, height, n_ref)).astype(F)
    for i in range(close):
        r, phi = rng.uniform(5.0, 30.0), rng.uniform(0.0, 2.0 * np.pi)
        ref_x = np.insert(ref_x, 2 * i + 1, F(ref_x[2 * i] + r * np.cos(phi)))
        ref_y = np.insert(ref_y, 2 * i + 1, F(ref_y[2 * i] + r * np.sin(phi)))
    n_ref = ref_x.size
    frame_width = width if frame_width is None else int(frame_width)
    shrink = frame_width / width
    keep = rng.uniform(size=n_ref) >= drop
    if keep.sum() < min(n_ref, 3):
        keep[:] = True
    cx, cy = width / 2.0, height / 2.0
    dx, dy = ref_x[keep].astype(np.float64) - cx, ref_y[keep].astype(np.float64) - cy
    c, s = np.cos(angle) * scale, np.sin(angle) * scale
    x = (cx + c * dx - s * dy + shift[0] + rng.normal(0.0, jitter, dx.size)) * shrink
    y = (cy + s * dx + c * dy + shift[1] + rng.normal(0.0, jitter, dx.size)) * shrink
    for _ in range(int(round(add * n_ref))):
        at = rng.randint(0, x.size + 1)
        x = np.insert(x, at, rng.uniform(0.0, width) * shrink)
        y = np.insert(y, at, rng.uniform(0.0, height) * shrink)
    return ref_x, ref_y, x.astype(F), y.astype(F), frame_width
