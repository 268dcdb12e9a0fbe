"""GPU: a pass's result and counters depend on the frames, weights, mode and sigmas alone -- never on what the handle or
the process ran before.  nlstack_pass.hip carries state from pass to pass (list-length hints per handle and per
geometry, two alternating scratch sets with their clean / dirty bookkeeping, lazily made buffers that outlive a change
of the active frame count); the other parity tests make a fresh handle per pass and never drive it.  Here one handle
lives through stale hints in both directions, queued passes, walks over engines, weights, frame counts and developer
switches, failures in between -- alone and as tiles of a group -- and EVERY pass is held to the project's bar against
the CPU oracle on the same frames: clip counters equal (modes 2 ... 5), values bit-exact for median, mean, linear fit,
weighted passes and every nl_stack_set_exact flavour, within RTOL with the oracle's NaN pattern for the default
dispatch of sigma, winsorized and MAD clipping.  Second, weaker: its bits and counters are those of the same pass run
alone on a fresh handle without shared hints (developer switch 512)."""
import collections

import numpy as np
import pytest

from test_gpu_parity import DISPATCH_TABLE
from util import RTOL, bits_equal, close_values, describe_mismatch, make_frames, same_values

pytestmark = pytest.mark.gpu

assert RTOL == 1e-5         # the bar of close_values below

NO_SHARED_HINTS = 512       # developer switch: no list-length hints from earlier handles of the same geometry
SIGMAS = (3.0, 2.5)

# protocol bits (nl_stack_last_pass_protocol) the second pass of a handle reports, as test_dispatch_table pins them
PINNED = {(m, k): proto for m, k, weighted, exact, flags, _, proto in DISPATCH_TABLE if not weighted and exact == 0 and flags == 0}

# the smallest tile on which every tail path of a sigma / winsorized fast pass runs (TAIL_ORDER_ROWS): rows 0 ... 16 of a
# 4096-high image; the tile of the walks: the shape of test_generic_pass_and_first_replay_in_one_launch
Geometry = collections.namedtuple("Geometry", "width height rows")
TILE = Geometry(4096, 4096, 16)
WALK = Geometry(640, 24, 24)

Pass = collections.namedtuple("Pass", "bits counters protocol exact_list generic_list")


def weights_of(name, n):
    if name is None:
        return None
    if name == "a":
        return np.linspace(0.2, 1.0, n).astype(np.float32)
    assert name == "b"
    return (0.25 + 0.75 * ((np.arange(n) * 37 % 101) / 100.0)).astype(np.float32)


def upload(st, frames):
    for i, f in enumerate(frames):
        st.upload_tile(i, f)


class History:
    """Runs passes and holds them to the bar; oracle results and the results of passes run alone are computed once per
    (data set, mode, frames, weights, sigmas, flavour) and never changed."""

    def __init__(self, nl, oracle):
        self.nl, self.oracle = nl, oracle
        self._want, self._alone, self._out, self._data = {}, {}, {}, {}

    def data(self, name, make):
        if name not in self._data:
            frames = make()
            if isinstance(frames, np.ndarray):
                frames.setflags(write=False)
            self._data[name] = frames
        return self._data[name]

    def open(self, capacity, geom):
        return self.nl.StackHandle(capacity, geom.width, geom.height, row0=0, rows=geom.rows)

    def run(self, st, mode, sl, sh):
        """one finished pass on st: (bits of the result tile, counters)"""
        key = (st.width, st.height)
        if key not in self._out:
            self._out[key] = np.zeros(st.width * st.height, np.float32)
        out = self._out[key]
        _, cl, ch = st.run(mode, sl, sh, 0.0, out=out)
        return out[:st.tile_pixels].copy(), (cl, ch)

    def want(self, data, frames, mode, sl, sh, wname):
        n = frames.shape[0]
        if mode in (0, 5):
            wname = None                     # the reference computes the weights, then does not pass them
        key = (data, mode, n, wname, sl, sh)
        if key not in self._want:
            rc, want, wl, wh, _ = self.oracle.stack_apply(mode, frames, weights_of(wname, n), sl, sh, 0.0, num_cpu=16)
            assert rc == 0
            self._want[key] = (want, (wl, wh))
        return self._want[key]

    def alone(self, data, frames, geom, mode, sl, sh, wname, flavour):
        n = frames.shape[0]
        key = (data, mode, n, wname, sl, sh, flavour)
        if key not in self._alone:
            with self.open(n, geom) as st:
                upload(st, frames)
                st.set_weights(weights_of(wname, n))
                st.set_exact(flavour)
                st.set_dev_flags(NO_SHARED_HINTS)
                self._alone[key] = self.run(st, mode, sl, sh)
        return self._alone[key]

    def judge(self, got, gc, data, frames, mode, sl, sh, wname, flavour, what):
        """the oracle bar for a result (tile bits, counters) of a pass over `frames`"""
        want, wc = self.want(data, frames, mode, sl, sh, wname)
        if mode >= 2:
            assert gc == wc, "%s: clip counters %r vs oracle %r" % (what, gc, wc)
        exact = mode in (0, 1, 5) or wname is not None or flavour != 0
        assert (same_values if exact else close_values)(got, want), "%s: %s" % (what, describe_mismatch(got, want))

    def check(self, st, geom, data, frames, mode, sl, sh, wname=None, flavour=0, what=""):
        """one pass on st, held to the oracle bar and to the same pass run alone; st is set up by the caller"""
        what = "%s mode %d n %d weights %r flavour %d sigmas %r on %s" % (what, mode, frames.shape[0], wname, flavour, (sl, sh), data)
        got, gc = self.run(st, mode, sl, sh)
        p = Pass(got, gc, st.last_pass_protocol, st.last_fallback_pixels, st.last_generic_pixels)
        self.judge(got, gc, data, frames, mode, sl, sh, wname, flavour, what)
        alone, ac = self.alone(data, frames, geom, mode, sl, sh, wname, flavour)
        assert gc == ac, "%s: clip counters %r, run alone %r" % (what, gc, ac)
        assert bits_equal(got, alone), "%s vs run alone: %s" % (what, describe_mismatch(got, alone))
        return p


@pytest.fixture(scope="module")
def history(nl, oracle):
    return History(nl, oracle)


# ---- 1. stale hints, both directions -----------------------------------------------------------------------------------
HINT_ROWS = [(2, 24), (3, 24), (3, 48), (2, 100), (2, 128), (3, 128), (2, 300), (3, 300)]
QUIET_MOST = 512            # exact list of a quiet pass: the fused protocol and the one-launch tail want <= 512
LOUD_LEAST = 4096           # lists of a loud pass: 5 x the largest clamped replay grid (768), 8 x the protocol thresholds
LOUD_PIXELS = 8192


def quiet_frames(history, n):
    """no missing samples, no border, no hot or cold pixels: next to nothing is handed over"""
    tile = history.data("quiet", lambda: make_frames(300, TILE.width, TILE.rows, seed=9100, nan_frac=0.0, hot=0.0, cold=0.0,
                                                     nan_border=False, all_nan_patch=False))
    return tile[:n]


def loud_frames(history, n):
    """the quiet frames with hand-overs built in: one infinite sample (alternating sign, walking through the frames) in
    every 8th pixel -- infinite samples go to the exact list -- and 10 missing samples (more than kPadMax = 8: the zonal
    kernels hand such a pixel to the generic pass) in 8 192 pixels between them"""
    def make():
        f = quiet_frames(history, n).copy()
        i = np.arange(LOUD_PIXELS)
        f[i % n, 8 * i] = np.where(i & 1, -np.inf, np.inf).astype(np.float32)
        for j in range(10):
            f[(i + j) % n, 8 * i + 4] = np.nan
        return f
    return history.data("loud%d" % n, make)


def hint_data(history, name, n):
    return quiet_frames(history, n) if name == "quiet" else loud_frames(history, n)


def check_lists(p, name, what):
    print("%s %s: protocol %d, exact list %d, generic list %d, counters %r" % (what, name, p.protocol, p.exact_list, p.generic_list, p.counters))
    if name == "quiet":
        assert p.exact_list <= QUIET_MOST, "%s: quiet exact list of %d pixels" % (what, p.exact_list)
    else:
        assert p.exact_list >= LOUD_LEAST, "%s: loud exact list of %d pixels" % (what, p.exact_list)
        assert p.generic_list >= LOUD_LEAST, "%s: loud generic list of %d pixels" % (what, p.generic_list)


def short_hint_protocol(history, mode, n, seen):
    """The protocol bits a pass dispatched on a short hint must report: what test_dispatch_table pins for the row -- where
    that pin was itself taken on a short hint.  The table's frames (fill_synthetic(3), same tile, same sigmas) are run
    here as the table runs them; a row whose exact list there is longer than QUIET_MOST (the winsorized 48-frame row:
    pinned 0, the protocol of a LONG hint) pins nothing about a short one, and what is asked of the pass is the fused
    bit: a handle without a hint, or with a long one, never reports it.  A row the table does not hold: as seen."""
    if (mode, n) not in PINNED:
        return seen
    def table_pass():
        with history.open(n, TILE) as st:
            st.fill_synthetic(3)
            st.set_dev_flags(NO_SHARED_HINTS)
            for _ in range(2):
                st.run(mode, *SIGMAS, fetch=False)
            return st.last_pass_protocol, st.last_fallback_pixels
    proto, listed = history.data(("table", mode, n), table_pass)
    assert proto == PINNED[(mode, n)], "mode %d n %d: the table's own pass ran protocol %d" % (mode, n, proto)
    print("mode %d n %d: the dispatch table's pass: protocol %d on an exact list of %d pixels" % (mode, n, proto, listed))
    if listed <= QUIET_MOST:
        return proto
    assert not proto & 1
    return seen | 1


def two_then_two(history, mode, n, first, second):
    """`first` twice, `second` uploaded into the same slots twice: the third pass is dispatched on the hint the second
    left -- of the other data set -- and must report the second's protocol bits"""
    what = "mode %d n %d %s->%s" % (mode, n, first, second)
    passes = []
    with history.open(n, TILE) as st:
        for k, name in enumerate((first, first, second, second)):
            if k in (0, 2):
                upload(st, hint_data(history, name, n))
            p = history.check(st, TILE, name, hint_data(history, name, n), mode, *SIGMAS, what="%s pass %d" % (what, k))
            check_lists(p, name, "%s pass %d" % (what, k))
            passes.append(p)
    assert passes[2].protocol == passes[1].protocol, "%s: the third pass ran protocol %d, the second %d" % (what, passes[2].protocol, passes[1].protocol)
    return passes


@pytest.mark.parametrize("mode,n", HINT_ROWS)
def test_hint_too_small_on_the_same_handle(history, mode, n):
    passes = two_then_two(history, mode, n, "quiet", "loud")
    assert passes[1].protocol == short_hint_protocol(history, mode, n, passes[1].protocol), "second quiet pass: protocol %d" % passes[1].protocol


@pytest.mark.parametrize("mode,n", HINT_ROWS)
def test_hint_too_large_on_the_same_handle(history, mode, n):
    two_then_two(history, mode, n, "loud", "quiet")


@pytest.mark.parametrize("first,second", [("quiet", "loud"), ("loud", "quiet")])
@pytest.mark.parametrize("mode,n", HINT_ROWS)
def test_hint_from_the_process_table(history, mode, n, first, second):
    """handle A finishes passes on `first` and is closed; handle B of the same geometry starts from what A saw"""
    what = "mode %d n %d table %s->%s" % (mode, n, first, second)
    with history.open(n, TILE) as a:
        upload(a, hint_data(history, first, n))
        for k in range(2):
            pa = history.check(a, TILE, first, hint_data(history, first, n), mode, *SIGMAS, what="%s A%d" % (what, k))
            check_lists(pa, first, "%s A%d" % (what, k))
    with history.open(n, TILE) as b:
        upload(b, hint_data(history, second, n))
        pb = history.check(b, TILE, second, hint_data(history, second, n), mode, *SIGMAS, what="%s B" % what)
        check_lists(pb, second, "%s B" % what)
    # B's first pass runs what A's second pass ran: it inherited A's hint (a handle without one runs protocol 0)
    assert pb.protocol == pa.protocol, "%s: B ran protocol %d, A %d" % (what, pb.protocol, pa.protocol)
    if first == "quiet":
        assert pb.protocol == short_hint_protocol(history, mode, n, pb.protocol), "%s: B ran protocol %d" % (what, pb.protocol)


@pytest.mark.parametrize("mode,n", HINT_ROWS)
def test_queued_passes_share_the_hint_of_the_pass_before_the_queue(history, mode, n):
    """three passes enqueued without a finish in between -- kappa 3, 0.8, 3 -- all sized by the hint of the one finished
    pass before them.  kappa 0.8 clips more samples per side than a zone holds almost everywhere: the middle pass's own
    lists are long (asserted below, in a pass of its own) although the frames stay what they were."""
    what = "mode %d n %d queued" % (mode, n)
    frames = quiet_frames(history, n)
    with history.open(n, TILE) as st:
        upload(st, frames)
        p = history.check(st, TILE, "quiet", frames, mode, 3.0, 3.0, what=what + " first")
        check_lists(p, "quiet", what + " first")
        for kappa in (3.0, 0.8, 3.0):
            st.run_async(mode, kappa, kappa, 0.0)
        out = np.zeros(TILE.width * TILE.height, np.float32)
        gc = st.finish(out)
        got = out[:st.tile_pixels]
        history.judge(got, gc, "quiet", frames, mode, 3.0, 3.0, None, 0, what + " last of the queue")
        assert gc == p.counters and bits_equal(got, p.bits), "%s: %s" % (what, describe_mismatch(got, p.bits))
        check_lists(Pass(got, gc, st.last_pass_protocol, st.last_fallback_pixels, st.last_generic_pixels), "quiet", what + " last of the queue")
        # the middle pass by itself, dispatched on the short hint the queue's last pass left
        mid = history.check(st, TILE, "quiet", frames, mode, 0.8, 0.8, what=what + " kappa 0.8")
        print("%s kappa 0.8: protocol %d, exact list %d, generic list %d" % (what, mid.protocol, mid.exact_list, mid.generic_list))
        assert mid.exact_list + mid.generic_list >= LOUD_LEAST, "%s: kappa 0.8 listed %d + %d pixels" % (what, mid.exact_list, mid.generic_list)
        history.check(st, TILE, "quiet", frames, mode, 3.0, 3.0, what=what + " after kappa 0.8")


# ---- 4. order independence of the suite --------------------------------------------------------------------------------
def test_evicting_the_geometry_from_the_hint_table_changes_nothing(history, nl):
    """the stale-hint sequence of the headline row twice; in between, 33 passes of other geometries (one more than the
    process-wide hint table holds) evict the row's entry: the second time round starts without a hint"""
    first = two_then_two(history, 2, 128, "quiet", "loud")
    for i in range(33):
        with nl.StackHandle(9 + i, 64, 2) as st:
            st.fill_synthetic(i)
            st.run(2, *SIGMAS, fetch=False)
    second = two_then_two(history, 2, 128, "quiet", "loud")
    for k, (a, b) in enumerate(zip(first, second)):
        assert a.counters == b.counters and bits_equal(a.bits, b.bits), "pass %d: %s" % (k, describe_mismatch(a.bits, b.bits))


# ---- 2. a walk over engines, weights and frame counts on one handle ---------------------------------------------------------
# Steps: ("n", k) nl_stack_set_active_frames, ("w", name) weights (None: off), ("x", flavour) nl_stack_set_exact,
# ("f", flags) developer switches, ("p", mode[, "fused"]) one pass with SIGMAS held to the bar ("fused": it must report
# the fused protocol), ("fail", mode, error) a pass that must fail.
F = ("p", 2, "fused")       # a sigma fast pass of 128 frames in the fused protocol
RESET = [("w", None), ("x", 0), ("f", 0)]
AT_128 = RESET + [("n", 128), ("p", 2)]              # ... and a pass that leaves a hint of this frame count


def n_change(k, mode):
    # weights on before the change: the change drops them, the mean pass behind it must be the unweighted mean; the
    # default-dispatch pass in front of it runs on a hint from another frame count
    return [("w", "a"), ("n", k), ("p", mode), ("p", 1)]


WALK_300 = {
    # every dispatch boundary (8 | 9, 24 | 25, 64 | 65, 128 | 129, 256 | 257) crossed going up and going down
    "frame counts": RESET + [("n", 300), ("p", 2)] + n_change(5, 2) + n_change(257, 3) + n_change(8, 3) + n_change(256, 2) +
                    n_change(9, 2) + n_change(129, 3) + n_change(24, 3) + n_change(128, 2) + n_change(25, 2) + n_change(100, 3) +
                    n_change(64, 2) + n_change(65, 3) + n_change(300, 3),
    # every engine family right behind and right in front of a fused sigma fast pass
    "families": AT_128 + [F, ("p", 1), F, ("p", 0), F, F, ("p", 3), F, ("p", 4), F, ("p", 5), F,
                          ("w", "a"), ("p", 2), ("w", None), F, ("w", "a"), ("p", 3), ("w", None), F,
                          ("x", 1), ("p", 2), ("x", 0), F, ("x", 2), ("p", 2), ("x", 0), F, ("x", 3), ("p", 2), ("x", 0), F],
    # ... and some of the other pairs
    "other pairs": RESET + [("n", 64), ("p", 3), ("p", 4), ("p", 5), ("p", 0), ("p", 1), ("w", "b"), ("p", 3), ("p", 2), ("w", None),
                            ("x", 1), ("p", 3), ("x", 2), ("p", 3), ("x", 3), ("p", 3), ("x", 0), ("p", 4), ("p", 3)],
    # plain protocol: the reduction kernel leaves the scratch set zeroed, a mean pass keeps it so, a median pass does not
    "keep clean": AT_128 + [("f", 1), ("p", 2), ("p", 1), ("p", 2), ("p", 2), ("p", 0), ("p", 2), ("f", 0), ("p", 2)],
    "failures": AT_128 + [F, ("w", "a"), ("fail", 4, "ERR_WEIGHTED_MAD"), ("w", None), F, ("fail", 9, "ERR_INVALID_MODE"), F],
    # weights on -> off -> other weights at one frame count: the decision pass's bounds / rounds buffers are reused
    "weights": RESET + [("n", 128), ("w", "a"), ("p", 2), ("p", 3), ("w", None), ("p", 2), ("p", 3), ("w", "b"), ("p", 2), ("p", 3),
                        ("n", 300), ("w", "a"), ("p", 3), ("p", 2), ("w", None), ("p", 3), ("p", 2), ("w", "b"), ("p", 3), ("p", 2)],
    "switches": AT_128 + [("f", 1), ("p", 2), ("f", 0), ("p", 2), ("f", 2), ("p", 2), ("f", 0), ("p", 2), ("f", 32), ("p", 2), ("f", 0), ("p", 2),
                          ("f", 8192), ("p", 2), ("f", 0), ("p", 2), ("f", 16384), ("p", 3), ("f", 0), ("p", 3)],
    # the linear-fit cascade's state arrays were sized for the capacity's lane count
    "linear fit": RESET + [("n", 300), ("p", 5), ("n", 64), ("p", 2), ("p", 5), ("n", 200), ("p", 3), ("p", 5)],
}
WALK_128 = RESET + [("n", 128), ("p", 5), ("p", 2), F, ("n", 64), ("p", 5), F[:2], ("n", 20), ("p", 3), ("p", 1), ("n", 128), ("p", 5), ("p", 2), F]


def walk_frames(history):
    return history.data("walk", lambda: make_frames(300, WALK.width, WALK.height, seed=4300, nan_frac=0.03, ties=True))


class Walker:
    """a handle and what the walk has set on it"""

    def __init__(self, history, capacity):
        self.history, self.st = history, history.open(capacity, WALK)
        self.frames = walk_frames(history)
        upload(self.st, self.frames[:capacity])
        self.n, self.wname, self.flavour = capacity, None, 0

    def step(self, k, op):
        from nightlight_amd import capi
        h, st, what = self.history, self.st, "step %d %r" % (k, op)
        if op[0] == "n":
            st.set_active_frames(op[1])
            if op[1] != self.n:
                self.wname = None            # weights are per frame of a given batch: a change drops them
            self.n = op[1]
        elif op[0] == "w":
            st.set_weights(weights_of(op[1], self.n))
            self.wname = op[1]
        elif op[0] == "x":
            st.set_exact(op[1])
            self.flavour = op[1]
        elif op[0] == "f":
            st.set_dev_flags(op[1])
        elif op[0] == "p":
            mode = op[1]
            wname = self.wname if mode in (1, 2, 3) else None
            p = h.check(st, WALK, "walk", self.frames[:self.n], mode, *SIGMAS, wname=wname, flavour=self.flavour, what=what)
            print("%s: n %d weights %r flavour %d: %s, protocol %d, exact list %d, generic list %d" %
                  (what, self.n, wname, self.flavour, st.last_kernel_name, p.protocol, p.exact_list, p.generic_list))
            if len(op) > 2:
                assert p.protocol & 1, "%s: not a fused pass (protocol %d, exact list %d)" % (what, p.protocol, p.exact_list)
        else:
            assert op[0] == "fail"
            assert st.last_generic_pixels > 0, "%s: the pass before the failure listed nothing" % what
            with pytest.raises(capi.NlError) as e:
                st.run(op[1], *SIGMAS)
            assert e.value.code == getattr(capi, op[2]), what
            assert (st.last_fallback_pixels, st.last_generic_pixels) == (0, 0), "%s: a failed pass reports lists" % what

    def walk(self, ops):
        for k, op in enumerate(ops):
            self.step(k, op)


@pytest.fixture(scope="module")
def walker_300(history):
    w = Walker(history, 300)
    yield w
    w.st.close()


@pytest.mark.parametrize("leg", sorted(WALK_300))
def test_walk_on_one_handle_of_300_frames(walker_300, leg):
    # (one handle for every leg: what a leg leaves behind is history for the next; each leg sets what it relies on)
    walker_300.walk(WALK_300[leg])


def test_walk_on_one_handle_of_128_frames(history):
    # capacity 128: one liveness mask per pixel of the linear-fit cascade, another n_pad than the 300-frame handle's
    w = Walker(history, 128)
    try:
        w.walk(WALK_128)
    finally:
        w.st.close()


# ---- 3. the same through a group ----------------------------------------------------------------------------------------
GROUP_WALK = [(128, 2, None), (20, 3, None), (128, 2, "a"), (64, 5, None), (128, 2, None)]


def group_run(g, mode):
    got, cl, ch = g.run(mode, *SIGMAS)
    return got, (cl, ch)


def test_walk_through_a_group_of_three_tiles(history, nl):
    frames = walk_frames(history)[:128]
    alone = {}
    for n, mode, wname in GROUP_WALK:
        if (n, mode, wname) in alone:
            continue
        with nl.StackGroup(n, WALK.width, WALK.height, devices=[0, 0, 0]) as g:
            g.upload_frames(frames[:n])
            g.set_weights(weights_of(wname, n))
            for t in range(g.size):
                g.tile(t).set_dev_flags(NO_SHARED_HINTS)
            alone[(n, mode, wname)] = group_run(g, mode)
    with nl.StackGroup(128, WALK.width, WALK.height, devices=[0, 0, 0]) as g:
        assert g.size == 3
        g.upload_frames(frames)
        for k, (n, mode, wname) in enumerate(GROUP_WALK):
            what = "group step %d: n %d mode %d weights %r" % (k, n, mode, wname)
            if n != g.n_frames:
                g.set_weights(weights_of("b", g.n_frames))      # on before the change: the change drops them
            g.set_active_frames(n)
            if wname is not None:
                g.set_weights(weights_of(wname, n))
            got, gc = group_run(g, mode)
            history.judge(got, gc, "walk", frames[:n], mode, *SIGMAS, wname if mode in (1, 2, 3) else None, 0, what)
            a, ac = alone[(n, mode, wname)]
            assert gc == ac and bits_equal(got, a), "%s vs run alone: %s" % (what, describe_mismatch(got, a))
