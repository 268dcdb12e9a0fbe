"""Thin Python view of one nl_stack_t handle (include/nlstack.h).

Used by the tests, bench.py and the row-tile sharding helper; every method is
one C-ABI call.  Naming follows the reference's domain: frames, tiles, stack
passes, clip counters (internal/ops/stack/stack.go).
"""
import ctypes as C

import numpy as np

from . import capi


def _u16ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def _sigmas(sigma_low, sigma_high, ref_loc):
    return C.c_float(sigma_low), C.c_float(sigma_high), C.c_float(ref_loc)


def _run_counted(entry, ptr, lead, out):
    """One counted pass through `entry`, a pass entry of the library without maps, on the handle or group `ptr`:
    entry(ptr, *lead, out, &clip_low, &clip_high).  `out`: the whole-image float32 array the rows are written to, or
    None (the result stays on the device).  Returns (out, clip_low, clip_high)."""
    cl, ch = C.c_int64(0), C.c_int64(0)
    capi.check(entry(ptr, *lead, capi.fptr(out) if out is not None else None, C.byref(cl), C.byref(ch)))
    return out, cl.value, ch.value


def _run_maps(entry, ptr, n, lead, out=None, reject_low=None, reject_high=None):
    """One maps pass through `entry`, an nl_stack_run_maps* / nl_group_run_maps* function of the library, over an image
    of n pixels; the whole-image arrays not given are made here.  Returns (out, clip_low, clip_high, reject_low,
    reject_high)."""
    out = np.zeros(n, np.float32) if out is None else out
    reject_low = np.zeros(n, np.uint16) if reject_low is None else reject_low
    reject_high = np.zeros(n, np.uint16) if reject_high is None else reject_high
    for a, t in ((out, np.float32), (reject_low, np.uint16), (reject_high, np.uint16)):
        assert a.dtype == t and a.size == n and a.flags.c_contiguous
    cl, ch = C.c_int64(0), C.c_int64(0)
    capi.check(entry(ptr, *lead, capi.fptr(out), C.byref(cl), C.byref(ch), _u16ptr(reject_low), _u16ptr(reject_high)))
    return out, cl.value, ch.value, reject_low, reject_high


class StackHandle:
    """Frames of one row tile [row0, row0+rows) resident in HBM as planar
    [n_frames][rows*width] fp32, plus the result tile and clip counters."""

    def __init__(self, n_frames, width, height, row0=0, rows=None, device=0):
        self._lib = capi.load()
        rows = height - row0 if rows is None else rows
        self.n_frames, self.width, self.height = int(n_frames), int(width), int(height)
        self.row0, self.rows, self.device = int(row0), int(rows), int(device)
        self._h = self._lib.nl_stack_create(self.n_frames, self.width, self.height,
                                            self.row0, self.rows, self.device)
        if not self._h:
            raise capi.NlError(capi.ERR_HIP, capi.last_error())

    @classmethod
    def _borrow(cls, handle, n_frames, width, height, row0, rows):
        """View of a handle owned by someone else (a tile of an nl_group): never destroyed here."""
        self = cls.__new__(cls)
        self._lib = capi.load()
        self.n_frames, self.width, self.height = int(n_frames), int(width), int(height)
        self.row0, self.rows, self.device = int(row0), int(rows), -1
        self._h, self._borrowed = handle, True
        return self

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if self._h:
            if not getattr(self, "_borrowed", False):
                self._lib.nl_stack_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def tile_pixels(self):
        return self.rows * self.width

    # -- frames ------------------------------------------------------------
    def upload_frame(self, idx, frame):
        """frame: full image, width*height float32 (fits.Image.Data)."""
        frame = np.ascontiguousarray(frame, dtype=np.float32).reshape(-1)
        assert frame.size == self.width * self.height
        capi.check(self._lib.nl_stack_upload_frame(self._h, int(idx), capi.fptr(frame)))

    def upload_frame_async(self, idx, frame):
        """Overlapped upload through the pinned staging ring (frame = whole image)."""
        frame = np.ascontiguousarray(frame, dtype=np.float32).reshape(-1)
        assert frame.size == self.width * self.height
        capi.check(self._lib.nl_stack_upload_frame_async(self._h, int(idx), capi.fptr(frame)))

    def upload_wait(self):
        capi.check(self._lib.nl_stack_upload_wait(self._h))

    def upload_tile(self, idx, tile):
        tile = np.ascontiguousarray(tile, dtype=np.float32).reshape(-1)
        assert tile.size == self.tile_pixels
        capi.check(self._lib.nl_stack_upload_tile(self._h, int(idx), capi.fptr(tile)))

    def upload_frames(self, frames):
        for i, f in enumerate(frames):
            self.upload_frame(i, f)

    def download_tile(self, idx):
        out = np.empty(self.tile_pixels, np.float32)
        capi.check(self._lib.nl_stack_download_tile(self._h, int(idx), capi.fptr(out)))
        return out

    def download_rows(self, idx, first_row, n_rows):
        """Rows [first_row, first_row+n_rows) (tile-relative) of frame idx; idx=-1: of the result."""
        out = np.empty(int(n_rows) * self.width, np.float32)
        capi.check(self._lib.nl_stack_download_rows(self._h, int(idx), int(first_row), int(n_rows),
                                                    capi.fptr(out)))
        return out

    def fill_synthetic(self, seed=0x4E4C5354):
        capi.check(self._lib.nl_stack_fill_synthetic(self._h, C.c_uint64(seed)))

    @property
    def device_bytes(self):
        """Device memory the handle holds right now (create-time buffers + lazily allocated scratch)."""
        return int(self._lib.nl_stack_device_bytes(self._h))

    def frames_device_ptr(self):
        return self._lib.nl_stack_frames_device_ptr(self._h)

    def frame_stride(self):
        """Floats between consecutive frames of the buffer frames_device_ptr() points at."""
        return int(self._lib.nl_stack_frame_stride(self._h))

    def attach_device_frames(self, ptr, stride=None):
        """Lends a device buffer (None restores the owned one); `stride` in floats, default dense (rows*width)."""
        if stride is None or ptr is None:
            capi.check(self._lib.nl_stack_attach_device_frames(self._h, C.c_void_p(ptr)))
        else:
            capi.check(self._lib.nl_stack_attach_device_frames_strided(self._h, C.c_void_p(ptr), int(stride)))

    def set_active_frames(self, n):
        """Use frame slots [0, n) for the next uploads / passes (n <= the count given at creation)."""
        capi.check(self._lib.nl_stack_set_active_frames(self._h, int(n)))
        self.n_frames = int(n)

    def set_weights(self, weights):
        if weights is None:
            capi.check(self._lib.nl_stack_set_weights(self._h, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.float32)
        assert w.size == self.n_frames
        capi.check(self._lib.nl_stack_set_weights(self._h, capi.fptr(w)))

    # -- stack passes ------------------------------------------------------
    def run(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """One pass. Returns (result or None, clip_low, clip_high).  `out` is a
        full-image float32 array whose tile rows get written; with fetch=False
        the result stays on the device."""
        return _run_counted(self._lib.nl_stack_run, self._h, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(out, fetch))

    def _result_array(self, out, fetch):
        """Where a pass's rows go: `out`, a fresh whole-image array if none is given, None with fetch=False."""
        if not fetch:
            return None
        return np.zeros(self.width * self.height, np.float32) if out is None else out

    def run_maps(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, reject_low=None,
                 reject_high=None, fast=False):
        """One pass on the bit-exact column kernel that also says WHERE it clipped (include/nlstack_maps.h).
        fast=True: nl_stack_run_maps_fast (include/nlstack_fastmaps.h) -- the same maps from the default pass's
        engines where they exist (unweighted sigma / winsorized clipping up to 128 frames; the result is then the
        default pass's, not the bit-exact one), the column kernel everywhere else.
        Returns (result, clip_low, clip_high, reject_low, reject_high): the maps are whole-image uint16 arrays,
        reject_low[p] / reject_high[p] = how often the reference increments clipLow / clipHigh at pixel p; their
        sums are the two totals.  `out`, `reject_low`, `reject_high`: whole-image arrays (float32, uint16, uint16)
        whose tile rows get written; those not given are made here, zero outside the tile."""
        entry = self._lib.nl_stack_run_maps_fast if fast else self._lib.nl_stack_run_maps
        return self._run_maps(entry, mode, sigma_low, sigma_high, ref_loc, out, reject_low, reject_high)

    def _run_maps(self, entry, mode, sigma_low, sigma_high, ref_loc, out=None, reject_low=None, reject_high=None):
        return _run_maps(entry, self._h, self.width * self.height, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc),
                         out, reject_low, reject_high)

    def run_maps_resident(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, reject_low=None,
                          reject_high=None):
        """run_maps on the register-resident engines (nl_stack_run_maps_resident, include/nlstack_residentmaps.h):
        the linear fit of up to 512 frames on its own kernels and cascade -- the result is then bit-exact, the pass
        about as fast as run(ST_LINEAR_FIT) -- sigma / winsorized clipping as run_maps(fast=True), the column kernel
        everywhere else.  Arguments and return value are those of run_maps."""
        return self._run_maps(self._lib.nl_stack_run_maps_resident, mode, sigma_low, sigma_high, ref_loc, out, reject_low, reject_high)

    def run_maps_deep(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, reject_low=None,
                      reject_high=None):
        """run_maps_resident with the deep sigma / winsorized stacks on their own engines as well
        (nl_stack_run_maps_deep, include/nlstack_deepmaps.h): unweighted sigma / winsorized clipping of 129 ... 512
        frames on the LDS-column kernels of the default pass -- the result is then the default pass's -- and the pass
        of run_maps_resident everywhere else.  Arguments and return value are those of run_maps."""
        return self._run_maps(self._lib.nl_stack_run_maps_deep, mode, sigma_low, sigma_high, ref_loc, out, reject_low, reject_high)

    def run_maps_full(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, reject_low=None,
                      reject_high=None):
        """run_maps_deep with MAD sigma and the median on their own engines as well (nl_stack_run_maps_full,
        include/nlstack_fullmaps.h): unweighted MAD sigma of 1 ... 512 frames on the MAD kernels of the default pass --
        the result is then the default pass's, bit for bit -- the median on its default kernels with zero maps, and
        the pass of run_maps_deep everywhere else.  Arguments and return value are those of run_maps."""
        return self._run_maps(self._lib.nl_stack_run_maps_full, mode, sigma_low, sigma_high, ref_loc, out, reject_low, reject_high)

    def run_maps_deepstack(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, reject_low=None,
                           reject_high=None):
        """run_maps_full with the stacks beyond 512 frames on engines of their own as well (nl_stack_run_maps_deepstack,
        include/nlstack_deepstackmaps.h): unweighted MAD sigma of 513 ... 2048 frames on the 8- / 16-lane kernel of
        run_deepstack -- the result is then run_deepstack's, bit for bit, the maps run_maps' -- the median on its deep
        kernel with zero maps, unweighted sigma / winsorized clipping beyond 512 frames on the wave-per-pixel replay
        (result and maps are run_maps'), and the pass of run_maps_full everywhere else.  Arguments and return value are
        those of run_maps."""
        return self._run_maps(self._lib.nl_stack_run_maps_deepstack, mode, sigma_low, sigma_high, ref_loc, out, reject_low, reject_high)

    def run_linfit_weighted(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """One pass of the weighted linear fit (include/nlstack_wlinfit.h; an EXTENSION, the reference's fit takes
        no weights): the reference's linear-fit rejection, then the mean of the survivors with the weights of
        set_weights.  Returns (result or None, clip_low, clip_high) as run does; the counters are those of
        run(ST_LINEAR_FIT).  Without weights it raises NlError (ERR_INVALID_ARG)."""
        return _run_counted(self._lib.nl_stack_run_linfit_weighted, self._h, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(out, fetch))

    def run_linfit_weighted_async(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """run_linfit_weighted without the wait: finish() completes it."""
        capi.check(self._lib.nl_stack_run_linfit_weighted_async(self._h, C.c_float(sigma_low), C.c_float(sigma_high),
                                                                C.c_float(ref_loc)))

    def run_clip_weighted(self, mode=capi.ST_AUTO, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """One pass of weighted sigma / winsorized clipping whose weights follow their frames
        (include/nlstack_wclip.h; an EXTENSION: the reference multiplies a survivor by whichever weight its
        quickselect left in the survivor's slot): the reference's rejection, then the mean of the survivors, each
        with its own frame's weight of set_weights.  `mode` is ST_SIGMA, ST_WINSOR_SIGMA, or ST_AUTO where that
        resolves to one of them.  Returns (result or None, clip_low, clip_high) as run does; the counters are those of
        run(mode).  Without weights it raises NlError (ERR_INVALID_ARG)."""
        return _run_counted(self._lib.nl_stack_run_clip_weighted, self._h,
                            (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc), self._result_array(out, fetch))

    def run_clip_weighted_async(self, mode=capi.ST_AUTO, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """run_clip_weighted without the wait: finish() completes it."""
        capi.check(self._lib.nl_stack_run_clip_weighted_async(self._h, int(mode), C.c_float(sigma_low),
                                                              C.c_float(sigma_high), C.c_float(ref_loc)))

    def run_mad_weighted(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """One pass of weighted MAD-sigma stacking whose weights follow their frames (include/nlstack_wmad.h; an
        EXTENSION: the reference panics on MAD sigma with weights, and run(ST_MAD_SIGMA) with weights raises
        ERR_WEIGHTED_MAD): the reference's MAD-sigma rejection on the values alone, then the mean of the survivors
        in frame order, each with its own frame's weight of set_weights.  Returns (result or None, clip_low,
        clip_high) as run does; the counters are those of run(ST_MAD_SIGMA) without weights.  Without weights it
        raises NlError (ERR_INVALID_ARG)."""
        return _run_counted(self._lib.nl_stack_run_mad_weighted, self._h, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(out, fetch))

    def run_mad_weighted_async(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """run_mad_weighted without the wait: finish() completes it."""
        capi.check(self._lib.nl_stack_run_mad_weighted_async(self._h, C.c_float(sigma_low), C.c_float(sigma_high),
                                                             C.c_float(ref_loc)))

    def run_mad_weighted_deepstack(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """run_mad_weighted for deep stacks (include/nlstack_deepwmad.h; an extension of depth, not of semantics):
        513 ... 2048 active frames on the 8- / 16-lane MAD kernel, record only, and the streaming kernel of the weighted
        passes -- bit-equal to run_mad_weighted, the same counters -- and run_mad_weighted's own pass at every other
        depth.  Arguments and return value are those of run_mad_weighted."""
        return _run_counted(self._lib.nl_stack_run_mad_weighted_deepstack, self._h, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(out, fetch))

    def run_mad_weighted_deepstack_async(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """run_mad_weighted_deepstack without the wait: finish() completes it."""
        capi.check(self._lib.nl_stack_run_mad_weighted_deepstack_async(self._h, C.c_float(sigma_low), C.c_float(sigma_high),
                                                                       C.c_float(ref_loc)))

    def run_deepstack(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, out=None, fetch=True):
        """run for deep stacks (include/nlstack_deepstack.h; an extension of depth, not of semantics): the median and
        unweighted MAD sigma of 513 ... 2048 active frames on register-resident kernels with 8 or 16 lanes per pixel
        -- the median bit-equal to run(ST_MEDIAN), MAD sigma with run(ST_MAD_SIGMA)'s counters and the mean of the
        same survivors -- and run's own pass for every other mode and depth.  Arguments and return value are those
        of run."""
        return _run_counted(self._lib.nl_stack_run_deepstack, self._h, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(out, fetch))

    def run_deepstack_async(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """run_deepstack without the wait: finish() completes it."""
        capi.check(self._lib.nl_stack_run_deepstack_async(self._h, int(mode), C.c_float(sigma_low), C.c_float(sigma_high),
                                                          C.c_float(ref_loc)))

    def coverage(self, out=None):
        """Whole-image uint16 map of how many active frames have a sample (not NaN) at each pixel: the tile's rows
        of `out` (made here, zero outside the tile, if not given).  No pass: the last result stays."""
        out = np.zeros(self.width * self.height, np.uint16) if out is None else out
        assert out.dtype == np.uint16 and out.size == self.width * self.height and out.flags.c_contiguous
        capi.check(self._lib.nl_stack_coverage(self._h, _u16ptr(out)))
        return out

    @property
    def last_coverage_ms(self):
        """GPU time of the kernels of the last coverage() call; -1 before the first."""
        return float(self._lib.nl_stack_last_coverage_ms(self._h))

    def run_async(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        capi.check(self._lib.nl_stack_run_async(self._h, int(mode), C.c_float(sigma_low),
                                                C.c_float(sigma_high), C.c_float(ref_loc)))

    def finish(self, out=None):
        cl, ch = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_finish(self._h, capi.fptr(out) if out is not None else None,
                                             C.byref(cl), C.byref(ch)))
        return cl.value, ch.value

    def result_tile(self):
        """The result tile only (rows*width), downloaded from the device."""
        full = np.zeros(self.width * self.height, np.float32)
        self.finish(full)
        return full[self.row0 * self.width:(self.row0 + self.rows) * self.width].copy()

    def set_exact(self, on=True):
        """Force the bit-exact kernels (verification); default is the fast path."""
        capi.check(self._lib.nl_stack_set_exact(self._h, int(on)))

    def set_dev_flags(self, flags):
        """A/B switches of the fast path (include/nlstack.h: nl_stack_set_dev_flags)."""
        capi.check(self._lib.nl_stack_set_dev_flags(self._h, int(flags)))

    @property
    def last_fallback_pixels(self):
        return int(self._lib.nl_stack_last_fallback_pixels(self._h))

    @property
    def last_pass_protocol(self):
        """Bit 0: fused protocol, bit 1: generic pass + first replay in one launch (diagnostics)."""
        return int(self._lib.nl_stack_last_pass_protocol(self._h))

    @property
    def last_generic_pixels(self):
        return int(self._lib.nl_stack_last_generic_pixels(self._h))

    @property
    def linfit_stage_counts(self):
        """list lengths of the last linear-fit cascade (see include/nlstack.h); [] if none ran"""
        buf = (C.c_uint * 8)()
        k = int(self._lib.nl_stack_linfit_stage_counts(self._h, buf, 8))
        return [int(buf[i]) for i in range(max(k, 0))]

    @property
    def last_mode(self):
        return self._lib.nl_stack_last_mode(self._h)

    @property
    def last_kernel_ms(self):
        return float(self._lib.nl_stack_last_kernel_ms(self._h))

    @property
    def last_dominant_kernel_ms(self):
        return float(self._lib.nl_stack_last_dominant_kernel_ms(self._h))

    @property
    def last_kernel_name(self):
        return self._lib.nl_stack_last_kernel_name(self._h).decode()

    def pass_times(self, back=0):
        """(pass ms, dominant-kernel ms) of the pass enqueued `back` passes ago, from the
        handle's ring of HIP events -- no host sync was needed while the passes were queued."""
        p, d = C.c_float(), C.c_float()
        capi.check(self._lib.nl_stack_pass_times(self._h, int(back), C.byref(p), C.byref(d)))
        return float(p.value), float(d.value)

    @property
    def stream_ptr(self):
        """hipStream_t of the handle as an integer (torch.cuda.ExternalStream takes it)."""
        return int(self._lib.nl_stack_stream(self._h) or 0)

    def copy_counters_async(self, device_ptr):
        """Enqueue a copy of the last pass's counters to a device buffer (2 x int64) on the handle's stream."""
        capi.check(self._lib.nl_stack_copy_counters_async(self._h, C.c_void_p(int(device_ptr))))

    def set_counters_buffer(self, device_ptr):
        """Passes enqueued from now on leave their counters in the caller's device buffer (32 bytes; None: the handle's own)."""
        capi.check(self._lib.nl_stack_set_counters_buffer(self._h, C.c_void_p(int(device_ptr)) if device_ptr else None))

    def order_stream_after(self, hip_stream):
        """`hip_stream` (integer hipStream_t) waits for everything enqueued on the handle so far."""
        capi.check(self._lib.nl_stack_order_stream_after(self._h, C.c_void_p(int(hip_stream))))

    @property
    def counters_device_ptr(self):
        """Device address of the last pass's {clip_low, clip_high} (2 x int64)."""
        return int(self._lib.nl_stack_counters_device_ptr(self._h) or 0)

    def find_sigmas(self, mode, clip_perc_low, clip_perc_high, ref_loc=0.0, reduce=None,
                    fetch=True):
        """Goal-seek bisection (stackfindsigma.go:48-98).  `reduce(lo, hi) ->
        (lo, hi)` maps this tile's counters to the totals over all tiles."""
        cl, ch = C.c_int64(0), C.c_int64(0)
        sl, sh, passes = C.c_float(), C.c_float(), C.c_int()
        out = np.zeros(self.width * self.height, np.float32) if fetch else None

        def _cb(counters, _user):
            try:
                lo, hi = reduce(int(counters[0]), int(counters[1]))
                counters[0], counters[1] = int(lo), int(hi)
                return 0
            except Exception:   # never unwind through the C frame
                return 1

        cb = capi.REDUCE_FN(_cb) if reduce is not None else C.cast(None, capi.REDUCE_FN)
        capi.check(self._lib.nl_stack_find_sigmas(
            self._h, int(mode), C.c_float(ref_loc), C.c_float(clip_perc_low),
            C.c_float(clip_perc_high), cb, None, capi.fptr(out) if fetch else None,
            C.byref(cl), C.byref(ch), C.byref(sl), C.byref(sh), C.byref(passes)))
        return out, cl.value, ch.value, float(sl.value), float(sh.value), passes.value

    # -- stack of stacks ---------------------------------------------------
    def accumulate(self, weight, first):
        capi.check(self._lib.nl_stack_accumulate(self._h, C.c_float(weight), int(bool(first))))

    def accumulate_finalize(self, weight_sum):
        out = np.zeros(self.width * self.height, np.float32)
        capi.check(self._lib.nl_stack_accumulate_finalize(self._h, C.c_float(weight_sum),
                                                          capi.fptr(out)))
        return out

    # -- per-frame statistics ----------------------------------------------
    def frame_stats(self, idx, variance=True):
        mn, mean, mx = C.c_float(), C.c_float(), C.c_float()
        var = C.c_double()
        capi.check(self._lib.nl_stack_frame_stats(self._h, int(idx), C.byref(mn), C.byref(mean),
                                                  C.byref(mx), C.byref(var) if variance else None))
        return (np.float32(mn.value), np.float32(mean.value), np.float32(mx.value),
                float(var.value) if variance else None)

    def frame_location_scale(self, idx, estimator=capi.LSE_SC_MEDIAN_QN, seeds=None, num_samples=capi.LOCSCALE_SAMPLES,
                             min_max=None):
        """Stats.Location() / Scale() of resident slot idx of a whole-image handle (idx < 0: of the last pass's
        result), see location_scale.  Returns (location, scale, info)."""
        return _location_scale(lambda *a: self._lib.nl_stack_frame_location_scale(self._h, int(idx), *a), estimator,
                               seeds, num_samples, min_max)

    def frame_noise(self, idx):
        v = C.c_float()
        capi.check(self._lib.nl_stack_frame_noise(self._h, int(idx), C.byref(v)))
        return np.float32(v.value)

    def weights_from_noise(self):
        noise = np.zeros(self.n_frames, np.float32)
        capi.check(self._lib.nl_stack_weights_from_noise(self._h, capi.fptr(noise)))
        return noise


    # ---- formats and steps either side of the stack (include/nlstack.h, F3 / F4) ----
    def upload_frame_fits(self, idx, raw, bitpix, bscale=1.0, bzero=0.0, multiplier=1.0, offset=0.0):
        """Big-endian FITS payload bytes of this handle's tile -> frame slot idx,
        decoded on the device; returns (min, max, mean) of the decoded tile."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        stats = np.zeros(3, np.float32)
        capi.check(self._lib.nl_stack_upload_frame_fits(
            self._h, int(idx), raw.ctypes.data_as(C.c_void_p), int(bitpix), float(bscale), float(bzero),
            float(multiplier), float(offset), capi.fptr(stats)))
        return stats

    def upload_frame_projected(self, idx, src, src_w, src_h, trans, out_of_bounds=float("nan"),
                               multiplier=1.0, offset=0.0):
        src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_upload_frame_projected(
            self._h, int(idx), capi.fptr(src), int(src_w), int(src_h), capi.fptr(t), float(out_of_bounds),
            float(multiplier), float(offset)))

    def upload_frame_fits_async(self, idx, raw, bitpix, bscale=1.0, bzero=0.0, multiplier=1.0, offset=0.0):
        """Overlapped form of upload_frame_fits (pinned ring, copy stream, no statistics)."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        capi.check(self._lib.nl_stack_upload_frame_fits_async(
            self._h, int(idx), raw.ctypes.data_as(C.c_void_p), int(bitpix), float(bscale), float(bzero),
            float(multiplier), float(offset)))

    def upload_frame_projected_async(self, idx, src, src_w, src_h, trans, out_of_bounds=float("nan"),
                                     multiplier=1.0, offset=0.0):
        src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_upload_frame_projected_async(
            self._h, int(idx), capi.fptr(src), int(src_w), int(src_h), capi.fptr(t), float(out_of_bounds),
            float(multiplier), float(offset)))

    def frame_affine(self, idx, multiplier, offset):
        capi.check(self._lib.nl_stack_frame_affine(self._h, int(idx), float(multiplier), float(offset)))

    def frame_calibrate(self, idx, calib):
        """OpCalibrate.Apply on resident slot idx (any row tile; calib on the handle's device)."""
        capi.check(self._lib.nl_stack_frame_calibrate(self._h, int(idx), calib._c))

    def frame_badpixel(self, idx, sigma_low=3.0, sigma_high=5.0):
        """OpBadPixel.Apply (mono) on resident slot idx of a whole-image handle.
        Returns (removed, (diff_mean, diff_std))."""
        removed, stats = C.c_int64(0), (C.c_float * 2)()
        capi.check(self._lib.nl_stack_frame_badpixel(self._h, int(idx), float(sigma_low), float(sigma_high),
                                                     C.byref(removed), stats))
        return int(removed.value), (np.float32(stats[0]), np.float32(stats[1]))

    def upload_frame_cfa(self, idx, raw, raw_width, raw_height, channel, cfa="RGGB", calib=None, sigma_low=3.0,
                         sigma_high=5.0):
        """OpCalibrate, OpBadPixel (Bayer branch) and OpDebayer of a raw raw_width x raw_height mosaic into
        resident slot idx of a whole-image handle of the debayered shape (debayer_shape).
        Returns (removed, (delta_mean, delta_std))."""
        raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(-1)
        assert raw.size == int(raw_width) * int(raw_height)
        removed, stats = C.c_int64(0), (C.c_float * 2)()
        capi.check(self._lib.nl_stack_upload_frame_cfa(self._h, int(idx), capi.fptr(raw), int(raw_width),
                                                       int(raw_height), None if calib is None else calib._c,
                                                       _cstr(channel), _cstr(cfa), float(sigma_low),
                                                       float(sigma_high), C.byref(removed), stats))
        return int(removed.value), (np.float32(stats[0]), np.float32(stats[1]))

    def frame_find_stars(self, idx, location, scale, star_sig=15.0, bp_sigma=5.0, star_in_out=1.4, radius=16,
                         diff_std=None):
        """star.FindStars on resident slot idx of a whole-image handle (see find_stars)."""
        return _find_stars(lambda *a: self._lib.nl_stack_frame_find_stars(self._h, int(idx), *a), location, scale,
                           star_sig, bp_sigma, star_in_out, radius, diff_std)

    def result_find_stars(self, location, scale, star_sig=15.0, bp_sigma=5.0, star_in_out=1.4, radius=16,
                          diff_std=None):
        """star.FindStars on the last pass's result, still on the device (see find_stars)."""
        return _find_stars(lambda *a: self._lib.nl_stack_result_find_stars(self._h, *a), location, scale, star_sig,
                           bp_sigma, star_in_out, radius, diff_std)

    def frame_back_extract(self, idx, stars, grid_size, hfr_factor=4.0, sigma=1.5, clip=0, render=False):
        """OpBackExtract on resident slot idx of a whole-image handle, in place (see back_extract).
        Returns (None, background or None, cells, info)."""
        _, bg, cells, info = _back_extract(lambda *a: self._lib.nl_stack_frame_back_extract(self._h, int(idx), *a),
                                           self.width, self.height, stars, grid_size, hfr_factor, sigma, clip,
                                           render)
        return None, bg, cells, info

    def frame_deband_horiz(self, idx, percentile=50.0, window=128, sigma=3.0, location=0.0, scale=0.0):
        """OpDebandHoriz on resident slot idx of a whole-image handle, in place (see deband_horiz).  Returns info."""
        return _deband(lambda *a: self._lib.nl_stack_frame_deband_horiz(self._h, int(idx), *a), percentile, window,
                       sigma, location, scale)

    def frame_deband_vert(self, idx, percentile=50.0, window=128, sigma=3.0, location=0.0, scale=0.0):
        """OpDebandVert on resident slot idx of a whole-image handle, in place (see deband_vert).  Returns info."""
        return _deband(lambda *a: self._lib.nl_stack_frame_deband_vert(self._h, int(idx), *a), percentile, window,
                       sigma, location, scale)

    def frame_gaussian_blur(self, idx, sigma):
        """OpGaussianBlur on resident slot idx of a whole-image handle, in place (see gaussian_blur)."""
        capi.check(self._lib.nl_stack_frame_gaussian_blur(self._h, int(idx), float(sigma)))

    def frame_unsharp_mask(self, idx, sigma, gain, min, max, abs_threshold):
        """OpUnsharpMask on resident slot idx of a whole-image handle, in place (see unsharp_mask)."""
        capi.check(self._lib.nl_stack_frame_unsharp_mask(self._h, int(idx), float(sigma), float(gain), float(min),
                                                         float(max), float(abs_threshold)))

    def result_gaussian_blur(self, sigma):
        """OpGaussianBlur on the last pass's result, still on the device, in place (download_rows(-1, ...) reads it)."""
        capi.check(self._lib.nl_stack_result_gaussian_blur(self._h, float(sigma)))

    def result_unsharp_mask(self, sigma, gain, min, max, abs_threshold):
        """OpUnsharpMask on the last pass's result, still on the device, in place."""
        capi.check(self._lib.nl_stack_result_unsharp_mask(self._h, float(sigma), float(gain), float(min), float(max),
                                                          float(abs_threshold)))

    def frame_tone(self, idx, kind, *p, stats=False):
        """One tone curve of the stretch command (capi.TONE_*, see tone) on resident slot idx, in place; any row tile.
        stats=True: returns (min, mean, max) of the transformed slot from the same pass, the bits frame_stats would
        return afterwards."""
        return _tone(lambda *a: self._lib.nl_stack_frame_tone(self._h, int(idx), *a), kind, p, stats)

    def result_tone(self, kind, *p, stats=False):
        """One tone curve on the last pass's result, still on the device, in place (download_rows(-1, ...) reads it)."""
        return _tone(lambda *a: self._lib.nl_stack_result_tone(self._h, *a), kind, p, stats)

    def frame_export_gray(self, idx, min, max, gamma=1.0, bits=16):
        """OpSave's quantisation of resident slot idx (see export_gray); the slot stays as it is."""
        return _export_gray(lambda *a: self._lib.nl_stack_frame_export_gray(self._h, int(idx), *a), self.tile_pixels,
                            min, max, gamma, bits)

    def result_export_gray(self, min, max, gamma=1.0, bits=16):
        """OpSave's quantisation of the last pass's result, still on the device."""
        return _export_gray(lambda *a: self._lib.nl_stack_result_export_gray(self._h, *a), self.tile_pixels, min, max,
                            gamma, bits)

    # -- the rgb / lrgb command: three slots `planes` of this handle are the channels ------------------------------
    def frame_combine_from(self, idx, src, src_idx, min, mult):
        """The pixel loop of NewRGBFromChannels: slot idx = (slot src_idx of `src` - min) * mult; src_idx -1 reads the
        last pass's result of `src`; src may be this handle and the same slot (in place)."""
        capi.check(self._lib.nl_stack_frame_combine_from(self._h, int(idx), src._h, int(src_idx), float(min),
                                                         float(mult)))

    def rgb_scale_offset_clamp(self, planes, alpha, beta, stats=False):
        """ScaleOffsetClampRGB on the three planes, in place.  stats=True: returns a (3, 3) array, {min, mean, max} per
        plane from the same pass, the bits frame_stats would return afterwards."""
        a, b = _f32x3(alpha), _f32x3(beta)
        out = np.zeros(9, np.float32) if stats else None
        capi.check(self._lib.nl_stack_rgb_scale_offset_clamp(self._h, _planes(planes), capi.fptr(a), capi.fptr(b),
                                                             None if out is None else capi.fptr(out)))
        return None if out is None else out.reshape(3, 3)

    def rgb_darkest_block(self, planes, block, border):
        """findDarkestBlock: the (r, g, b) means of the darkest block x block square inside the border."""
        out = capi.Rgb()
        capi.check(self._lib.nl_stack_rgb_darkest_block(self._h, _planes(planes), int(block), float(border),
                                                        C.byref(out)))
        return _rgb_out(out)

    def rgb_mean_star_intensity(self, planes, stars, skip_bright, skip_dim, clip):
        """meanStarIntensity over the star list (capi.STAR_DTYPE) with the channel clip levels `clip`."""
        stars = np.ascontiguousarray(np.zeros(0, capi.STAR_DTYPE) if stars is None else stars, dtype=capi.STAR_DTYPE)
        out = capi.Rgb()
        capi.check(self._lib.nl_stack_rgb_mean_star_intensity(
            self._h, _planes(planes), stars.ctypes.data_as(C.c_void_p), int(stars.size), float(skip_bright),
            float(skip_dim), _rgb_in(clip), C.byref(out)))
        return _rgb_out(out)

    def rgb_balance(self, planes, stars, block, border, skip_bright, skip_dim, shadows, highlights, loc, scale):
        """SetBlackWhitePoints on the three planes, in place (see rgb_balance).  Returns the report dict."""
        return _rgb_balance(lambda *a: self._lib.nl_stack_rgb_balance(self._h, _planes(planes), *a), stars, block,
                            border, skip_bright, skip_dim, shadows, highlights, loc, scale)

    def rgb_chroma(self, planes, kind, *p):
        """One chroma or hue step (capi.CHROMA_GAMMA (gamma, threshold), CHROMA_NEUTRALIZE (low, high), CHROMA_FOR_HUES
        (from, to, factor), ROTATE_HUES (from, to, offset, lthres)) on planes {h, c, l}, in place."""
        assert len(p) <= 4
        op = capi.Chroma(int(kind), (C.c_float * 4)(*[float(v) for v in p]))
        capi.check(self._lib.nl_stack_rgb_chroma(self._h, _planes(planes), C.byref(op)))

    def rgb_export(self, planes, min, max, gamma=1.0, bits=16):
        """WriteTIFF16 / WriteJPG's pixel loop on the three planes (see export_rgb); the planes stay as they are."""
        return _export_rgb(lambda *a: self._lib.nl_stack_rgb_export(self._h, _planes(planes), *a), self.tile_pixels,
                           min, max, gamma, bits)

    def frame_bin_from(self, idx, src, src_idx, n):
        """NewImageBinNxN of resident slot src_idx of the whole-image handle `src` into slot idx of this one, whose
        shape is bin_shape of the source's (n <= 1: a device copy)."""
        capi.check(self._lib.nl_stack_frame_bin_from(self._h, int(idx), src._h, int(src_idx), int(n)))

    def frame_project_from(self, idx, src, src_idx, trans, out_of_bounds=float("nan")):
        """OpAlign's Project of resident slot src_idx of the whole-image handle `src` through the forward transform
        `trans` into slot idx of this handle (any row tile).  Bit-identical to upload_frame_projected of the same
        source; the source slot stays as it is."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_project_from(self._h, int(idx), src._h, int(src_idx), capi.fptr(t),
                                                         float(out_of_bounds)))

    def project_tile_paths(self, src, src_idx, trans):
        """(staged, direct): how many workgroup tiles of frame_project_from(., src, src_idx, trans) stage their source
        box in LDS, and how many take their taps from global memory (developer query)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        staged, direct = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_project_tile_paths(self._h, src._h, int(src_idx), capi.fptr(t),
                                                         C.byref(staged), C.byref(direct)))
        return int(staged.value), int(direct.value)

    def frame_resample_from(self, idx, src, src_idx, trans, out_of_bounds=float("nan"), kernel=capi.RS_LANCZOS3,
                            clamp=False):
        """frame_project_from with the resampling kernel `kernel` (capi.RS_BILINEAR, RS_BICUBIC, RS_LANCZOS3) and, with
        clamp, the result held to the range of its four central taps (include/nlstack_resample.h; an EXTENSION, the
        reference resamples bilinearly).  Where a pixel's wide footprint does not fit the source it gets the bilinear
        value, so the valid area does not depend on the kernel."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_resample_from(self._h, int(idx), src._h, int(src_idx), capi.fptr(t),
                                                          float(out_of_bounds), int(kernel), int(bool(clamp))))

    def resample_tile_paths(self, src, src_idx, trans, kernel=capi.RS_LANCZOS3):
        """project_tile_paths for frame_resample_from(., src, src_idx, trans, ., kernel) (developer query)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        staged, direct = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_resample_tile_paths(self._h, src._h, int(src_idx), capi.fptr(t), int(kernel),
                                                          C.byref(staged), C.byref(direct)))
        return int(staged.value), int(direct.value)

    def frame_drizzle_from(self, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac=1.0, weight=1.0, first=False,
                           kernel=capi.DZ_TURBO):
        """Drizzle: lays the unresampled resident slot src_idx of the whole-image handle `src` through the forward
        transform `trans` (source -> reference pixel) onto this handle's planes sum_idx (flux) and wgt_idx (weight),
        whose grid has `scale` pixels per reference pixel; every source pixel is a drop of `pixfrac` times its side
        (include/nlstack_drizzle.h; an EXTENSION, the reference has no drizzle).  first starts the planes, otherwise
        the frame is added to them.  kernel: capi.DZ_TURBO (axis-aligned drop) or DZ_POINT."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_drizzle_from(self._h, int(sum_idx), int(wgt_idx), src._h, int(src_idx),
                                                         capi.fptr(t), float(scale), float(pixfrac), float(weight),
                                                         int(bool(first)), int(kernel)))

    def drizzle_finalize(self, sum_idx, wgt_idx, out_idx, min_weight=0.0, empty=float("nan")):
        """Slot out_idx = sum / weight where the weight exceeds min_weight, else `empty`; the slots may alias."""
        capi.check(self._lib.nl_stack_drizzle_finalize(self._h, int(sum_idx), int(wgt_idx), int(out_idx),
                                                       float(min_weight), float(empty)))

    def frame_reject_against(self, idx, model_idx, low, high):
        """(n_low, n_high): the pixels of slot idx more than `low` below or `high` above the model in slot model_idx
        become NaN (absolute thresholds >= 0), which a drizzle skips; everything else keeps its bits."""
        n_low, n_high = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_frame_reject_against(self._h, int(idx), int(model_idx), float(low), float(high),
                                                           C.byref(n_low), C.byref(n_high)))
        return int(n_low.value), int(n_high.value)

    def drizzle_tile_paths(self, src, src_idx, trans, scale, pixfrac=1.0):
        """project_tile_paths for frame_drizzle_from(., ., src, src_idx, trans, scale, pixfrac) (developer query)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        staged, direct = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_drizzle_tile_paths(self._h, src._h, int(src_idx), capi.fptr(t), float(scale),
                                                         float(pixfrac), C.byref(staged), C.byref(direct)))
        return int(staged.value), int(direct.value)

    def frame_drizzle_cfa_from(self, sum_idx, wgt_idx, src, src_idx, trans, scale, channel, cfa="RGGB", pixfrac=1.0,
                               weight=1.0, first=False, kernel=capi.DZ_TURBO):
        """CFA drizzle: frame_drizzle_from for the pixels of `channel` ("R", "G", "B") of the raw `cfa` mosaic in slot
        src_idx of the whole-image handle `src`, no debayer in front; `trans` maps mosaic pixels to reference pixels
        (drizzle_cfa_transform).  The planes equal those of frame_drizzle_from on a copy of the mosaic whose other
        pixels are NaN (include/nlstack_cfadrizzle.h; an EXTENSION)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_drizzle_cfa_from(self._h, int(sum_idx), int(wgt_idx), src._h, int(src_idx),
                                                             capi.fptr(t), float(scale), float(pixfrac), float(weight),
                                                             int(bool(first)), int(kernel), _cstr(channel), _cstr(cfa)))

    def frame_drizzle_square_from(self, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac=1.0, weight=1.0,
                                  first=False):
        """frame_drizzle_from with the square kernel: a drop is the image of the shrunken pixel under the transform (a
        rotated square) and lays its flux down by the exact area of its overlap with each output pixel, under any
        rotation (include/nlstack_sqdrizzle.h; an EXTENSION)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_drizzle_square_from(self._h, int(sum_idx), int(wgt_idx), src._h, int(src_idx),
                                                                capi.fptr(t), float(scale), float(pixfrac), float(weight),
                                                                int(bool(first))))

    def frame_drizzle_square_cfa_from(self, sum_idx, wgt_idx, src, src_idx, trans, scale, channel, cfa="RGGB", pixfrac=1.0,
                                      weight=1.0, first=False):
        """frame_drizzle_cfa_from with the square kernel: the planes equal those of frame_drizzle_square_from on a copy
        of the mosaic whose other pixels are NaN (include/nlstack_sqdrizzle.h; an EXTENSION)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_stack_frame_drizzle_square_cfa_from(self._h, int(sum_idx), int(wgt_idx), src._h,
                                                                    int(src_idx), capi.fptr(t), float(scale),
                                                                    float(pixfrac), float(weight), int(bool(first)),
                                                                    _cstr(channel), _cstr(cfa)))

    def drizzle_square_tile_paths(self, src, src_idx, trans, scale, pixfrac=1.0):
        """drizzle_tile_paths for the two square entries: the window of the square radius (developer query)."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        staged, direct = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_drizzle_square_tile_paths(self._h, src._h, int(src_idx), capi.fptr(t), float(scale),
                                                                float(pixfrac), C.byref(staged), C.byref(direct)))
        return int(staged.value), int(direct.value)

    def frame_reject_against_cfa(self, idx, model_idx, channel, cfa, low, high):
        """(n_low, n_high): frame_reject_against on the pixels of `channel` of the `cfa` mosaic in slot idx; every
        other pixel keeps its bits and counts nowhere."""
        n_low, n_high = C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.nl_stack_frame_reject_against_cfa(self._h, int(idx), int(model_idx), _cstr(channel),
                                                               _cstr(cfa), float(low), float(high), C.byref(n_low),
                                                               C.byref(n_high)))
        return int(n_low.value), int(n_high.value)

    def frame_badpixel_cfa(self, idx, channel, cfa="RGGB", sigma_low=3.0, sigma_high=5.0):
        """CosmeticCorrectionBayer for one channel in place on the resident mosaic in slot idx of a whole-image
        handle: upload_frame_cfa's bad-pixel step without the debayer.  Returns (removed, (delta_mean, delta_std))."""
        removed, stats = C.c_int64(0), (C.c_float * 2)()
        capi.check(self._lib.nl_stack_frame_badpixel_cfa(self._h, int(idx), _cstr(channel), _cstr(cfa),
                                                         float(sigma_low), float(sigma_high), C.byref(removed), stats))
        return int(removed.value), (np.float32(stats[0]), np.float32(stats[1]))

    def download_result_fits(self):
        raw = np.empty(self.tile_pixels * 4, np.uint8)
        capi.check(self._lib.nl_stack_download_result_fits(self._h, raw.ctypes.data_as(C.c_void_p)))
        return raw


class StackGroup:
    """nl_group_*: one stack over several GPUs from one process -- tile t owns the rows
    group_tile_rows(height, n_tiles, t) of all frames on devices[t]; counters summed on the
    host (stack.go:142-152, 193-198).  devices=None: one tile per visible device."""

    def __init__(self, n_frames, width, height, n_tiles=0, devices=None):
        self._lib = capi.load()
        self.n_frames, self.width, self.height = int(n_frames), int(width), int(height)
        dev = None
        if devices is not None:
            n_tiles = len(devices)
            dev = (C.c_int * n_tiles)(*[int(d) for d in devices])
        self._g = self._lib.nl_group_create(self.n_frames, self.width, self.height, int(n_tiles), dev)
        if not self._g:
            raise capi.NlError(capi.ERR_HIP, capi.last_error())
        self.size = self._lib.nl_group_size(self._g)

    def close(self):
        if self._g:
            self._lib.nl_group_destroy(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def tile_rows(self, t):
        r0, nr = C.c_int(), C.c_int()
        self._lib.nl_group_tile_rows(self.height, self.size, int(t), C.byref(r0), C.byref(nr))
        return r0.value, nr.value

    def tile(self, t):
        """Borrowed view of tile t's handle (nl_group_tile): the group keeps ownership."""
        r0, nr = self.tile_rows(t)
        h = self._lib.nl_group_tile(self._g, int(t))
        if not h:
            raise IndexError(t)
        return StackHandle._borrow(h, self.n_frames, self.width, self.height, r0, nr)

    def upload_frames(self, frames):
        for i, f in enumerate(frames):
            f = np.ascontiguousarray(f, dtype=np.float32).reshape(-1)
            assert f.size == self.width * self.height
            capi.check(self._lib.nl_group_upload_frame(self._g, i, capi.fptr(f)))

    def upload_frame_fits(self, idx, raw, bitpix, bscale=1.0, bzero=0.0, multiplier=1.0, offset=0.0):
        """raw: big-endian FITS payload of the WHOLE frame; every tile decodes its rows on its device."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        capi.check(self._lib.nl_group_upload_frame_fits(
            self._g, int(idx), raw.ctypes.data_as(C.c_void_p), int(bitpix), float(bscale), float(bzero),
            float(multiplier), float(offset)))

    def upload_frame_projected(self, idx, src, src_w, src_h, trans, out_of_bounds=float("nan"),
                               multiplier=1.0, offset=0.0):
        src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_group_upload_frame_projected(
            self._g, int(idx), capi.fptr(src), int(src_w), int(src_h), capi.fptr(t), float(out_of_bounds),
            float(multiplier), float(offset)))

    def frame_project_from(self, idx, src, src_idx, trans, out_of_bounds=float("nan")):
        """StackHandle.frame_project_from on the group: every tile projects its own rows from the resident slot."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_group_frame_project_from(self._g, int(idx), src._h, int(src_idx), capi.fptr(t),
                                                         float(out_of_bounds)))

    def frame_resample_from(self, idx, src, src_idx, trans, out_of_bounds=float("nan"), kernel=capi.RS_LANCZOS3,
                            clamp=False):
        """StackHandle.frame_resample_from on the group: every tile resamples its own rows from the resident slot."""
        t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
        capi.check(self._lib.nl_group_frame_resample_from(self._g, int(idx), src._h, int(src_idx), capi.fptr(t),
                                                          float(out_of_bounds), int(kernel), int(bool(clamp))))

    def fill_synthetic(self, seed=0x4E4C5354):
        capi.check(self._lib.nl_group_fill_synthetic(self._g, C.c_uint64(seed)))

    def set_active_frames(self, n):
        """StackHandle.set_active_frames on every tile."""
        capi.check(self._lib.nl_group_set_active_frames(self._g, int(n)))
        self.n_frames = int(n)

    def set_weights(self, weights):
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        capi.check(self._lib.nl_group_set_weights(self._g, capi.fptr(w) if w is not None else None))

    def set_exact(self, on=True):
        capi.check(self._lib.nl_group_set_exact(self._g, int(on)))

    def run(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """download=False: the result stays on the devices (e.g. for accumulate); returns (None, low, high)."""
        return _run_counted(self._lib.nl_group_run, self._g, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(download))

    def _result_array(self, download):
        return np.zeros(self.width * self.height, np.float32) if download else None

    def run_maps(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, fast=False):
        """StackHandle.run_maps over the tiles: (result, clip_low, clip_high, reject_low, reject_high), every tile
        writing its own rows.  fast=True: nl_group_run_maps_fast."""
        return self._run_maps(self._lib.nl_group_run_maps_fast if fast else self._lib.nl_group_run_maps, mode, sigma_low, sigma_high, ref_loc)

    def _run_maps(self, entry, mode, sigma_low, sigma_high, ref_loc):
        return _run_maps(entry, self._g, self.width * self.height, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc))

    def run_maps_resident(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """StackHandle.run_maps_resident over the tiles (nl_group_run_maps_resident): the return value of run_maps."""
        return self._run_maps(self._lib.nl_group_run_maps_resident, mode, sigma_low, sigma_high, ref_loc)

    def run_maps_deep(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """StackHandle.run_maps_deep over the tiles (nl_group_run_maps_deep): the return value of run_maps."""
        return self._run_maps(self._lib.nl_group_run_maps_deep, mode, sigma_low, sigma_high, ref_loc)

    def run_maps_full(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """StackHandle.run_maps_full over the tiles (nl_group_run_maps_full): the return value of run_maps."""
        return self._run_maps(self._lib.nl_group_run_maps_full, mode, sigma_low, sigma_high, ref_loc)

    def run_maps_deepstack(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0):
        """StackHandle.run_maps_deepstack over the tiles (nl_group_run_maps_deepstack): the return value of run_maps."""
        return self._run_maps(self._lib.nl_group_run_maps_deepstack, mode, sigma_low, sigma_high, ref_loc)

    def run_linfit_weighted(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """StackHandle.run_linfit_weighted over the tiles: (result or None, clip_low, clip_high)."""
        return _run_counted(self._lib.nl_group_run_linfit_weighted, self._g, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(download))

    def run_clip_weighted(self, mode=capi.ST_AUTO, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """StackHandle.run_clip_weighted over the tiles: (result or None, clip_low, clip_high)."""
        return _run_counted(self._lib.nl_group_run_clip_weighted, self._g,
                            (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc), self._result_array(download))

    def run_mad_weighted(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """StackHandle.run_mad_weighted over the tiles: (result or None, clip_low, clip_high)."""
        return _run_counted(self._lib.nl_group_run_mad_weighted, self._g, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(download))

    def run_mad_weighted_deepstack(self, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """StackHandle.run_mad_weighted_deepstack over the tiles: (result or None, clip_low, clip_high)."""
        return _run_counted(self._lib.nl_group_run_mad_weighted_deepstack, self._g, _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(download))

    def run_deepstack(self, mode, sigma_low=2.75, sigma_high=2.75, ref_loc=0.0, download=True):
        """StackHandle.run_deepstack over the tiles: (result or None, clip_low, clip_high)."""
        return _run_counted(self._lib.nl_group_run_deepstack, self._g, (int(mode),) + _sigmas(sigma_low, sigma_high, ref_loc),
                            self._result_array(download))

    def coverage(self):
        """StackHandle.coverage over the tiles."""
        out = np.zeros(self.width * self.height, np.uint16)
        capi.check(self._lib.nl_group_coverage(self._g, _u16ptr(out)))
        return out

    def upload_frame(self, idx, frame):
        """Overlapped upload of one whole frame (nl_group_upload_frame)."""
        f = np.ascontiguousarray(frame, dtype=np.float32).reshape(-1)
        assert f.size == self.width * self.height
        capi.check(self._lib.nl_group_upload_frame(self._g, int(idx), capi.fptr(f)))

    def find_sigmas(self, mode, clip_perc_low, clip_perc_high, ref_loc=0.0):
        out = np.zeros(self.width * self.height, np.float32)
        cl, ch = C.c_int64(0), C.c_int64(0)
        sl, sh, passes = C.c_float(), C.c_float(), C.c_int()
        capi.check(self._lib.nl_group_find_sigmas(
            self._g, int(mode), C.c_float(ref_loc), C.c_float(clip_perc_low), C.c_float(clip_perc_high),
            capi.fptr(out), C.byref(cl), C.byref(ch), C.byref(sl), C.byref(sh), C.byref(passes)))
        return out, cl.value, ch.value, float(sl.value), float(sh.value), passes.value

    def accumulate(self, weight, first):
        capi.check(self._lib.nl_group_accumulate(self._g, C.c_float(weight), int(bool(first))))

    def accumulate_finalize(self, weight_sum):
        out = np.zeros(self.width * self.height, np.float32)
        capi.check(self._lib.nl_group_accumulate_finalize(self._g, C.c_float(weight_sum), capi.fptr(out)))
        return out


def fits_parse_header(file_bytes, frame_id=0):
    """Header of a FITS file image (read.go:445-469, 97-147): dict with bitpix, naxisn, bzero, bscale, exposure,
    pixels, header_bytes (= offset of the payload), payload_bytes, padded_payload_bytes."""
    lib = capi.load()
    buf = np.frombuffer(file_bytes, dtype=np.uint8)
    h = capi.FitsHeader()
    capi.check(lib.nl_fits_parse_header(buf.ctypes.data_as(C.c_void_p), buf.size, int(frame_id), C.byref(h)))
    return {"bitpix": h.bitpix, "naxisn": [h.naxisn[i] for i in range(h.naxis)], "bzero": np.float32(h.bzero),
            "bscale": np.float32(h.bscale), "exposure": np.float32(h.exposure), "pixels": h.pixels,
            "header_bytes": h.header_bytes, "payload_bytes": h.payload_bytes,
            "padded_payload_bytes": h.padded_payload_bytes}


def fits_write_header(naxisn, bzero=0.0, bscale=1.0, exposure=0.0):
    """The header Image.Write emits for a BITPIX -32 image (write.go:54-89), padded to 2880-byte blocks."""
    lib = capi.load()
    ax = (C.c_int32 * len(naxisn))(*[int(n) for n in naxisn])
    n = lib.nl_fits_write_header(None, 0, len(naxisn), ax, float(bzero), float(bscale), float(exposure))
    if n < 0:
        raise capi.NlError(capi.ERR_INVALID_ARG, capi.last_error())
    out = np.empty(n, np.uint8)
    got = lib.nl_fits_write_header(out.ctypes.data_as(C.c_void_p), n, len(naxisn), ax, float(bzero), float(bscale),
                                   float(exposure))
    assert got == n
    return out.tobytes()


def fits_padded_bytes(payload_bytes):
    return int(capi.load().nl_fits_padded_bytes(int(payload_bytes)))


def fits_decode(raw, bitpix, bscale=1.0, bzero=0.0, device=0):
    lib = capi.load()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    bpv = {8: 1, 16: 2, 32: 4, 64: 8, -32: 4, -64: 8}.get(int(bitpix), 1)
    n = raw.size // bpv
    out = np.empty(n, np.float32)
    stats = np.zeros(3, np.float32)
    capi.check(lib.nl_fits_decode(raw.ctypes.data_as(C.c_void_p), int(bitpix), n, float(bscale),
                                  float(bzero), capi.fptr(out), capi.fptr(stats), int(device)))
    return out, stats


def project_bilinear(src, src_w, src_h, dst_w, dst_h, trans, out_of_bounds=float("nan"), device=0):
    lib = capi.load()
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
    dst = np.empty(int(dst_w) * int(dst_h), np.float32)
    capi.check(lib.nl_project_bilinear(capi.fptr(src), int(src_w), int(src_h), capi.fptr(dst), int(dst_w),
                                       int(dst_h), capi.fptr(t), float(out_of_bounds), int(device)))
    return dst


def weights_from_scalars(weighting, per_frame):
    """getWeights (stack.go:231-270) on per-frame exposure / noise / HFR."""
    lib = capi.load()
    pf = np.ascontiguousarray(per_frame, dtype=np.float32)
    w = np.zeros(pf.size, np.float32)
    bad = C.c_int(-1)
    rc = lib.nl_weights_from_scalars(int(weighting), capi.fptr(pf), pf.size, capi.fptr(w),
                                     C.byref(bad))
    if rc != capi.OK:
        raise capi.NlError(rc, capi.last_error())
    return None if weighting == capi.WEIGHT_NONE else w


class Calibration:
    """OpCalibrate's dark and / or flat master resident on one device (nl_calib_t).  The flat's
    shape defaults to (width, height); flat_width / flat_height give it another one (the reference
    then fails with "dark dimensions ... differ from flat dimensions ...")."""

    def __init__(self, device, width, height, dark=None, flat=None, flat_width=None, flat_height=None):
        self._lib = capi.load()
        self._c = None
        fw = int(width if flat_width is None else flat_width)
        fh = int(height if flat_height is None else flat_height)
        d = None if dark is None else np.ascontiguousarray(dark, dtype=np.float32).reshape(-1)
        f = None if flat is None else np.ascontiguousarray(flat, dtype=np.float32).reshape(-1)
        assert d is None or d.size == int(width) * int(height)
        assert f is None or f.size == fw * fh
        c = self._lib.nl_calib_create(int(device), None if d is None else capi.fptr(d), int(width), int(height),
                                      None if f is None else capi.fptr(f), fw, fh)
        if not c:
            msg = capi.last_error()
            raise capi.NlError(capi.ERR_NO_DEVICE if "no HIP device" in msg else capi.ERR_INVALID_ARG, msg)
        self._c = c
        self.device, self.width, self.height = int(device), int(width), int(height)

    @property
    def flat_max(self):
        """FlatFrame.Stats.Max() as taken when the masters were set."""
        out = C.c_float()
        capi.check(self._lib.nl_calib_flat_max(self._c, C.byref(out)))
        return np.float32(out.value)

    def close(self):
        if self._c:
            self._lib.nl_calib_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _device(device):
    """The device of a host form: `device`, default 0."""
    return 0 if device is None else int(device)


def _host_frame(frame, width=None, height=None, copy=True, planes=1):
    """A host frame (or `planes` of them) as flat contiguous float32: a copy of the caller's that the library may write
    in place, or with copy=False the caller's own where it already is one.  Without width and height any size that
    holds `planes` whole planes."""
    out = np.array(frame, dtype=np.float32, copy=True) if copy else np.ascontiguousarray(frame, dtype=np.float32)
    out = out.reshape(-1)
    if width is None:
        assert out.size % int(planes) == 0
    else:
        assert out.size == int(planes) * int(width) * int(height)
    return out


def preprocess_frame(frame, width, height, calib=None, sigma_low=3.0, sigma_high=5.0, frame_id=0, device=None):
    """OpCalibrate then OpBadPixel (mono) on one host frame, on calib's device (else `device`, default 0).
    Returns (out, removed, (diff_mean, diff_std))."""
    frame = _host_frame(frame, width, height, copy=False)
    if device is None:
        device = calib.device if calib is not None else 0
    out = np.empty_like(frame)
    removed, stats = C.c_int64(0), (C.c_float * 2)()
    lib = capi.load()
    capi.check(lib.nl_preprocess_frame(None if calib is None else calib._c, int(frame_id), capi.fptr(frame),
                                       capi.fptr(out), int(width), int(height), float(sigma_low), float(sigma_high),
                                       C.byref(removed), stats, int(device)))
    return out, int(removed.value), (np.float32(stats[0]), np.float32(stats[1]))


def _find_stars(call, location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std, capacity=16384):
    """One nl_*find_stars call through `call(<parameters from location on>)`; retried once with the reported count
    when `capacity` was short."""
    args = (float(location), float(scale), float(star_sig), float(bp_sigma), float(star_in_out), int(radius),
            float("nan") if diff_std is None else float(diff_std))
    n, shifts, hfr = C.c_int(0), C.c_float(0.0), C.c_float(0.0)
    for _ in range(2):
        out = np.zeros(max(capacity, 1), capi.STAR_DTYPE)
        capi.check(call(*args, out.ctypes.data_as(C.c_void_p), int(capacity), C.byref(n), C.byref(shifts),
                        C.byref(hfr)))
        if n.value <= capacity:
            break
        capacity = n.value
    return out[:n.value].copy(), np.float32(shifts.value), np.float32(hfr.value)


def find_stars(frame, width, height, location, scale, star_sig=15.0, bp_sigma=5.0, star_in_out=1.4, radius=16,
               diff_std=None, device=None):
    """star.FindStars (internal/star/findstars.go:59-103) on one host frame on `device` (default 0).
    location / scale: the frame's Stats.Location() / Scale(); diff_std: MedianDiffStats.StdDev() or None (nil).
    Returns (stars, sum_of_shifts, avg_hfr): stars a structured array with the fields index value x y mass hfr."""
    frame = _host_frame(frame, width, height, copy=False)
    lib = capi.load()
    return _find_stars(lambda *a: lib.nl_find_stars(capi.fptr(frame), int(width), int(height), *a,
                                                    _device(device)),
                       location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std)


def _back_extract(call, width, height, stars, grid_size, hfr_factor, sigma, clip, render):
    """One nl_*back_extract call through `call(<parameters from grid_size on>)`."""
    stars = np.ascontiguousarray(np.zeros(0, capi.STAR_DTYPE) if stars is None else stars, dtype=capi.STAR_DTYPE)
    g = int(grid_size)
    n_cells = ((int(width) + g // 2) // g) * ((int(height) + g // 2) // g) if g > 0 else 0
    cells = np.zeros(max(n_cells, 1), np.float32)
    bg = np.empty(int(width) * int(height), np.float32) if render else None
    info = capi.Background()
    capi.check(call(g, float(hfr_factor), float(sigma), int(clip), stars.ctypes.data_as(C.c_void_p), int(stars.size),
                    None if bg is None else capi.fptr(bg), capi.fptr(cells), int(n_cells), C.byref(info)))
    info = {name: getattr(info, name) for name, _ in capi.Background._fields_}
    for k in ("spacing_x", "spacing_y", "min", "max"):
        info[k] = np.float32(info[k])
    return None, bg, cells[:n_cells].copy(), info


def back_extract(frame, width, height, stars, grid_size, hfr_factor=4.0, sigma=1.5, clip=0, render=False,
                 device=None):
    """OpBackExtract (internal/ops/pre/preprocess.go:372-398): pre.NewBackground over the frame with the star list
    find_stars returned, then Subtract (render=False) or Render + subtract (render=True), on `device` (default 0).
    Returns (out, background or None, cells, info): out the subtracted frame (None when grid_size <= 0, the
    reference's no-op), cells the smoothed grid, info the dict of nl_background_t."""
    out = _host_frame(frame, width, height)
    lib = capi.load()
    _, bg, cells, info = _back_extract(
        lambda *a: lib.nl_back_extract(capi.fptr(out), int(width), int(height), *a, _device(device)),
        width, height, stars, grid_size, hfr_factor, sigma, clip, render)
    return (out if int(grid_size) > 0 else None), bg, cells, info


def locscale_seeds(key, n=capi.LOCSCALE_MAX_SEEDS):
    """n nonzero xorshift32 seeds from one 64-bit key (splitmix64), for callers that want the reference's "any seed"
    behaviour.  Host only."""
    seeds = np.zeros(int(n), np.uint32)
    capi.check(capi.load().nl_locscale_seeds(int(key) & (2 ** 64 - 1), seeds.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             seeds.size))
    return seeds


def _location_scale(call, estimator, seeds, num_samples, min_max):
    """One nl_*location_scale call through `call(<parameters from estimator on>)`: (location, scale, info)."""
    seeds = np.ascontiguousarray(np.zeros(0, np.uint32) if seeds is None else seeds, dtype=np.uint32)
    mm = None if min_max is None else np.ascontiguousarray(min_max, dtype=np.float32)
    assert mm is None or mm.size == 2
    loc, scale, info = C.c_float(), C.c_float(), capi.LocScale()
    capi.check(call(int(estimator), int(num_samples), seeds.ctypes.data_as(C.POINTER(C.c_uint32)), seeds.size,
                    None if mm is None else capi.fptr(mm), C.byref(loc), C.byref(scale), C.byref(info)))
    out = {name: getattr(info, name) for name, _ in capi.LocScale._fields_}
    out["draws"] = [int(v) for v in info.draws]
    for name in ("min", "max", "epsilon"):
        out[name] = np.float32(out[name])
    return np.float32(loc.value), np.float32(scale.value), out


def location_scale(frame, width, height, estimator=capi.LSE_SC_MEDIAN_QN, seeds=None,
                   num_samples=capi.LOCSCALE_SAMPLES, min_max=None, device=None):
    """Stats.Location() / Scale() (internal/stats/stats.go:225-244) of one host frame on `device` (default 0), bit-exact
    given the seeds: estimator capi.LSE_MEAN_STDDEV, LSE_MEDIAN_MAD (2 seeds), LSE_SC_MEDIAN_QN (25 seeds, the
    reference's default) or LSE_HISTOGRAM; seeds nonzero uint32, one per sampling call (locscale_seeds); min_max the
    cached Stats.Min() / Max() where they differ from the frame's.  Returns (location, scale, info): info the dict of
    nl_locscale_t."""
    frame = _host_frame(frame, width, height, copy=False)
    lib = capi.load()
    return _location_scale(lambda *a: lib.nl_location_scale(capi.fptr(frame), int(width), int(height), *a,
                                                            _device(device)),
                           estimator, seeds, num_samples, min_max)


class Aligner:
    """star.Aligner up to the minimiser (internal/star/align.go:58-206) on `device` (default 0): NewAligner over the
    reference frame's stars (find_stars' array, brightest first) and the priming constant k.  Immutable once created;
    match and match_stars may be called from several threads at once."""

    def __init__(self, ref_width, ref_height, ref_stars, k=50, device=None):
        self._lib = capi.load()
        self.k = int(k)
        ref_stars = np.ascontiguousarray(ref_stars, dtype=capi.STAR_DTYPE)
        self.n_ref_stars = int(ref_stars.size)
        self._h = self._lib.nl_aligner_create(_device(device), int(ref_width), int(ref_height),
                                              ref_stars.ctypes.data_as(C.c_void_p), self.n_ref_stars, self.k)
        if not self._h:
            raise capi.NlError(capi.ERR_INVALID_ARG, capi.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nl_aligner_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self):
        """(picked, triangles): pickBrightestDistant's indices into the reference stars and the reference triangles
        (capi.TRIANGLE_DTYPE) in generateTriangles' order."""
        n_picked, n_tris = C.c_int(0), C.c_int(0)
        picked = np.zeros(capi.ALIGN_MAX_K, np.int32)
        p32 = C.POINTER(C.c_int32)
        capi.check(self._lib.nl_aligner_info(self._h, picked.ctypes.data_as(p32), picked.size, C.byref(n_picked),
                                             C.byref(n_tris), None, 0))
        tris = np.zeros(max(n_tris.value, 1), capi.TRIANGLE_DTYPE)
        capi.check(self._lib.nl_aligner_info(self._h, None, 0, None, None, tris.ctypes.data_as(C.c_void_p), tris.size))
        return picked[:n_picked.value].copy(), tris[:n_tris.value].copy()

    def match(self, frame_width, stars, triangles=False):
        """Align (:74-83) up to the minimiser for one frame's stars.  Returns (candidates, ref_index, info): the
        shortlist (capi.CANDIDATE_DTYPE), per candidate and star the index of its reference star or -1, and the dict
        of nl_align_info_t -- with triangles=True also the frame's triangles and every triangle's nearest reference
        triangle (tri_dist, tri_ref)."""
        stars = np.ascontiguousarray(stars, dtype=capi.STAR_DTYPE)
        cands = np.zeros(self.k, capi.CANDIDATE_DTYPE)
        ref_index = np.zeros((self.k, max(stars.size, 1)), np.int32)
        n_cands, info = C.c_int(0), capi.AlignInfo()
        if triangles:
            cap = min(self.k, max(stars.size, 1))
            cap = max(cap * (cap - 1) * (cap - 2) // 6, 1)
            tris, dist, ref = np.zeros(cap, capi.TRIANGLE_DTYPE), np.zeros(cap, np.float32), np.zeros(cap, np.int32)
            info.triangles = tris.ctypes.data_as(C.c_void_p)
            info.tri_dist, info.tri_ref = capi.fptr(dist), ref.ctypes.data_as(C.POINTER(C.c_int32))
            info.tri_capacity = cap
        capi.check(self._lib.nl_aligner_match(self._h, int(frame_width), stars.ctypes.data_as(C.c_void_p),
                                              int(stars.size), cands.ctypes.data_as(C.c_void_p), self.k,
                                              C.byref(n_cands), ref_index.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.byref(info)))
        nc, nt = n_cands.value, info.n_triangles
        out = {"n_picked": info.n_picked, "n_triangles": nt, "scale_factor": np.float32(info.scale_factor),
               "picked": np.array(info.picked[:info.n_picked], np.int32)}
        if triangles:
            out.update(triangles=tris[:nt].copy(), tri_dist=dist[:nt].copy(), tri_ref=ref[:nt].copy())
        # (the library writes nc rows of n_stars, one behind the other)
        rows = ref_index.reshape(-1)[:nc * stars.size].reshape(nc, stars.size).copy()
        return cands[:nc].copy(), rows, out

    def match_stars(self, transforms, stars):
        """findBestMatch's matching alone (:194-206) for the caller's transforms (n x 6): (ref_index, num_matches)."""
        stars = np.ascontiguousarray(stars, dtype=capi.STAR_DTYPE)
        t = np.ascontiguousarray(transforms, dtype=np.float32).reshape(-1, 6)
        ref_index = np.zeros((t.shape[0], max(stars.size, 1)), np.int32)
        counts = np.zeros(max(t.shape[0], 1), np.int32)
        p32 = C.POINTER(C.c_int32)
        capi.check(self._lib.nl_aligner_match_stars(self._h, capi.fptr(t), t.shape[0], stars.ctypes.data_as(C.c_void_p),
                                                    int(stars.size), ref_index.ctypes.data_as(p32),
                                                    counts.ctypes.data_as(p32)))
        return ref_index[:, :stars.size].copy(), counts[:t.shape[0]].copy()


def _deband(call, percentile, window, sigma, location, scale):
    """One nl_*deband_* call through `call(<parameters from percentile on>)`: the dict of nl_deband_t."""
    info = capi.Deband()
    capi.check(call(float(percentile), int(window), float(sigma), float(location), float(scale), C.byref(info)))
    return {name: np.float32(getattr(info, name)) for name, _ in capi.Deband._fields_}


def _deband_host(entry, frame, width, height, percentile, window, sigma, location, scale, device):
    out = _host_frame(frame, width, height)
    info = _deband(lambda *a: entry(capi.fptr(out), int(width), int(height), *a, _device(device)),
                   percentile, window, sigma, location, scale)
    return out, info


def deband_horiz(frame, width, height, percentile=50.0, window=128, sigma=3.0, location=0.0, scale=0.0, device=None):
    """OpDebandHoriz (internal/ops/pre/banding.go:61-132) on one host frame on `device` (default 0): every row is
    scaled so that its percentile (over the samples <= location + sigma * scale; sigma 0: all finite ones) meets the
    median of the percentiles in a window of rows.  location / scale: the frame's Stats.Location() / Scale().
    Returns (out, info): info the dict of nl_deband_t (threshold, lowest, highest); under the operator's own guards
    out is the frame unchanged and info (threshold, 1, 0)."""
    return _deband_host(capi.load().nl_deband_horiz, frame, width, height, percentile, window, sigma, location, scale,
                        device)


def deband_vert(frame, width, height, percentile=50.0, window=128, sigma=3.0, location=0.0, scale=0.0, device=None):
    """OpDebandVert (internal/ops/pre/banding.go:197-270): deband_horiz over columns."""
    return _deband_host(capi.load().nl_deband_vert, frame, width, height, percentile, window, sigma, location, scale,
                        device)


def bin_shape(width, height, n):
    """The (width, height) OpBin gives a frame: (width // n, height // n), unchanged for n <= 1 (host only)."""
    w, h = C.c_int(0), C.c_int(0)
    capi.check(capi.load().nl_bin_shape(int(width), int(height), int(n), C.byref(w), C.byref(h)))
    return int(w.value), int(h.value)


def bin_nxn(frame, width, height, n, device=None):
    """fits.NewImageBinNxN (internal/fits/fits.go:163-195) of one host frame on `device` (default 0); n <= 1 copies.
    Returns (out, out_width, out_height)."""
    frame = _host_frame(frame, width, height, copy=False)
    ow, oh = bin_shape(width, height, n)
    out = np.empty(ow * oh, np.float32)
    capi.check(capi.load().nl_bin_nxn(capi.fptr(frame), int(width), int(height), int(n), capi.fptr(out),
                                      _device(device)))
    return out, ow, oh


def gaussian_kernel_1d(sigma, capacity=None):
    """GaussianKernel1D (internal/ops/stretch/usm.go:41-82): the taps for `sigma` as float32 (host only).  capacity:
    the room offered to the library (default: the tap count, asked for first)."""
    lib = capi.load()
    n = C.c_int(0)
    if capacity is None:
        rc = lib.nl_gaussian_kernel_1d(float(sigma), None, 0, C.byref(n))
        if rc != capi.OK and n.value == 0:
            capi.check(rc)
        capacity = n.value
    taps = np.empty(max(int(capacity), 1), np.float32)
    capi.check(lib.nl_gaussian_kernel_1d(float(sigma), capi.fptr(taps), int(capacity), C.byref(n)))
    return taps[:n.value].copy()


def lanczos3_table():
    """The library's Lanczos-3 table, [RS_PHASES, 6] float32 (include/nlstack_resample.h; host only, no device)."""
    table = np.empty((capi.RS_PHASES, 6), np.float32)
    capi.check(capi.load().nl_resample_lanczos3_table(capi.fptr(table)))
    return table


def drizzle_geometry(trans, scale, pixfrac=1.0):
    """(src_to_out, out_to_src, half_width, radius) of a drizzle of the forward transform `trans` onto a grid of
    `scale` pixels per reference pixel with drops of `pixfrac` (include/nlstack_drizzle.h; host only, no device)."""
    t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
    f, g = np.empty(6, np.float32), np.empty(6, np.float32)
    hw, radius = C.c_float(0.0), C.c_int(0)
    capi.check(capi.load().nl_drizzle_geometry(capi.fptr(t), float(scale), float(pixfrac), capi.fptr(f), capi.fptr(g),
                                               C.byref(hw), C.byref(radius)))
    return f, g, np.float32(hw.value), int(radius.value)


def drizzle_square_geometry(trans, scale, pixfrac=1.0):
    """(src_to_out, out_to_src, corners, box_half, radius) of a square drizzle: corners is float32 (4, 2), the corners
    of a drop relative to its centre in output pixels in the order the kernel walks them; box_half = (bx, by), the
    half-sides of the drop's bounding box (include/nlstack_sqdrizzle.h; host only, no device)."""
    t = np.ascontiguousarray(trans, dtype=np.float32).reshape(6)
    f, g = np.empty(6, np.float32), np.empty(6, np.float32)
    corners, box = np.empty(8, np.float32), np.empty(2, np.float32)
    radius = C.c_int(0)
    capi.check(capi.load().nl_drizzle_square_geometry(capi.fptr(t), float(scale), float(pixfrac), capi.fptr(f), capi.fptr(g),
                                                      capi.fptr(corners), capi.fptr(box), C.byref(radius)))
    return f, g, corners.reshape(4, 2), box, int(radius.value)


def drizzle_cfa_transform(trans_debayered, cfa):
    """The forward transform of the raw `cfa` mosaic that belongs to `trans_debayered`, a transform estimated on a
    plane debayered from it: plane pixel (x, y) is mosaic pixel (x + xo, y + yo) (include/nlstack_cfadrizzle.h; host
    only, no device)."""
    t = np.ascontiguousarray(trans_debayered, dtype=np.float32).reshape(6)
    out = np.empty(6, np.float32)
    capi.check(capi.load().nl_drizzle_cfa_transform(capi.fptr(t), _cstr(cfa), capi.fptr(out)))
    return out


def blur_tap_paths(n_taps):
    """(row_staged, col_staged): whether the row and the column pass of an n_taps kernel stage their tile in LDS or
    take every tap from global memory (developer query)."""
    row, col = C.c_int(0), C.c_int(0)
    capi.check(capi.load().nl_blur_tap_paths(int(n_taps), C.byref(row), C.byref(col)))
    return bool(row.value), bool(col.value)


def convolve_separable(frame, width, height, taps, device=None):
    """Convolve1DX then Convolve1DY (usm.go:85-114) of one host frame with the caller's taps on `device` (default 0);
    bit-exact.  Returns the filtered frame."""
    out = _host_frame(frame, width, height)
    t = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
    capi.check(capi.load().nl_convolve_separable(capi.fptr(out), int(width), int(height), capi.fptr(t) if t.size else None,
                                                 int(t.size), _device(device)))
    return out


def gaussian_blur(frame, width, height, sigma, device=None):
    """OpGaussianBlur (internal/ops/stretch/stretch.go:368-376) of one host frame; sigma 0 returns it unchanged."""
    out = _host_frame(frame, width, height)
    capi.check(capi.load().nl_gaussian_blur(capi.fptr(out), int(width), int(height), float(sigma),
                                            _device(device)))
    return out


def unsharp_mask(frame, width, height, sigma, gain, min, max, abs_threshold, device=None):
    """UnsharpMask (usm.go:153-159) of one host frame: pixels below abs_threshold stay, the others become
    d + (d - blurred) * gain clipped to min, then max; sigma 0 or gain 0 returns the frame unchanged."""
    src = _host_frame(frame, width, height, copy=False)
    out = np.empty_like(src)
    capi.check(capi.load().nl_unsharp_mask(capi.fptr(src), capi.fptr(out), int(width), int(height), float(sigma),
                                           float(gain), float(min), float(max), float(abs_threshold),
                                           _device(device)))
    return out


def _tone(call, kind, p, stats):
    """call(curve, mn, mean, mx) with the nl_tone_t of kind and its arguments p; the statistics when asked for."""
    assert len(p) <= 3
    t = capi.Tone(int(kind), (C.c_float * 3)(*[float(v) for v in p]))
    if not stats:
        capi.check(call(C.byref(t), None, None, None))
        return None
    mn, mean, mx = C.c_float(), C.c_float(), C.c_float()
    capi.check(call(C.byref(t), C.byref(mn), C.byref(mean), C.byref(mx)))
    return np.float32(mn.value), np.float32(mean.value), np.float32(mx.value)


def tone(frame, kind, *p, stats=False, device=None):
    """One per-pixel curve of the reference's stretch command (internal/fits/pixelops.go) over a host frame on
    `device` (default 0).  kind and p, the pixel function's own arguments: capi.TONE_SCALE_OFFSET (scale, offset),
    TONE_NORMALIZE (min, max), TONE_GAMMA (g), TONE_PARTIAL_GAMMA (from, to, g), TONE_MIDTONES (mid, black),
    TONE_SHIFT_BLACK (before, after).  Bit-exact but for pixels whose power falls on a rounding boundary (one fp32 ulp).
    Returns the transformed frame; with stats=True (frame, (min, mean, max)) from the same pass."""
    out = _host_frame(frame)
    dev = _device(device)
    st = _tone(lambda *a: capi.load().nl_tone(capi.fptr(out), int(out.size), *a, dev), kind, p, stats)
    return (out, st) if stats else out


def _export_gray(call, n, min, max, gamma, bits):
    """call(min, max, gamma, bits, out) into n counts: uint8, or big-endian uint16 as the bytes lie in image.Gray16.Pix"""
    raw = np.empty(int(n) * (2 if int(bits) == 16 else 1), np.uint8)
    capi.check(call(float(min), float(max), float(gamma), int(bits), raw.ctypes.data_as(C.c_void_p)))
    return raw.view(">u2") if int(bits) == 16 else raw


def export_gray(frame, min, max, gamma=1.0, bits=16, device=None):
    """OpSave's pixel loop (WriteMonoTIFF16 / WriteMonoJPG) over a host frame: (d - min) / (max - min) clipped to
    [0, 1] (NaN: 0), gamma, then counts of 16 bits (returned as big-endian uint16, the byte layout of Go's
    image.Gray16.Pix) or 8 bits (uint8) by truncation."""
    src = _host_frame(frame, copy=False)
    dev = _device(device)
    return _export_gray(lambda *a: capi.load().nl_export_gray(capi.fptr(src), int(src.size), *a, dev), src.size, min,
                        max, gamma, bits)


def _planes(planes):
    assert len(planes) == 3
    return (C.c_int * 3)(*[int(v) for v in planes])


def _f32x3(v):
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    assert a.size == 3
    return a


def _rgb_in(v):
    return capi.Rgb(*[float(x) for x in v])


def _rgb_out(c):
    return np.array([c.r, c.g, c.b], np.float32)


def rgb_normalization(mins, maxs):
    """getCommonNormalizationFactors (rgb.go:65-78) of the channels' Stats.Min() / Max(): (min, mult).  Host only."""
    mn, mult = C.c_float(), C.c_float()
    capi.check(capi.load().nl_rgb_normalization(capi.fptr(_f32x3(mins)), capi.fptr(_f32x3(maxs)), C.byref(mn),
                                                C.byref(mult)))
    return np.float32(mn.value), np.float32(mult.value)


def rgb_balance_coeffs(cur_shadows, cur_highlights, target_shadows, target_highlights):
    """The scalar part of setBlackWhitePoints (rgb.go:125-145): (alpha[3], beta[3]).  Host only."""
    alpha, beta = np.zeros(3, np.float32), np.zeros(3, np.float32)
    capi.check(capi.load().nl_rgb_balance_coeffs(_rgb_in(cur_shadows), _rgb_in(cur_highlights), _rgb_in(target_shadows),
                                                 _rgb_in(target_highlights), capi.fptr(alpha), capi.fptr(beta)))
    return alpha, beta


def _rgb_balance(call, stars, block, border, skip_bright, skip_dim, shadows, highlights, loc, scale):
    """One nl_*rgb_balance call through `call(<parameters from stars on>)`: the dict of nl_rgb_balance_t."""
    stars = np.ascontiguousarray(np.zeros(0, capi.STAR_DTYPE) if stars is None else stars, dtype=capi.STAR_DTYPE)
    rep = capi.RgbBalance()
    capi.check(call(stars.ctypes.data_as(C.c_void_p), int(stars.size), int(block), float(border), float(skip_bright),
                    float(skip_dim), _rgb_in(shadows), _rgb_in(highlights), capi.fptr(_f32x3(loc)),
                    capi.fptr(_f32x3(scale)), C.byref(rep)))
    out = {k: np.array(getattr(rep, k), np.float32) for k in ("alpha1", "beta1", "alpha2", "beta2")}
    out["darkest"], out["stars"] = _rgb_out(rep.darkest), _rgb_out(rep.stars)
    return out


def rgb_balance(planar, width, height, stars, block, border, skip_bright, skip_dim, shadows, highlights, loc, scale,
                device=None):
    """SetBlackWhitePoints (rgb.go:94-120) of a planar RGB image (3 * width * height floats, fits.Image.Data) on
    `device` (default 0): loc / scale are the channels' Stats.Location() / Scale(), shadows / highlights the target
    colours.  Bit-exact.  Returns (balanced image, report dict)."""
    out = _host_frame(planar, width, height, planes=3)
    lib = capi.load()
    rep = _rgb_balance(lambda *a: lib.nl_rgb_balance(capi.fptr(out), int(width), int(height), *a,
                                                     _device(device)),
                       stars, block, border, skip_bright, skip_dim, shadows, highlights, loc, scale)
    return out, rep


def _export_rgb(call, n, min, max, gamma, bits):
    """call(min, max, gamma, bits, out) into n pixels of R G B A: an (n, 4) array of uint8, or of big-endian uint16 as
    the bytes lie in image.RGBA64.Pix"""
    raw = np.empty(int(n) * (8 if int(bits) == 16 else 4), np.uint8)
    capi.check(call(float(min), float(max), float(gamma), int(bits), raw.ctypes.data_as(C.c_void_p)))
    return (raw.view(">u2") if int(bits) == 16 else raw).reshape(-1, 4)


def export_rgb(planar, min, max, gamma=1.0, bits=16, device=None):
    """The pixel loop of WriteTIFF16 (bits 16) / WriteJPG (bits 8) over a planar RGB image (3 * n floats): per pixel
    R G B A with A all ones, as image.RGBA64.Pix / image.RGBA.Pix hold them."""
    src = _host_frame(planar, copy=False, planes=3)
    dev = _device(device)
    return _export_rgb(lambda *a: capi.load().nl_export_rgb(capi.fptr(src), src.size // 3, *a, dev), src.size // 3, min,
                       max, gamma, bits)


def _cstr(s):
    return (s or "").encode("utf-8")


def debayer_shape(width, height, channel, cfa):
    """The (width, height) OpDebayer gives a frame: unchanged when channel or cfa is "" (host only)."""
    w, h = C.c_int(0), C.c_int(0)
    capi.check(capi.load().nl_debayer_shape(int(width), int(height), _cstr(channel), _cstr(cfa), C.byref(w),
                                            C.byref(h)))
    return int(w.value), int(h.value)


def preprocess_frame_cfa(frame, width, height, channel, cfa="RGGB", calib=None, sigma_low=3.0, sigma_high=5.0,
                         frame_id=0, device=None):
    """OpCalibrate, OpBadPixel and OpDebayer on one host frame, on calib's device (else `device`, default 0).
    Returns (out, out_width, out_height, removed, (mean, std)): the Bayer branch's delta statistics, or the mono
    MedianDiffStats when channel is ""."""
    frame = _host_frame(frame, width, height, copy=False)
    if device is None:
        device = calib.device if calib is not None else 0
    lib = capi.load()
    ow, oh = C.c_int(0), C.c_int(0)
    # (an unknown CFA or channel is reported by the entry point itself, in the reference's order)
    rc = lib.nl_debayer_shape(int(width), int(height), _cstr(channel), _cstr(cfa), C.byref(ow), C.byref(oh))
    out = np.empty(max(ow.value * oh.value, 1) if rc == capi.OK else 1, np.float32)
    removed, stats = C.c_int64(0), (C.c_float * 2)()
    capi.check(lib.nl_preprocess_frame_cfa(None if calib is None else calib._c, int(frame_id), capi.fptr(frame),
                                           int(width), int(height), _cstr(channel), _cstr(cfa), float(sigma_low),
                                           float(sigma_high), capi.fptr(out), C.byref(ow), C.byref(oh),
                                           C.byref(removed), stats, int(device)))
    return (out[:ow.value * oh.value], int(ow.value), int(oh.value), int(removed.value),
            (np.float32(stats[0]), np.float32(stats[1])))


def median_filter_3x3(image, width, height, device=0):
    lib = capi.load()
    src = np.ascontiguousarray(image, dtype=np.float32).reshape(-1)
    dst = np.empty_like(src)
    capi.check(lib.nl_median_filter_3x3(capi.fptr(src), capi.fptr(dst), int(width), int(height),
                                        int(device)))
    return dst


def median_filter_mask(data, mask, device=0):
    """MedianFilter (ops/pre/badpixels.go:54-77): out[i] = median of data[i + mask[j]] inside the data."""
    lib = capi.load()
    src = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
    m = np.ascontiguousarray(mask, dtype=np.int32)
    dst = np.empty_like(src)
    capi.check(lib.nl_median_filter_mask(capi.fptr(src), capi.fptr(dst), src.size,
                                         m.ctypes.data_as(C.POINTER(C.c_int32)), m.size, int(device)))
    return dst
