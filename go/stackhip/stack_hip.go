// Package stack -- drop-in replacement for the reference's
// internal/ops/stack/stack.go that runs OpStack.Apply on an AMD MI355X through
// libnlstack.so (C ABI: include/nlstack.h).
//
// NOT compiled in the build image (no Go toolchain there): this file is the
// binding a Nightlight maintainer adds.  It keeps the package name, the
// operator type string "stack", the JSON fields, the constructor names and the
// Apply signature of the reference (stack.go:66-115), so cmd/nightlight/main.go
// and internal/ops/stack/stackbatches.go compile against it unchanged.  Build
// with:  go build -tags=jsoniter,hip ./cmd/nightlight   (and drop stack.go's
// Apply behind `//go:build !hip`).
//
//go:build hip

package stack

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../nightlight_amd -lnlstack -Wl,-rpath,${SRCDIR}/../../nightlight_amd
#include <stdlib.h>
#include "nlstack.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/mlnoga/nightlight/internal/fits"
	"github.com/mlnoga/nightlight/internal/ops"
)

// Devices lists the GPUs this process stacks on: every stack is split into one row tile per
// entry (nl_group_*, the same pixel-range split the reference makes over goroutines,
// stack.go:142-152), the clip counters are summed on the host.  nil = all visible GPUs.
var Devices []int

// lastError reads the calling OS thread's message.  nl_last_error() is thread-local and a
// goroutine may migrate between the failing cgo call and this one, so every call+error pair
// runs under runtime.LockOSThread (see Apply).
func lastError() error { return errors.New(C.GoString(C.nl_last_error())) }

// ProjectFrom is the f.Project call of OpAlign.Apply (internal/ops/post/postprocess.go:185) for a frame that is
// resident on the device: slot srcIdx of the whole-image staging handle src, resampled through the forward
// transform {A,B,C,D,E,F} into slot dstIdx of the stack handle dst (any row tile).  The handles are the
// *C.nl_stack_t of nl_stack_create as unsafe.Pointer.  The source slot stays as it is and may be overwritten on return.
func ProjectFrom(dst unsafe.Pointer, dstIdx int, src unsafe.Pointer, srcIdx int, trans [6]float32, outOfBounds float32) error {
	runtime.LockOSThread() // nl_last_error() is per OS thread
	defer runtime.UnlockOSThread()
	if rc := C.nl_stack_frame_project_from((*C.nl_stack_t)(dst), C.int(dstIdx), (*C.nl_stack_t)(src), C.int(srcIdx),
		(*C.float)(unsafe.Pointer(&trans[0])), C.float(outOfBounds)); rc != C.NL_OK {
		return lastError()
	}
	return nil
}

// GroupProjectFrom is ProjectFrom into slot idx of every tile of a group (*C.nl_group_t): each tile projects its own rows.
func GroupProjectFrom(g unsafe.Pointer, idx int, src unsafe.Pointer, srcIdx int, trans [6]float32, outOfBounds float32) error {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.nl_group_frame_project_from((*C.nl_group_t)(g), C.int(idx), (*C.nl_stack_t)(src), C.int(srcIdx),
		(*C.float)(unsafe.Pointer(&trans[0])), C.float(outOfBounds)); rc != C.NL_OK {
		return lastError()
	}
	return nil
}

// ResampleFrom is ProjectFrom with a resampling kernel of the caller's choice (include/nlstack_resample.h): kernel 0 is
// the reference's bilinear interpolation, 1 bicubic (Catmull-Rom), 2 Lanczos-3; clamp holds every pixel to the range of
// its four nearest source pixels.  An EXTENSION, not in the reference: Image.Project resamples bilinearly.
func ResampleFrom(dst unsafe.Pointer, dstIdx int, src unsafe.Pointer, srcIdx int, trans [6]float32, outOfBounds float32,
	kernel int, clamp bool) error {
	runtime.LockOSThread() // nl_last_error() is per OS thread
	defer runtime.UnlockOSThread()
	c := C.int(0)
	if clamp {
		c = 1
	}
	if rc := C.nl_stack_frame_resample_from((*C.nl_stack_t)(dst), C.int(dstIdx), (*C.nl_stack_t)(src), C.int(srcIdx),
		(*C.float)(unsafe.Pointer(&trans[0])), C.float(outOfBounds), C.int(kernel), c); rc != C.NL_OK {
		return lastError()
	}
	return nil
}

// GroupResampleFrom is ResampleFrom into slot idx of every tile of a group (*C.nl_group_t): each tile resamples its own rows.
func GroupResampleFrom(g unsafe.Pointer, idx int, src unsafe.Pointer, srcIdx int, trans [6]float32, outOfBounds float32,
	kernel int, clamp bool) error {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	c := C.int(0)
	if clamp {
		c = 1
	}
	if rc := C.nl_group_frame_resample_from((*C.nl_group_t)(g), C.int(idx), (*C.nl_stack_t)(src), C.int(srcIdx),
		(*C.float)(unsafe.Pointer(&trans[0])), C.float(outOfBounds), C.int(kernel), c); rc != C.NL_OK {
		return lastError()
	}
	return nil
}

// LocationScale is Stats.Location() / Scale() (internal/stats/stats.go:225-244) of a frame that is resident on the
// device: slot idx of the whole-image handle h (idx < 0: the last pass's result), with the estimator the reference
// runs (stats.LSEstimator as an int, 3 = LSESCMedianQn by default; 2 = LSEIKSS is not implemented on the device).
// The reference seeds every sampling call from the clock; here the seeds of one estimate derive from key, and the
// result is the reference's for those seeds, bit for bit.  minMax: nil, or the cached Stats.Min() / Max() where
// UpdateCachedWith has moved them away from the frame's own.
func LocationScale(h unsafe.Pointer, idx int, estimator int, key uint64, minMax *[2]float32) (location, scale float32, err error) {
	runtime.LockOSThread() // nl_last_error() is per OS thread
	defer runtime.UnlockOSThread()
	var seeds [C.NL_LOCSCALE_MAX_SEEDS]C.uint32_t
	C.nl_locscale_seeds(C.uint64_t(key), &seeds[0], C.NL_LOCSCALE_MAX_SEEDS)
	var mm *C.float
	if minMax != nil {
		mm = (*C.float)(unsafe.Pointer(&minMax[0]))
	}
	var l, s C.float
	if rc := C.nl_stack_frame_location_scale((*C.nl_stack_t)(h), C.int(idx), C.int(estimator), C.NL_LOCSCALE_SAMPLES,
		&seeds[0], C.NL_LOCSCALE_MAX_SEEDS, mm, &l, &s, nil); rc != C.NL_OK {
		return 0, 0, lastError()
	}
	return float32(l), float32(s), nil
}

// GroupRunMaps is one stack pass over the tiles of a group (*C.nl_group_t) that also says where it clipped
// (include/nlstack_maps.h): rejectLow[p] / rejectHigh[p] count the increments of numClippedLow / numClippedHigh at
// pixel p (stack.go:411-424 and its siblings), their sums are the two totals; out is the bit-exact result.  All three
// are whole-image slices of width*height elements; nil leaves that output out.  The reference has no counterpart: it
// keeps the totals only.
func GroupRunMaps(g unsafe.Pointer, mode StackMode, sigmaLow, sigmaHigh, refFrameLoc float32, out []float32,
	rejectLow, rejectHigh []uint16) (clipLow, clipHigh int64, err error) {
	runtime.LockOSThread() // nl_last_error() is per OS thread
	defer runtime.UnlockOSThread()
	var o *C.float
	var lo, hi *C.uint16_t
	if out != nil {
		o = (*C.float)(unsafe.Pointer(&out[0]))
	}
	if rejectLow != nil {
		lo = (*C.uint16_t)(unsafe.Pointer(&rejectLow[0]))
	}
	if rejectHigh != nil {
		hi = (*C.uint16_t)(unsafe.Pointer(&rejectHigh[0]))
	}
	var cl, ch C.int64_t
	if rc := C.nl_group_run_maps((*C.nl_group_t)(g), C.int(mode), C.float(sigmaLow), C.float(sigmaHigh),
		C.float(refFrameLoc), o, &cl, &ch, lo, hi); rc != C.NL_OK {
		return 0, 0, lastError()
	}
	return int64(cl), int64(ch), nil
}

// GroupCoverage fills coverage (width*height elements) with the number of frames that have a sample at each pixel:
// the n the gather of every Stack* function leaves (stack.go:380-387).
func GroupCoverage(g unsafe.Pointer, coverage []uint16) error {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	if rc := C.nl_group_coverage((*C.nl_group_t)(g), (*C.uint16_t)(unsafe.Pointer(&coverage[0]))); rc != C.NL_OK {
		return lastError()
	}
	return nil
}

// Apply stacks a set of light frames on the GPUs.  Same contract as
// internal/ops/stack/stack.go:115-227: mode validation and auto selection,
// weights from getWeights (kept in Go, stack.go:231-270), one result image with
// the summed exposure, the "Clipped low ..." log line from the counters.
func (op *OpStack) Apply(f []*fits.Image, c *ops.Context) (result *fits.Image, err error) {
	mode := op.Mode
	if mode < StMedian || mode > StAuto {
		return nil, errors.New("invalid stacking mode")
	}
	if mode == StAuto {
		mode = autoSelectStackingMode(len(f))
	}
	fmt.Fprintf(c.Log, "Stacking %d frames with stacking mode %d and sigma low %g high %g:\n",
		len(f), mode, op.SigmaLow, op.SigmaHigh)

	weights, err := getWeights(f, op.Weighting)
	if err != nil {
		return nil, err
	}
	if mode == StMADSigma && weights != nil && !op.WeightsFollowFrames { // (with the switch: nl_group_run_mad_weighted, below)
		return nil, errors.New("MADSigma stacking with weights is still unimplemented") // reference panics, stack.go:185
	}

	// the reference indexes every frame with the first frame's length (stack.go:151) and would
	// panic on a short one; the C side cannot see slice lengths, so check here
	for _, l := range f {
		if len(l.Data) != len(f[0].Data) {
			return nil, fmt.Errorf("%d: frame has %d pixels, expected %d", l.ID, len(l.Data), len(f[0].Data))
		}
	}

	runtime.LockOSThread() // nl_last_error() is per OS thread
	defer runtime.UnlockOSThread()

	width, height := int(f[0].Naxisn[0]), len(f[0].Data)/int(f[0].Naxisn[0])
	var devs *C.int
	if len(Devices) > 0 {
		cdev := make([]C.int, len(Devices))
		for i, d := range Devices {
			cdev[i] = C.int(d)
		}
		devs = &cdev[0]
	}
	// One group per Apply, as the reference allocates per call (stack.go:131-138).  nl_group_destroy parks the large
	// device buffers, the next Apply with the same geometry takes them over (bench.py "fresh_handle": create + destroy
	// 3 ms for the first handle of a process, well below one pass afterwards); C.nl_release_cached_memory() returns
	// them to the driver when the process is done stacking.
	g := C.nl_group_create(C.int(len(f)), C.int(width), C.int(height), C.int(len(Devices)), devs)
	if g == nil {
		return nil, lastError()
	}
	defer C.nl_group_destroy(g)

	// one cgo call per Go slice: [][]float32 cannot cross cgo, and the copy builds the planar
	// [N][rows*W] layout of every device tile on the way.  Each tile copies its rows into its
	// own pinned staging buffer before the call returns (no Go pointer is retained) and the
	// DMA of frame i overlaps the staging of frame i+1; the pass waits for them on the device.
	for i, l := range f {
		if rc := C.nl_group_upload_frame(g, C.int(i), (*C.float)(unsafe.Pointer(&l.Data[0]))); rc != C.NL_OK {
			return nil, lastError()
		}
	}
	var wp *C.float
	if weights != nil {
		wp = (*C.float)(unsafe.Pointer(&weights[0]))
	}
	if rc := C.nl_group_set_weights(g, wp); rc != C.NL_OK {
		return nil, lastError()
	}

	data := make([]float32, len(f[0].Data))
	var clipLow, clipHigh C.int64_t
	// An EXTENSION, not in the reference (include/nlstack_wlinfit.h): OpStack gains the field
	//	WeightedLinearFit bool `json:"weightedLinearFit,omitempty"`
	// in stack.go's struct (default false, so existing JSON round-trips unchanged).  When it is set, the mode
	// resolves to the linear fit and there are weights, the fit rejects as always and the survivors are averaged
	// with the weights; otherwise the linear fit drops the weights as the reference does (stack.go:188-189).
	// Another EXTENSION (include/nlstack_wclip.h): the field
	//	WeightsFollowFrames bool `json:"weightsFollowFrames,omitempty"`
	// When it is set, the mode resolves to sigma or winsorized sigma clipping and there are weights, the rejection runs
	// as always and each survivor is averaged with ITS frame's weight; otherwise a survivor takes the weight that
	// QSelectMedianFloat32 left in its slot, as in the reference (stack.go:487).  With MAD sigma and weights
	// (include/nlstack_wmad.h) the same switch runs the MAD rejection and averages each survivor with its frame's weight;
	// without it that combination fails as above.
	var rc C.int
	if op.WeightedLinearFit && mode == StLinearFit && weights != nil {
		rc = C.nl_group_run_linfit_weighted(g, C.float(op.SigmaLow), C.float(op.SigmaHigh), C.float(op.RefFrameLoc),
			(*C.float)(unsafe.Pointer(&data[0])), &clipLow, &clipHigh)
	} else if op.WeightsFollowFrames && (mode == StSigma || mode == StWinsorSigma) && weights != nil {
		rc = C.nl_group_run_clip_weighted(g, C.int(mode), C.float(op.SigmaLow), C.float(op.SigmaHigh), C.float(op.RefFrameLoc),
			(*C.float)(unsafe.Pointer(&data[0])), &clipLow, &clipHigh)
	} else if op.WeightsFollowFrames && mode == StMADSigma && weights != nil {
		// (include/nlstack_wmad.h: without the switch weighted MAD sigma fails as in the reference)
		rc = C.nl_group_run_mad_weighted(g, C.float(op.SigmaLow), C.float(op.SigmaHigh), C.float(op.RefFrameLoc),
			(*C.float)(unsafe.Pointer(&data[0])), &clipLow, &clipHigh)
	} else {
		rc = C.nl_group_run(g, C.int(mode), C.float(op.SigmaLow), C.float(op.SigmaHigh), C.float(op.RefFrameLoc),
			(*C.float)(unsafe.Pointer(&data[0])), &clipLow, &clipHigh)
	}
	if rc != C.NL_OK {
		return nil, lastError()
	}
	if mode >= StSigma {
		fmt.Fprintf(c.Log, "Clipped low %d (%.2f%%) high %d (%.2f%%)\n",
			int64(clipLow), float32(clipLow)*100.0/(float32(len(data)*len(f))),
			int64(clipHigh), float32(clipHigh)*100.0/(float32(len(data)*len(f))))
	}

	exposureSum := float32(0)
	for _, l := range f {
		exposureSum += l.Exposure
	}
	stack := fits.NewImageFromNaxisn(f[0].Naxisn, data)
	stack.Exposure = exposureSum
	return stack, nil
}
