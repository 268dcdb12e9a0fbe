/* nlstack_resample.h -- bicubic and Lanczos-3 resampling for the resident projection, entries of the C ABI of
 * libnlstack.so.  AN EXTENSION: the reference's Image.Project resamples bilinearly and knows no other kernel.  Part of
 * nlstack.h, which includes it behind the types it needs: include nlstack.h, not this file. */
#ifndef NLSTACK_RESAMPLE_H
#define NLSTACK_RESAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the resident projection with a wider resampling kernel (labelled extension) ----
 * nl_stack_frame_project_from resamples bilinearly because Image.Project does (internal/fits/project.go:26-76).
 * Bilinear interpolation is a low-pass filter whose strength depends on the sub-pixel phase, so every aligned frame
 * gets a different blur.  The entries declared here project a resident frame exactly as nl_stack_frame_project_from
 * does -- the same handles, transform, checks and errors -- with the resampling kernel of the caller's choice.
 * nl_stack_frame_project_from, nl_group_frame_project_from and the projected uploads stay what they are.  There is
 * no reference to compare the wide kernels with: this text is the contract.
 *
 * Definition.  For destination pixel (col, row) compute X, Y, fx = floor(X), fy = floor(Y), the range tests,
 * xl = (int)fx, yl = (int)fy, xr = X - (float)xl and yr = Y - (float)yl exactly as the bilinear projection does
 * (coord.go:142-143, project.go:52-56).  xr and yr are exact and lie in [0, 1).
 *
 * A kernel has radius R: 1 for NL_RS_BILINEAR, 2 for NL_RS_BICUBIC, 3 for NL_RS_LANCZOS3.  Its footprint is the
 * columns xl-(R-1) ... xl+R and the rows yl-(R-1) ... yl+R of the source.
 *
 * Three cases per pixel.
 *   - The 2x2 footprint does not fit in the source (the bilinear projection's test): the result is out_of_bounds.
 *   - The 2x2 footprint fits but the wide one does not (xl-(R-1) < 0, xl+R > src_w-1, or the same in y): the result is
 *     the bilinear value, bit for bit what nl_stack_frame_project_from gives.  The valid area and the coverage of a
 *     stack therefore do not depend on the kernel.
 *   - The wide footprint fits: the result is the separable sum below.
 *
 * Separable sum.  fp32, never fused, left to right; t[j][i] is the tap in footprint row j and footprint column i.
 *   For j = 0 ... 2R-1:  r_j = (((t[j][0]*wx[0] + t[j][1]*wx[1]) + t[j][2]*wx[2]) + ...)
 *   then                 v   = (((r_0*wy[0] + r_1*wy[1]) + r_2*wy[2]) + ...)
 * Non-finite taps take part as they are: a NaN tap gives NaN, Inf*0 gives NaN.
 *
 * Bicubic weights: Keys with a = -0.5 (Catmull-Rom), as Horner forms in fp32 with t = xr (wy: the same with t = yr).
 *   w0 = ((-0.5f*t + 1)*t - 0.5f)*t
 *   w1 = (1.5f*t - 2.5f)*t*t + 1
 *   w2 = ((-1.5f*t + 2)*t + 0.5f)*t
 *   w3 = (0.5f*t - 0.5f)*t*t
 *
 * Lanczos-3 weights: from a table of NL_RS_PHASES = 1024 rows of 6 fp32 values.  Row q belongs to f = q/1024; tap i
 * is at distance x = f - (i-2).  L(x) = 3 sin(pi x) sin(pi x/3) / (pi^2 x^2) is evaluated in double, with L(0) = 1 and
 * L exactly 0 at every other integer x, so row 0 is exactly (0,0,1,0,0,0).  Each row is divided by its sum in double
 * and then rounded to fp32.  The library builds the table once on the host and keeps one copy per device;
 * nl_resample_lanczos3_table returns it.  The phase of a pixel is q = (int)(xr * 1024.0f): the multiplication is exact
 * and q <= 1023; wx = row q, and wy = the row of (int)(yr * 1024.0f).  The device result is BIT-EXACT GIVEN THE TABLE,
 * in the sense in which the blur is bit-exact given the taps.
 *
 * Clamp (optional; it takes out the dark rings Lanczos draws around stars).  t00, t01, t10, t11 are the four taps of
 * the 2x2 footprint (t01 = row yl, column xl+1).  lo = t00; for t in (t01, t10, t11): if (t < lo) lo = t.  hi the same
 * way with >.  Then if (v < lo) v = lo; if (v > hi) v = hi.  The comparisons are literal, so the chain fixes what
 * happens with NaN.  The clamp is a no-op for NL_RS_BILINEAR and for the pixels that fall back to the bilinear value. */
#define NL_RS_BILINEAR 0
#define NL_RS_BICUBIC 1
#define NL_RS_LANCZOS3 2
#define NL_RS_PHASES 1024

/* The Lanczos-3 table of the definition above into table[NL_RS_PHASES * 6], row after row.  Host only: it needs no
 * device.  NL_ERR_INVALID_ARG for a null pointer. */
int nl_resample_lanczos3_table(float *table /* NL_RS_PHASES * 6 */);

/* nl_stack_frame_project_from / nl_group_frame_project_from with the resampling kernel `kernel` (NL_RS_*) and, with
 * clamp != 0, the clamp.  The checks are those of nl_stack_frame_project_from; an unknown kernel gives
 * NL_ERR_INVALID_ARG before any device work.  NL_RS_BILINEAR runs the bilinear projection's own kernel, so a caller
 * switches kernels with one field.  Synchronous like the calls they extend. */
int nl_stack_frame_resample_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                                 float out_of_bounds, int kernel, int clamp);
int nl_group_frame_resample_from(nl_group_t *g, int idx, nl_stack_t *src, int src_idx, const float trans[6],
                                 float out_of_bounds, int kernel, int clamp);

/* Developer query, what nl_stack_project_tile_paths is for the bilinear kernel: of the workgroup tiles that
 * nl_stack_frame_resample_from(dst, ., src, src_idx, trans, ., kernel, .) launches, how many stage their source box
 * in LDS and how many take their taps from global memory.  Host arithmetic only, the kernel's own, so the counts are
 * exact.  The developer switches 32768 and 65536 of nl_stack_set_dev_flags on dst hold for the wide kernels as they
 * do for the bilinear one. */
int nl_stack_resample_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], int kernel,
                                 int64_t *staged, int64_t *direct);

#ifdef __cplusplus
}
#endif

#endif
