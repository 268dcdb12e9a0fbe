/* nlstack_align.h -- the alignment entries of the C ABI of libnlstack.so.  Part of nlstack.h, which includes it behind
 * the types it needs (nl_star_t): include nlstack.h, not this file. */
#ifndef NLSTACK_ALIGN_H
#define NLSTACK_ALIGN_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- OpAlign's estimate: star.Aligner up to the minimiser (internal/star/align.go:58-206) ----
 * What NewAligner and Align compute in front of gonum's Nelder-Mead, on the device: the triangles of the picked stars,
 * every triangle's nearest reference triangle, the shortlist of K candidates, each candidate's initial transform, and
 * per candidate every star's nearest reference star within 8 pixels.  The minimiser (:214-253), the residual and the
 * early exit at residual < 0.01 stay with the caller, which receives exactly what the objective function closes over.
 *
 * Bit-exact: every distance, index, transform and count is the reference's wherever the reference's own outcome does
 * not depend on the order Go's unstable sort.Slice leaves.  Both kd-trees (kdtree2.go, kdtree3p.go) prune on
 * distToPlane*distToPlane <= closestDsq and fp32 rounding is monotone, so they return the exact fp32 minimum of
 * dx*dx + dy*dy (+ dz*dz); the device finds the same minimum by brute force.  pickBrightestDistant (:86-104) and
 * NewTransform2D (coord.go:118-137) run on the host, literally: the latter rejects Inf (trans_ok = 0, the reference's
 * "divide by zero") and lets NaN through, and a NaN transform matches nothing.
 * Deviations:
 *   1. where two distinct reference points tie at the minimum distance the lowest index wins (the reference returns
 *      whichever its tree visits first, which depends on the order sort.Slice left).
 *   2. the shortlist is ordered by (dist, lowest tri_index); the reference's sort.Slice is unstable at equal dist.
 *   3. k > NL_ALIGN_MAX_K is an error; the reference takes any k.
 *   4. every candidate is evaluated; the reference's early exit (:250-252) is the caller's.
 * Errors, all NL_ERR_INVALID_ARG with a message naming the site, in front of the device check where they need no
 * device: null pointers; k <= 0 or above the cap; n_ref_stars <= 0 ("Unable to align without star detections in
 * reference frame", postprocess.go:203); n_stars <= 0; frame_width <= 0; capacities too small; a frame with triangles
 * against a reference with none (the reference indexes an empty tree and panics).  Fewer than 3 picked stars, or no
 * triangle in the frame, is no error: *n_cands = 0, as the reference returns the zero transform and MaxFloat32.
 * Without a device nl_aligner_create, nl_aligner_match and nl_aligner_match_stars fail with NL_ERR_NO_DEVICE. */
#define NL_ALIGN_MAX_K 128
typedef struct nl_aligner nl_aligner_t;
/* star.Triangle (align.go:39-46): same field order and size; a, b, c index the star list */
typedef struct nl_align_triangle {
    float d_ab, d_ac, d_bc;
    int32_t a, b, c;
} nl_align_triangle_t;
/* one entry of the shortlist (Match, :49-53) and what findBestMatch derives from it in front of the minimiser */
typedef struct nl_align_candidate {
    float dist;                      /* squared distance of the two triangles in (dAB, dAC, dBC) space */
    int32_t tri_index, ref_tri_index;
    int32_t a, b, c;                 /* the frame triangle's stars (:169-172) */
    int32_t ref_a, ref_b, ref_c;     /* the reference triangle's stars (:173-176) */
    float trans[6];                  /* NewTransform2D's A .. F (:177); zeros when trans_ok == 0 */
    int32_t trans_ok;                /* 0 = "divide by zero": the reference skips the candidate, its ref_index row is -1 */
    int32_t num_matches;             /* stars with a reference star at dsq < 64 (:200-202) */
    int32_t enough;                  /* trans_ok && num_matches >= n_stars / 3, integer division (:210) */
} nl_align_candidate_t;
/* how a match came about; info may be NULL.  The three pointers are inputs: NULL, or room for tri_capacity elements
 * each, which then receive the frame's triangles in the reference's order and every triangle's nearest reference
 * triangle (the matches of :137-141 in front of the sort).  tri_capacity below n_triangles is an error. */
typedef struct nl_align_info {
    nl_align_triangle_t *triangles;
    float *tri_dist;
    int32_t *tri_ref;
    int32_t tri_capacity;
    int32_t n_picked, n_triangles;
    float scale_factor;              /* float32(ref_width) / float32(frame_width) (:78) */
    int32_t picked[NL_ALIGN_MAX_K];  /* pickBrightestDistant's indices (:76) */
} nl_align_info_t;
#ifdef __cplusplus
static_assert(sizeof(nl_align_triangle_t) == 24 && sizeof(nl_align_candidate_t) == 72, "alignment structs: 24, 72 bytes");
#else
_Static_assert(sizeof(nl_align_triangle_t) == 24 && sizeof(nl_align_candidate_t) == 72, "alignment structs: 24, 72 bytes");
#endif

/* NewAligner (:58-71): picks the k brightest distant reference stars (minLength = float32(ref_height) * (1.0f/20.0f),
 * as the reference takes naxisn[1]), builds their triangles at scale 1.0 and keeps stars and triangles on `device`.
 * ref_stars in FindStars' order (brightest first).  NULL on an error (nl_last_error()). */
nl_aligner_t *nl_aligner_create(int device, int ref_width, int ref_height, const nl_star_t *ref_stars, int n_ref_stars,
                                int k);
void nl_aligner_destroy(nl_aligner_t *a);
/* The picked indices (at most picked_capacity are written, *n_picked is the full count), the number of reference
 * triangles, and with tris_out the triangles themselves (tri_capacity below the count is an error).  Host only. */
int nl_aligner_info(const nl_aligner_t *a, int32_t *picked_out, int picked_capacity, int *n_picked, int *n_triangles,
                    nl_align_triangle_t *tris_out, int tri_capacity);
/* Align (:74-83) up to the minimiser, for the stars of one frame of frame_width columns: *n_cands <= min(k, triangles)
 * candidates in shortlist order at cands_out (cand_capacity below that is an error), and at ref_index_out, *n_cands rows
 * of n_stars int32 (room for min(cand_capacity, k) rows), per candidate and star the index into ref_stars of refPoints[id]
 * (:201), -1 for its NaN point (:204).  After create an aligner is immutable: safe to call from several host threads
 * at once on one aligner, each call with a stream and scratch of its own. */
int nl_aligner_match(nl_aligner_t *a, int frame_width, const nl_star_t *stars, int n_stars,
                     nl_align_candidate_t *cands_out, int cand_capacity, int *n_cands, int32_t *ref_index_out,
                     nl_align_info_t *info);
/* The matching alone (:194-206, and what calcDist :260-276 needs) for the caller's n_transforms <= NL_ALIGN_MAX_K
 * transforms of six floats each: ref_index_out n_transforms rows of n_stars, num_matches_out n_transforms counts. */
int nl_aligner_match_stars(nl_aligner_t *a, const float *transforms, int n_transforms, const nl_star_t *stars,
                           int n_stars, int32_t *ref_index_out, int32_t *num_matches_out);

#ifdef __cplusplus
}
#endif

#endif
