// align.hpp -- OpAlign's estimate in front of the minimiser (star.Aligner, internal/star/align.go:58-206) for the C ABI
// in nlstack_align.hip: the triangles of the picked stars, every triangle's nearest reference triangle, and per
// candidate transform every star's nearest reference star.  The kd-trees of the reference are exact nearest-neighbour
// searches; the kernels search by brute force and return the same fp32 minimum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

constexpr int kAlignTriTile = 512;       // reference triangles per LDS tile of align_nearest_tri (float4 each: 8 KiB)
constexpr int kAlignStarTile = 1024;     // reference stars per LDS tile of align_match_stars (float2 each: 8 KiB)
constexpr int kAlignBlock = 256;         // threads per workgroup of both searches: one query per thread

// the most triangles m picked stars give: of the six orders of three stars at most one has dAB < dAC < dBC
inline int64_t align_max_triangles(int m) { return m < 3 ? 0 : (int64_t)m * (m - 1) * (m - 2) / 6; }

// workgroups along y of align_nearest_tri for n_queries (an upper bound) against n_refs: the reference range is split
// so that about a thousand workgroups run, each over whole tiles
int align_tri_chunks(int64_t n_queries, int64_t n_refs, int *tiles_per_chunk);

// generateTriangles (:108-130) over the m <= NL_ALIGN_MAX_K stars d_picked of d_xy, coordinates times scale: the
// triangles in the order of the reference's loops at d_tris (room for align_max_triangles(m)), their number at
// *d_count.  d_dist: m * m floats of scratch.  One workgroup.
hipError_t align_triangles_launch(const float2 *d_xy, const int32_t *d_picked, int m, float scale, float *d_dist,
                            nl_align_triangle_t *d_tris, int32_t *d_count, hipStream_t stream);

// closestTriangleMatches' searches (:137-141): for each of the *d_n_queries <= max_queries triangles at d_queries the
// smallest dsq to the n_refs > 0 triangles at d_refs and the lowest index that has it, at d_dist / d_ref.
// d_part: 2 * chunks * max_queries words of scratch (chunks = align_tri_chunks(max_queries, n_refs)).
hipError_t align_nearest_tri_launch(const nl_align_triangle_t *d_queries, const int32_t *d_n_queries, int64_t max_queries,
                              const nl_align_triangle_t *d_refs, int64_t n_refs, float2 *d_part, float *d_dist,
                              int32_t *d_ref, hipStream_t stream);

// findBestMatch's matching (:194-206) for n_trans transforms at d_trans (six floats each) at once: per transform and
// star the index of the nearest of the n_refs > 0 reference stars where dsq < 64, else -1, at d_ref_index
// [n_trans][n_stars]; the matches counted at d_counts[n_trans], which the launch zeroes first.
hipError_t align_match_stars_launch(const float *d_trans, int n_trans, const float2 *d_xy, int n_stars, const float2 *d_ref_xy,
                              int n_refs, int32_t *d_ref_index, int32_t *d_counts, hipStream_t stream);

}  // namespace nl
