// align.hip -- OpAlign's estimate in front of the minimiser (internal/star/align.go).  Kernels:
//   align_triangles     generateTriangles (:108-130): one workgroup.  The m * m distances of the scaled picked stars,
//                       then per thread a run of consecutive (a, b) rows: count the c with dAB < dAC < dBC, exclusive
//                       scan over the threads, write -- the triangles come out in the order of the reference's loops
//   align_nearest_tri   closestTriangleMatches' kd-tree searches (:137-141) by brute force: a query triangle per lane,
//                       the reference triangles of the workgroup's chunk through LDS in tiles, a running (dsq, index)
//                       minimum; blockIdx.y splits the reference range so that the device is filled
//   align_combine_tri   the chunks' minima folded in chunk order: the lowest index wins a tie
//   align_match_stars   findBestMatch's matching (:194-206) for every candidate at once, grid = (block of stars,
//                       candidate): proj = trans.Apply(p), the nearest reference star by brute force through LDS, its
//                       index where dsq < 64, else -1; the matches counted by wave ballot and one integer atomic
// Every distance is the reference's fp32 expression, unfused and left to right (coord.go:85-88, :105-108, :141-145;
// the library is built with -ffp-contract=off), compared with <, so a NaN never replaces the minimum and never matches.
#include "align.hpp"

#include "launch_common.hpp"

namespace nl {

namespace {

constexpr int kTriThreads = 1024;

// Dist2D (coord.go:79-88)
__device__ __forceinline__ float dist2d(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    const float dsq = dx * dx + dy * dy;
    return (float)sqrt((double)dsq);
}

// the c of row (ia, ib) that make a triangle, in order: f(ic, dAC, dBC)
template <class F>
__device__ __forceinline__ void for_row_triangles(const float *dist, int m, int row, F f)
{
    const int ia = row / m, ib = row - ia * m;
    if (ia == ib) return;
    const float dab = dist[row];
    for (int ic = 0; ic < m; ic++) {
        if (ic == ia || ic == ib) continue;
        const float dac = dist[ia * m + ic], dbc = dist[ib * m + ic];
        if (dab < dac && dac < dbc) f(ic, dac, dbc);
    }
}

__global__ __launch_bounds__(kTriThreads) void align_triangles(const float2 *__restrict__ xy,
                                                               const int32_t *__restrict__ picked, int m, float scale,
                                                               float *__restrict__ dist, int64_t capacity,
                                                               nl_align_triangle_t *__restrict__ tris,
                                                               int32_t *__restrict__ count)
{
    __shared__ float sx[NL_ALIGN_MAX_K], sy[NL_ALIGN_MAX_K];
    __shared__ int s_scan[kTriThreads];
    const int tid = (int)threadIdx.x;
    if (tid < m) {                                             // :115: Point2D{star.X*scaleFactor, star.Y*scaleFactor}
        const float2 p = xy[picked[tid]];
        sx[tid] = p.x * scale;
        sy[tid] = p.y * scale;
    }
    __syncthreads();
    const int rows = m * m;
    for (int i = tid; i < rows; i += kTriThreads) {
        const int ia = i / m, ib = i - ia * m;
        dist[i] = dist2d(sx[ia], sy[ia], sx[ib], sy[ib]);
    }
    __syncthreads();                                           // (the workgroup's own global writes are visible behind it)

    const int per = (rows + kTriThreads - 1) / kTriThreads;
    const int row0 = min(tid * per, rows), row1 = min(row0 + per, rows);
    int n = 0;
    for (int row = row0; row < row1; row++) for_row_triangles(dist, m, row, [&](int, float, float) { n++; });

    s_scan[tid] = n;                                           // inclusive scan over the threads (Hillis-Steele)
    __syncthreads();
    for (int step = 1; step < kTriThreads; step <<= 1) {
        const int add = tid >= step ? s_scan[tid - step] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    int64_t at = s_scan[tid] - n;
    if (tid == kTriThreads - 1) *count = s_scan[tid];

    for (int row = row0; row < row1; row++) {
        const int ia = row / m, ib = row - ia * m;
        for_row_triangles(dist, m, row, [&](int ic, float dac, float dbc) {
            if (at < capacity) tris[at] = nl_align_triangle_t{dist[row], dac, dbc, picked[ia], picked[ib], picked[ic]};
            at++;
        });
    }
}

// (dsq, index) minimum of one query over the reference chunk blockIdx.y, at part[chunk * max_queries + query]
__global__ __launch_bounds__(kAlignBlock) void align_nearest_tri(const nl_align_triangle_t *__restrict__ queries,
                                                                 const int32_t *__restrict__ n_queries_dev,
                                                                 int64_t max_queries,
                                                                 const nl_align_triangle_t *__restrict__ refs,
                                                                 int n_refs, int tiles_per_chunk,
                                                                 float2 *__restrict__ part)
{
    __shared__ float4 tile[kAlignTriTile];
    const int n_queries = min((int64_t)*n_queries_dev, max_queries);
    const int q0 = (int)blockIdx.x * kAlignBlock;
    if (q0 >= n_queries) return;                               // (the whole workgroup: in front of every barrier)
    const int q = q0 + (int)threadIdx.x;
    const bool live = q < n_queries;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) {
        const nl_align_triangle_t t = queries[q];
        px = t.d_ab; py = t.d_ac; pz = t.d_bc;
    }
    const int chunk0 = (int)blockIdx.y * tiles_per_chunk * kAlignTriTile;
    const int chunk1 = min(chunk0 + tiles_per_chunk * kAlignTriTile, n_refs);
    float best = INFINITY;
    int best_i = chunk0;
    for (int t0 = chunk0; t0 < chunk1; t0 += kAlignTriTile) {
        const int cnt = min(kAlignTriTile, chunk1 - t0);
        __syncthreads();
        for (int i = (int)threadIdx.x; i < cnt; i += kAlignBlock) {
            const nl_align_triangle_t r = refs[t0 + i];
            tile[i] = make_float4(r.d_ab, r.d_ac, r.d_bc, 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < cnt; i++) {                        // Dist3DSquared (coord.go:105-108)
            const float4 r = tile[i];
            const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
            const float dsq = dx * dx + dy * dy + dz * dz;
            if (dsq < best) { best = dsq; best_i = t0 + i; }
        }
    }
    if (live) part[(int64_t)blockIdx.y * max_queries + q] = make_float2(best, __int_as_float(best_i));
}

__global__ __launch_bounds__(kAlignBlock) void align_combine_tri(const float2 *__restrict__ part,
                                                                 const int32_t *__restrict__ n_queries_dev,
                                                                 int64_t max_queries, int chunks,
                                                                 float *__restrict__ dist, int32_t *__restrict__ ref)
{
    const int n_queries = min((int64_t)*n_queries_dev, max_queries);
    const int q = (int)(blockIdx.x * kAlignBlock + threadIdx.x);
    if (q >= n_queries) return;
    float2 best = part[q];
    for (int c = 1; c < chunks; c++) {                         // ascending indices: < keeps the lowest at a tie
        const float2 p = part[(int64_t)c * max_queries + q];
        if (p.x < best.x) best = p;
    }
    dist[q] = best.x;
    ref[q] = __float_as_int(best.y);
}

__global__ __launch_bounds__(kAlignBlock) void align_match_stars(const float *__restrict__ trans,
                                                                 const float2 *__restrict__ xy, int n_stars,
                                                                 const float2 *__restrict__ ref_xy, int n_refs,
                                                                 int32_t *__restrict__ ref_index,
                                                                 int32_t *__restrict__ counts)
{
    __shared__ float2 tile[kAlignStarTile];
    const int cand = (int)blockIdx.y;
    const int s = (int)(blockIdx.x * kAlignBlock + threadIdx.x);
    const bool live = s < n_stars;
    const float *t = trans + 6 * cand;
    const float ta = t[0], tb = t[1], tc = t[2], td = t[3], te = t[4], tf = t[5];
    float px = 0.0f, py = 0.0f;
    if (live) {                                                // Transform2D.Apply (coord.go:141-145)
        const float2 p = xy[s];
        px = ta * p.x + tb * p.y + tc;
        py = td * p.x + te * p.y + tf;
    }
    float best = INFINITY;
    int best_i = 0;
    for (int t0 = 0; t0 < n_refs; t0 += kAlignStarTile) {
        const int cnt = min(kAlignStarTile, n_refs - t0);
        __syncthreads();
        for (int i = (int)threadIdx.x; i < cnt; i += kAlignBlock) tile[i] = ref_xy[t0 + i];
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < cnt; i++) {                        // Dist2DSquared (coord.go:85-88)
            const float2 r = tile[i];
            const float dx = px - r.x, dy = py - r.y;
            const float dsq = dx * dx + dy * dy;
            if (dsq < best) { best = dsq; best_i = t0 + i; }
        }
    }
    const bool matched = live && best < 64.0f;                 // :164, :200: distSquared < 8*8
    if (live) ref_index[(int64_t)cand * n_stars + s] = matched ? best_i : -1;
    const unsigned long long votes = __ballot(matched);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&counts[cand], __popcll(votes));
}

}  // namespace

int align_tri_chunks(int64_t n_queries, int64_t n_refs, int *tiles_per_chunk)
{
    const int64_t tiles = (n_refs + kAlignTriTile - 1) / kAlignTriTile;
    const int64_t blocks = (n_queries + kAlignBlock - 1) / kAlignBlock;
    int64_t want = blocks > 0 ? (1024 + blocks - 1) / blocks : 1;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const int64_t per = tiles > 0 ? (tiles + want - 1) / want : 1;
    if (tiles_per_chunk) *tiles_per_chunk = (int)per;
    return tiles > 0 ? (int)((tiles + per - 1) / per) : 1;
}

hipError_t align_triangles_launch(const float2 *d_xy, const int32_t *d_picked, int m, float scale, float *d_dist,
                            nl_align_triangle_t *d_tris, int32_t *d_count, hipStream_t stream)
{
    Launcher L(stream);
    L(align_triangles, dim3(1), kTriThreads, 0, d_xy, d_picked, m, scale, d_dist, align_max_triangles(m), d_tris, d_count);
    return L.err;
}

hipError_t align_nearest_tri_launch(const nl_align_triangle_t *d_queries, const int32_t *d_n_queries, int64_t max_queries,
                              const nl_align_triangle_t *d_refs, int64_t n_refs, float2 *d_part, float *d_dist,
                              int32_t *d_ref, hipStream_t stream)
{
    int per = 1;
    const int chunks = align_tri_chunks(max_queries, n_refs, &per);
    const unsigned blocks = (unsigned)((max_queries + kAlignBlock - 1) / kAlignBlock);
    Launcher L(stream);
    L(align_nearest_tri, dim3(blocks, (unsigned)chunks), kAlignBlock, 0, d_queries, d_n_queries, max_queries, d_refs,
      (int)n_refs, per, d_part);
    L(align_combine_tri, dim3(blocks), kAlignBlock, 0, d_part, d_n_queries, max_queries, chunks, d_dist, d_ref);
    return L.err;
}

hipError_t align_match_stars_launch(const float *d_trans, int n_trans, const float2 *d_xy, int n_stars, const float2 *d_ref_xy,
                              int n_refs, int32_t *d_ref_index, int32_t *d_counts, hipStream_t stream)
{
    Launcher L(stream);
    L.keep(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)n_trans, stream));
    const unsigned blocks = (unsigned)((n_stars + kAlignBlock - 1) / kAlignBlock);
    L(align_match_stars, dim3(blocks, (unsigned)n_trans), kAlignBlock, 0, d_trans, d_xy, n_stars, d_ref_xy, n_refs,
      d_ref_index, d_counts);
    return L.err;
}

}  // namespace nl
