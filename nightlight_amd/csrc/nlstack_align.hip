// nlstack_align.hip -- the alignment entries of the C ABI (include/nlstack_align.h): star.Aligner up to the minimiser
// (internal/star/align.go:58-206).  The sequential parts run here on the host, literally -- pickBrightestDistant
// (:86-104), the shortlist (:143-155), NewTransform2D (coord.go:118-137); the kernels are in align.hip.
#include <math.h>

#include <algorithm>
#include <memory>
#include <mutex>

#include "align.hpp"
#include "nlstack_frame_common.hpp"

// One call's stream and device scratch.  An aligner parks them between calls; concurrent calls each take their own.
struct AlignWork {
    hipStream_t stream = nullptr;
    nl::DevBuffer buf;
    ~AlignWork()
    {
        buf.release();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct nl_aligner {
    int device = 0, ref_width = 0, ref_height = 0, k = 0;
    std::vector<nl_star_t> ref_stars;
    std::vector<int32_t> picked;
    std::vector<nl_align_triangle_t> tris;                     // the reference triangles, as on the device
    void *d_block = nullptr;                                   // d_ref_xy and d_tris
    float2 *d_ref_xy = nullptr;
    nl_align_triangle_t *d_tris = nullptr;
    std::mutex mu;                                             // guards parked
    std::vector<std::unique_ptr<AlignWork>> parked;
};

namespace {

// Dist2D (coord.go:79-88)
float dist2d(float ax, float ay, float bx, float by)
{
    const float dx = ax - bx, dy = ay - by;
    const float dsq = dx * dx + dy * dy;
    return (float)sqrt((double)dsq);
}

// pickBrightestDistant (:86-104)
std::vector<int32_t> pick_brightest_distant(const nl_star_t *stars, int n_stars, float min_length, int k)
{
    std::vector<int32_t> indices;
    for (int s = 0; (int)indices.size() < k && s < n_stars; s++) {
        bool far = true;
        for (size_t j = 0; j < indices.size() && far; j++) {
            const nl_star_t &b = stars[indices[j]];
            if (dist2d(stars[s].x, stars[s].y, b.x, b.y) < min_length) far = false;
        }
        if (far) indices.push_back(s);
    }
    return indices;
}

// NewTransform2D (coord.go:118-137); false: "divide by zero"
bool new_transform_2d(const nl_star_t &p1, const nl_star_t &p2, const nl_star_t &p3, const nl_star_t &p1p,
                      const nl_star_t &p2p, const nl_star_t &p3p, float t[6])
{
    const float den = (p2.y - p1.y) * (p3.x - p1.x) - (p2.x - p1.x) * (p3.y - p1.y);
    const float a = ((p3p.x - p1p.x) * (p2.y - p1.y) - (p2p.x - p1p.x) * (p3.y - p1.y)) / den;
    const float b = ((p2p.x - p1p.x) - a * (p2.x - p1.x)) / (p2.y - p1.y);
    const float c = p1p.x - a * p1.x - b * p1.y;
    const float d = ((p3p.y - p1p.y) * (p2.y - p1.y) - (p2p.y - p1p.y) * (p3.y - p1.y)) / den;
    const float e = ((p2p.y - p1p.y) - d * (p2.x - p1.x)) / (p2.y - p1.y);
    const float f = p1p.y - d * p1.x - e * p1.y;
    if (isinf(a) || isinf(b) || isinf(d) || isinf(e)) return false;
    t[0] = a; t[1] = b; t[2] = c; t[3] = d; t[4] = e; t[5] = f;
    return true;
}

int take_work(nl_aligner *a, std::unique_ptr<AlignWork> *w)
{
    {
        std::lock_guard<std::mutex> lk(a->mu);
        if (!a->parked.empty()) {
            *w = std::move(a->parked.back());
            a->parked.pop_back();
            return NL_OK;
        }
    }
    w->reset(new AlignWork);
    NL_HIP(hipStreamCreateWithFlags(&(*w)->stream, hipStreamNonBlocking));
    return NL_OK;
}

void park_work(nl_aligner *a, std::unique_ptr<AlignWork> w)
{
    std::lock_guard<std::mutex> lk(a->mu);
    a->parked.push_back(std::move(w));
}

std::vector<float2> star_xy(const nl_star_t *stars, int n)
{
    std::vector<float2> xy((size_t)n);
    for (int i = 0; i < n; i++) xy[(size_t)i] = make_float2(stars[i].x, stars[i].y);
    return xy;
}

// the device arrays of one match call, carved from the call's scratch
struct MatchArrays {
    float2 *xy, *part;
    int32_t *picked, *count, *tri_ref, *ref_index, *counts;
    float *dist, *tri_dist, *trans;
    nl_align_triangle_t *tris;
    size_t bytes;
    MatchArrays(void *base, int n_stars, int m, int64_t max_tris, int chunks, int rows)
    {
        nl::Carver c(base);
        xy = c.take<float2>((size_t)n_stars);
        picked = c.take<int32_t>(NL_ALIGN_MAX_K);
        count = c.take<int32_t>(1);
        dist = c.take<float>((size_t)m * (size_t)m);
        tris = c.take<nl_align_triangle_t>((size_t)max_tris);
        part = c.take<float2>((size_t)chunks * (size_t)max_tris);
        tri_dist = c.take<float>((size_t)max_tris);
        tri_ref = c.take<int32_t>((size_t)max_tris);
        trans = c.take<float>(6 * (size_t)rows);
        counts = c.take<int32_t>((size_t)rows);
        ref_index = c.take<int32_t>((size_t)rows * (size_t)n_stars);
        bytes = c.bytes();
    }
};

// stage 3 for `rows` transforms on w's stream: ref_index and counts down into the caller's arrays
int match_stars_run(nl_aligner *a, AlignWork &w, const MatchArrays &d, const float *trans, int rows, int n_stars,
                    int32_t *ref_index_out, int32_t *counts_out)
{
    NL_HIP(hipMemcpyAsync(d.trans, trans, sizeof(float) * 6 * (size_t)rows, hipMemcpyHostToDevice, w.stream));
    NL_HIP(nl::align_match_stars_launch(d.trans, rows, d.xy, n_stars, a->d_ref_xy, (int)a->ref_stars.size(), d.ref_index,
                                 d.counts, w.stream));
    NL_HIP(hipMemcpyAsync(ref_index_out, d.ref_index, sizeof(int32_t) * (size_t)rows * (size_t)n_stars,
                          hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipMemcpyAsync(counts_out, d.counts, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipStreamSynchronize(w.stream));
    return NL_OK;
}

int aligner_match_impl(nl_aligner *a, AlignWork &w, int frame_width, const nl_star_t *stars, int n_stars,
                       nl_align_candidate_t *cands_out, int cand_capacity, int *n_cands, int32_t *ref_index_out,
                       nl_align_info_t *info)
{
    const float min_length = (float)a->ref_height * (1.0f / 20.0f);                  // :75
    const float scale = (float)a->ref_width / (float)frame_width;                    // :78
    const std::vector<int32_t> picked = pick_brightest_distant(stars, n_stars, min_length, a->k);
    const int m = (int)picked.size();
    const int64_t max_tris = nl::align_max_triangles(m), n_refs = (int64_t)a->tris.size();
    const int chunks = nl::align_tri_chunks(max_tris, n_refs, nullptr);
    const int rows = std::min(a->k, cand_capacity);
    const MatchArrays need(nullptr, n_stars, m, max_tris, chunks, rows);
    NL_HIP(w.buf.reserve(need.bytes, w.stream));
    const MatchArrays d(w.buf.ptr, n_stars, m, max_tris, chunks, rows);

    if (info) {
        info->n_picked = m;
        info->n_triangles = 0;
        info->scale_factor = scale;
        memset(info->picked, 0, sizeof info->picked);
        std::copy(picked.begin(), picked.end(), info->picked);
    }
    *n_cands = 0;
    if (max_tris == 0) return NL_OK;

    // stages 1 and 2: the triangles, every triangle's nearest reference triangle
    const std::vector<float2> xy = star_xy(stars, n_stars);
    NL_HIP(hipMemcpyAsync(d.xy, xy.data(), sizeof(float2) * xy.size(), hipMemcpyHostToDevice, w.stream));
    NL_HIP(hipMemcpyAsync(d.picked, picked.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, w.stream));
    NL_HIP(nl::align_triangles_launch(d.xy, d.picked, m, scale, d.dist, d.tris, d.count, w.stream));
    if (n_refs > 0) {
        NL_HIP(nl::align_nearest_tri_launch(d.tris, d.count, max_tris, a->d_tris, n_refs, d.part, d.tri_dist, d.tri_ref,
                                     w.stream));
    }
    int32_t n_tris = 0;
    NL_HIP(hipMemcpyAsync(&n_tris, d.count, sizeof n_tris, hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipStreamSynchronize(w.stream));
    if (n_tris < 0 || n_tris > max_tris) return fail(NL_ERR_HIP, "aligner_match: %d triangles of at most %lld", n_tris, (long long)max_tris);
    if (info) info->n_triangles = n_tris;
    if (n_tris == 0) return NL_OK;
    if (n_refs == 0)
        return fail(NL_ERR_INVALID_ARG, "aligner_match: %d triangles against a reference with none (the reference indexes an empty tree, kdtree3p.go:82)", n_tris);
    if (info && (info->triangles || info->tri_dist || info->tri_ref) && info->tri_capacity < n_tris)
        return fail(NL_ERR_INVALID_ARG, "aligner_match: %d triangles, info has room for %d", n_tris, info->tri_capacity);
    const int n_short = std::min(a->k, (int)n_tris);                                 // :148-149
    if (cand_capacity < n_short)
        return fail(NL_ERR_INVALID_ARG, "aligner_match: %d candidates, room for %d", n_short, cand_capacity);

    std::vector<nl_align_triangle_t> tris((size_t)n_tris);
    std::vector<float> tri_dist((size_t)n_tris);
    std::vector<int32_t> tri_ref((size_t)n_tris);
    NL_HIP(hipMemcpyAsync(tris.data(), d.tris, sizeof(nl_align_triangle_t) * tris.size(), hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipMemcpyAsync(tri_dist.data(), d.tri_dist, sizeof(float) * tri_dist.size(), hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipMemcpyAsync(tri_ref.data(), d.tri_ref, sizeof(int32_t) * tri_ref.size(), hipMemcpyDeviceToHost, w.stream));
    NL_HIP(hipStreamSynchronize(w.stream));
    if (info && info->triangles) memcpy(info->triangles, tris.data(), sizeof(nl_align_triangle_t) * tris.size());
    if (info && info->tri_dist) memcpy(info->tri_dist, tri_dist.data(), sizeof(float) * tri_dist.size());
    if (info && info->tri_ref) memcpy(info->tri_ref, tri_ref.data(), sizeof(int32_t) * tri_ref.size());

    // the shortlist (:143-155): the n_short smallest by (dist, tri index); a NaN distance sorts last
    std::vector<int32_t> order((size_t)n_tris);
    for (int32_t i = 0; i < n_tris; i++) order[(size_t)i] = i;
    const auto key = [&](int32_t i) { const float v = tri_dist[(size_t)i]; return v != v ? INFINITY : v; };
    std::partial_sort(order.begin(), order.begin() + n_short, order.end(), [&](int32_t i, int32_t j) {
        const float di = key(i), dj = key(j);
        return di < dj || (di == dj && i < j);
    });

    // the candidates' transforms (:169-178); a skipped candidate goes to the device as NaN, which matches nothing
    std::vector<float> trans(6 * (size_t)n_short);
    for (int c = 0; c < n_short; c++) {
        nl_align_candidate_t &out = cands_out[c];
        memset(&out, 0, sizeof out);
        const int32_t ti = order[(size_t)c];
        const nl_align_triangle_t &tri = tris[(size_t)ti], &ref = a->tris[(size_t)tri_ref[(size_t)ti]];
        out.dist = tri_dist[(size_t)ti];
        out.tri_index = ti;
        out.ref_tri_index = tri_ref[(size_t)ti];
        out.a = tri.a; out.b = tri.b; out.c = tri.c;
        out.ref_a = ref.a; out.ref_b = ref.b; out.ref_c = ref.c;
        out.trans_ok = new_transform_2d(stars[tri.a], stars[tri.b], stars[tri.c], a->ref_stars[(size_t)ref.a],
                                        a->ref_stars[(size_t)ref.b], a->ref_stars[(size_t)ref.c], out.trans) ? 1 : 0;
        for (int i = 0; i < 6; i++) trans[6 * (size_t)c + (size_t)i] = out.trans_ok ? out.trans[i] : NAN;
    }

    // stage 3: every star's nearest reference star, per candidate
    std::vector<int32_t> counts((size_t)n_short);
    const int rc = match_stars_run(a, w, d, trans.data(), n_short, n_stars, ref_index_out, counts.data());
    if (rc != NL_OK) return rc;
    for (int c = 0; c < n_short; c++) {
        cands_out[c].num_matches = counts[(size_t)c];
        cands_out[c].enough = cands_out[c].trans_ok && counts[(size_t)c] >= n_stars / 3;   // :210
    }
    *n_cands = n_short;
    return NL_OK;
}

int create_check(int ref_width, int ref_height, const nl_star_t *ref_stars, int n_ref_stars, int k)
{
    if (!ref_stars) return fail(NL_ERR_INVALID_ARG, "aligner_create: null reference stars");
    if (k <= 0 || k > NL_ALIGN_MAX_K) return fail(NL_ERR_INVALID_ARG, "aligner_create: k %d (1 .. %d)", k, NL_ALIGN_MAX_K);
    if (n_ref_stars <= 0)
        return fail(NL_ERR_INVALID_ARG, "aligner_create: Unable to align without star detections in reference frame (postprocess.go:203)");
    if (ref_width <= 0 || ref_height <= 0)
        return fail(NL_ERR_INVALID_ARG, "aligner_create: reference frame of %d x %d", ref_width, ref_height);
    return NL_OK;
}

int create_impl(nl_aligner *a)
{
    const int n = (int)a->ref_stars.size(), m = (int)a->picked.size();
    const int64_t max_tris = nl::align_max_triangles(m);
    nl::Carver measure(nullptr);
    measure.take<float2>((size_t)n);
    measure.take<nl_align_triangle_t>((size_t)max_tris);
    NL_HIP(dev_malloc(&a->d_block, std::max(measure.bytes(), (size_t)256)));
    nl::Carver c(a->d_block);
    a->d_ref_xy = c.take<float2>((size_t)n);
    a->d_tris = c.take<nl_align_triangle_t>((size_t)max_tris);
    if (max_tris == 0) {
        const std::vector<float2> xy = star_xy(a->ref_stars.data(), n);
        NL_HIP(hipMemcpy(a->d_ref_xy, xy.data(), sizeof(float2) * xy.size(), hipMemcpyHostToDevice));
        return NL_OK;
    }
    // generateTriangles at scale 1.0 (:65) on a scratch of the call's own
    std::unique_ptr<AlignWork> w;
    int rc = take_work(a, &w);
    if (rc != NL_OK) return rc;
    nl::Carver s_measure(nullptr);
    s_measure.take<int32_t>(NL_ALIGN_MAX_K);
    s_measure.take<int32_t>(1);
    s_measure.take<float>((size_t)m * (size_t)m);
    NL_HIP(w->buf.reserve(s_measure.bytes(), w->stream));
    nl::Carver s(w->buf.ptr);
    int32_t *d_picked = s.take<int32_t>(NL_ALIGN_MAX_K), *d_count = s.take<int32_t>(1);
    float *d_dist = s.take<float>((size_t)m * (size_t)m);
    const std::vector<float2> xy = star_xy(a->ref_stars.data(), n);
    NL_HIP(hipMemcpyAsync(a->d_ref_xy, xy.data(), sizeof(float2) * xy.size(), hipMemcpyHostToDevice, w->stream));
    NL_HIP(hipMemcpyAsync(d_picked, a->picked.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, w->stream));
    NL_HIP(nl::align_triangles_launch(a->d_ref_xy, d_picked, m, 1.0f, d_dist, a->d_tris, d_count, w->stream));
    int32_t n_tris = 0;
    NL_HIP(hipMemcpyAsync(&n_tris, d_count, sizeof n_tris, hipMemcpyDeviceToHost, w->stream));
    NL_HIP(hipStreamSynchronize(w->stream));
    if (n_tris < 0 || n_tris > max_tris) return fail(NL_ERR_HIP, "aligner_create: %d triangles of at most %lld", n_tris, (long long)max_tris);
    a->tris.resize((size_t)n_tris);
    NL_HIP(hipMemcpy(a->tris.data(), a->d_tris, sizeof(nl_align_triangle_t) * a->tris.size(), hipMemcpyDeviceToHost));
    park_work(a, std::move(w));
    return NL_OK;
}

// what nl_aligner_match and nl_aligner_match_stars share, in front of the device
int stars_check(const char *who, const nl_aligner *a, const nl_star_t *stars, int n_stars)
{
    if (!a) return fail(NL_ERR_INVALID_ARG, "%s: null aligner", who);
    if (!stars) return fail(NL_ERR_INVALID_ARG, "%s: null stars", who);
    if (n_stars <= 0) return fail(NL_ERR_INVALID_ARG, "%s: %d stars", who, n_stars);
    return NL_OK;
}

}  // namespace

extern "C" {

nl_aligner_t *nl_aligner_create(int device, int ref_width, int ref_height, const nl_star_t *ref_stars, int n_ref_stars,
                                int k)
{
    if (create_check(ref_width, ref_height, ref_stars, n_ref_stars, k) != NL_OK) return nullptr;
    if (select_device(device) != NL_OK) return nullptr;
    nl_aligner *a = new nl_aligner;
    a->device = device;
    a->ref_width = ref_width;
    a->ref_height = ref_height;
    a->k = k;
    a->ref_stars.assign(ref_stars, ref_stars + n_ref_stars);
    a->picked = pick_brightest_distant(ref_stars, n_ref_stars, (float)ref_height * (1.0f / 20.0f), k);   // :63-64
    if (create_impl(a) != NL_OK) {
        const std::string keep = g_err;
        nl_aligner_destroy(a);
        g_err = keep;
        return nullptr;
    }
    return a;
}

void nl_aligner_destroy(nl_aligner_t *a)
{
    if (!a) return;
    (void)hipSetDevice(a->device);
    a->parked.clear();
    if (a->d_block) (void)hipFree(a->d_block);
    delete a;
}

int nl_aligner_info(const nl_aligner_t *a, int32_t *picked_out, int picked_capacity, int *n_picked, int *n_triangles,
                    nl_align_triangle_t *tris_out, int tri_capacity)
{
    if (!a) return fail(NL_ERR_INVALID_ARG, "aligner_info: null aligner");
    int rc = check_capacity("aligner_info (picked)", picked_capacity, picked_out);
    if (rc == NL_OK) rc = check_capacity("aligner_info (triangles)", tri_capacity, tris_out);
    if (rc != NL_OK) return rc;
    if (tris_out && (size_t)tri_capacity < a->tris.size())
        return fail(NL_ERR_INVALID_ARG, "aligner_info: %zu triangles, room for %d", a->tris.size(), tri_capacity);
    if (n_picked) *n_picked = (int)a->picked.size();
    if (n_triangles) *n_triangles = (int)a->tris.size();
    for (size_t i = 0; i < a->picked.size() && (int)i < picked_capacity; i++) picked_out[i] = a->picked[i];
    if (tris_out && !a->tris.empty()) memcpy(tris_out, a->tris.data(), sizeof(nl_align_triangle_t) * a->tris.size());
    return NL_OK;
}

int nl_aligner_match(nl_aligner_t *a, int frame_width, const nl_star_t *stars, int n_stars,
                     nl_align_candidate_t *cands_out, int cand_capacity, int *n_cands, int32_t *ref_index_out,
                     nl_align_info_t *info)
{
    int rc = stars_check("aligner_match", a, stars, n_stars);
    if (rc != NL_OK) return rc;
    if (!cands_out || !n_cands || !ref_index_out) return fail(NL_ERR_INVALID_ARG, "aligner_match: null output");
    if (frame_width <= 0) return fail(NL_ERR_INVALID_ARG, "aligner_match: frame width %d", frame_width);
    if (cand_capacity <= 0) return fail(NL_ERR_INVALID_ARG, "aligner_match: room for %d candidates", cand_capacity);
    if (info && info->tri_capacity < 0) return fail(NL_ERR_INVALID_ARG, "aligner_match: info has room for %d triangles", info->tri_capacity);
    if ((rc = nl::require_device()) != NL_OK || (rc = select_device(a->device)) != NL_OK) return rc;
    std::unique_ptr<AlignWork> w;
    if ((rc = take_work(a, &w)) != NL_OK) return rc;
    rc = aligner_match_impl(a, *w, frame_width, stars, n_stars, cands_out, cand_capacity, n_cands, ref_index_out, info);
    if (rc == NL_OK || rc == NL_ERR_INVALID_ARG) park_work(a, std::move(w));
    return rc;
}

int nl_aligner_match_stars(nl_aligner_t *a, const float *transforms, int n_transforms, const nl_star_t *stars,
                           int n_stars, int32_t *ref_index_out, int32_t *num_matches_out)
{
    int rc = stars_check("aligner_match_stars", a, stars, n_stars);
    if (rc != NL_OK) return rc;
    if (!transforms || !ref_index_out || !num_matches_out)
        return fail(NL_ERR_INVALID_ARG, "aligner_match_stars: null transforms or output");
    if (n_transforms <= 0 || n_transforms > NL_ALIGN_MAX_K)
        return fail(NL_ERR_INVALID_ARG, "aligner_match_stars: %d transforms (1 .. %d)", n_transforms, NL_ALIGN_MAX_K);
    if ((rc = nl::require_device()) != NL_OK || (rc = select_device(a->device)) != NL_OK) return rc;
    std::unique_ptr<AlignWork> w;
    if ((rc = take_work(a, &w)) != NL_OK) return rc;
    const auto run = [&]() -> int {
        const MatchArrays need(nullptr, n_stars, 0, 0, 1, n_transforms);
        NL_HIP(w->buf.reserve(need.bytes, w->stream));
        const MatchArrays d(w->buf.ptr, n_stars, 0, 0, 1, n_transforms);
        const std::vector<float2> xy = star_xy(stars, n_stars);
        NL_HIP(hipMemcpyAsync(d.xy, xy.data(), sizeof(float2) * xy.size(), hipMemcpyHostToDevice, w->stream));
        return match_stars_run(a, *w, d, transforms, n_transforms, n_stars, ref_index_out, num_matches_out);
    };
    rc = run();
    if (rc == NL_OK) park_work(a, std::move(w));
    return rc;
}

}  // extern "C"
