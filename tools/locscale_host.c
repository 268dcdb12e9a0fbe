/* locscale_host.c -- a single-threaded C restatement of LSESCMedianQn (internal/stats/stats.go:336-364, :436-499)
 * with the caller's seeds, for tools/locscale_probe.py: what the host would spend on the estimate after downloading
 * the frame.  A measurement aid, compiled by the probe (cc -O2 -ffp-contract=off -shared); the probe checks its result
 * against the device's bits.  No draw budget: the probe's frame is far inside it. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static uint32_t next(uint32_t *x)
{
    *x ^= *x << 13;
    *x ^= *x >> 17;
    *x ^= *x << 5;
    return *x;
}
static uint32_t below(uint32_t *x, uint32_t m) { return (uint32_t)(((uint64_t)next(x) * (uint64_t)m) >> 32); }

/* QSelectFloat32 (qsort.go:94-126), NaN-free input */
static float qselect(float *a, int n, int k)
{
    int left = 0, right = n - 1;
    while (left < right) {
        const float pivot = a[(left + right) >> 1];
        int l = left - 1, r = right + 1;
        for (;;) {
            do l++; while (a[l] < pivot);
            do r--; while (a[r] > pivot);
            if (l >= r) break;
            const float t = a[l]; a[l] = a[r]; a[r] = t;
        }
        const int offset = r - left + 1;
        if (k <= offset) right = r;
        else { left = r + 1; k -= offset; }
    }
    return a[left];
}
static float qselect_median(float *a, int n)
{
    const int k = (n >> 1) + 1;
    const float upper = qselect(a, n, k);
    if (n & 1) return upper;
    float lower = a[0];
    for (int i = 1; i < k - 1; i++)
        if (a[i] > lower) lower = a[i];
    return 0.5f * (lower + upper);
}

static float median(const float *d, uint32_t p, float *s, int n, uint32_t x)
{
    for (int i = 0; i < n; i++) s[i] = d[below(&x, p)];
    return qselect_median(s, n);
}
static float qn(const float *d, uint32_t p, float *s, int n, uint32_t x)
{
    for (int i = 0; i < n; i++) {
        const uint32_t i1 = 1 + below(&x, p - 1), i2 = below(&x, i1);
        s[i] = fabsf(d[i1] - d[i2]);
    }
    return qselect(s, n, (n >> 2) + 1) * 2.21914f;
}
static float bounded_median(const float *d, uint32_t p, float lo, float hi, float *s, int n, uint32_t x)
{
    for (int i = 0; i < n; i++) {
        float v;
        do v = d[below(&x, p)]; while (!(v >= lo && v <= hi));
        s[i] = v;
    }
    return qselect_median(s, n);
}
static float bounded_qn(const float *d, uint32_t p, float lo, float hi, float *s, int n, uint32_t x)
{
    for (int i = 0; i < n; i++) {
        float d1, d2;
        for (;;) {
            const uint32_t i1 = 1 + below(&x, p - 1);
            d1 = d[i1];
            if (d1 < lo || d1 > hi) continue;
            d2 = d[below(&x, i1)];
            if (d2 >= lo && d2 <= hi) break;
        }
        s[i] = fabsf(d1 - d2);
    }
    return qselect(s, n, (n >> 2) + 1) * 2.21914f;
}

/* FastApproxSigmaClippedMedianAndQn(data, 2, 2, epsilon, n) with seeds[0 .. 24]; returns the iterations */
int locscale_host(const float *d, uint32_t pixels, int n, const uint32_t *seeds, float epsilon, float *location,
                  float *scale)
{
    float *s = malloc(sizeof(float) * (size_t)n);
    int call = 0;
    float loc = median(d, pixels, s, n, seeds[call++]);
    float sc = qn(d, pixels, s, n, seeds[call++]);
    for (int i = 0;; i++) {
        const float lo = loc - 2.0f * sc, hi = loc + 2.0f * sc;
        const float new_loc = bounded_median(d, pixels, lo, hi, s, n, seeds[call++]);
        float new_sc = bounded_qn(d, pixels, lo, hi, s, n, seeds[call++]);
        new_sc = new_sc * 1.134f;
        if ((float)(fabs((double)(new_loc - loc)) + fabs((double)(new_sc - sc))) <= epsilon || i >= 10) {
            *location = loc;
            *scale = qn(d, pixels, s, n, seeds[call++]);
            free(s);
            return i + 1;
        }
        loc = new_loc;
        sc = new_sc;
    }
}
