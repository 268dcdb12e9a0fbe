// goal_seek.hpp -- the goal-seek of FindSigmasAndStack (spec: internal/ops/stack/stackfindsigma.go:27-170), host
// arithmetic only: the two searches as state machines fed with the counters of one pass at a time, and the ONE driver
// that runs them.  Included by nlstack_pass.hip and nlstack_group.hip; no kernel unit sees it.
#pragma once
#include <stdint.h>

#include "../../include/nlstack.h"

namespace nl {

// Bisection of the goal-seek (spec: stackfindsigma.go:48-98): sigma_low and
// sigma_high in [1,11], percentages in the reference's fp32 arithmetic, 21 passes at most.
struct SigmaBisection {
    float low_left = 1.0f, low_right = 11.0f, low_mid;
    float high_left = 1.0f, high_right = 11.0f, high_mid;
    float perc_low, perc_high, total;
    int i = 0;
    SigmaBisection(float clip_perc_low, float clip_perc_high, int64_t total_samples)
        : perc_low(clip_perc_low), perc_high(clip_perc_high), total((float)total_samples)
    {
        low_mid = 0.5f * (low_left + low_right);
        high_mid = 0.5f * (high_left + high_right);
    }
    // counters of the pass run with (low_mid, high_mid); true = done, else the mids have moved
    bool step(int64_t clip_low, int64_t clip_high)
    {
        const float pl = (float)clip_low * 100.0f / total;
        const float ph = (float)clip_high * 100.0f / total;
        const int delta_l = (int)(100 * pl + 0.5f) - (int)(100 * perc_low);
        const int delta_h = (int)(100 * ph + 0.5f) - (int)(100 * perc_high);
        if ((delta_l == 0 && delta_h == 0) || i >= 20) return true;
        i++;
        if (delta_l > 0) { low_left = low_mid; low_mid = 0.5f * (low_left + low_right); }
        else if (delta_l < 0) { low_right = low_mid; low_mid = 0.5f * (low_left + low_right); }
        if (delta_h > 0) { high_left = high_mid; high_mid = 0.5f * (high_left + high_right); }
        else if (delta_h < 0) { high_right = high_mid; high_mid = 0.5f * (high_left + high_right); }
        return false;
    }
};

// Newton's method of the goal-seek for the linear fit (spec: stackfindsigma.go:101-170), as a state
// machine fed with the counters of one pass at a time.  The reference's quirks are kept: both high
// deltas subtract the LOW target (:114, :155) and the loop counter advances by three per iteration.
struct SigmaNewton {
    float sig_low = 6.0f, sig_high = 6.0f;
    const float epsilon = 0.005f;
    float perc_low, total;
    int i = 0, phase = 0;                 // phase 0: base pass, 1: sig_low + eps, 2: sig_high + eps
    float delta_l = 0, delta_h = 0, new_low = 0;
    int64_t base_lo = 0, base_hi = 0;     // counters of the last base pass (what the reference returns)
    SigmaNewton(float clip_perc_low, int64_t total_samples) : perc_low(clip_perc_low), total((float)total_samples) {}
    // sigmas of the pass to run next
    float next_low() const { return phase == 1 ? sig_low + epsilon : sig_low; }
    float next_high() const { return phase == 2 ? sig_high + epsilon : sig_high; }
    // counters of that pass.  0: go on; 1: done, the pass just run was the base pass; 2: done, but
    // the result image has to be re-made with (sig_low, sig_high) -- a probe pass overwrote it
    int step(int64_t clip_low, int64_t clip_high)
    {
        if (phase == 0) {
            base_lo = clip_low; base_hi = clip_high;
            const float pl = (float)clip_low * 100.0f / total, ph = (float)clip_high * 100.0f / total;
            delta_l = pl - perc_low;
            delta_h = ph - perc_low;                             // sic
            const int li = (int)(100 * delta_l + 0.5f), hi = (int)(100 * delta_h + 0.5f);
            if ((li == 0 && hi == 0) || i >= 20) return 1;
            i++; phase = 1;
            return 0;
        }
        if (phase == 1) {
            const float d2 = (float)clip_low * 100.0f / total - perc_low;
            const float diff = (d2 - delta_l) / epsilon;
            if (diff == 0) return 2;
            new_low = sig_low - delta_l / diff;
            if (new_low < 0.1f) new_low = 0.1f;
            if (new_low > 20) new_low = 20;
            i++; phase = 2;
            return 0;
        }
        const float d3 = (float)clip_high * 100.0f / total - perc_low;      // sic
        const float diff = (d3 - delta_h) / epsilon;
        if (diff == 0) return 2;
        float new_high = sig_high - delta_h / diff;
        if (new_high < 0.1f) new_high = 0.1f;
        if (new_high > 20) new_high = 20;
        sig_low = new_low; sig_high = new_high;
        i++; phase = 0;
        return 0;
    }
};

// where the goal-seek leaves its outcome (the pointers of nl_stack_find_sigmas / nl_group_find_sigmas; any may be null)
struct GoalSeekReport {
    int64_t *clip_low, *clip_high;
    float *sigma_low, *sigma_high;
    int *passes;
};

// The driver.  `mode` is resolved (not NL_ST_AUTO); `total`: the samples the percentages are taken of.
//   counted_pass(sigma_low, sigma_high, c) -> code   one pass, c[0] / c[1] = its clip counters over those samples
//   remake(sigma_low, sigma_high) -> code            the base pass again, after a probe pass overwrote its result; not counted
//   finish() -> code                                 the result of the last pass into the caller's image, if it wants one
// Bisection for sigma / winsorized clipping, Newton's method for the linear fit; the other modes "do not support sigmas"
// (stackfindsigma.go:40-46) and are stacked once with 0, 0.  The report is the counters and sigmas of the pass whose
// result is held when finish() runs; it is written only when every pass succeeded, and before finish().
template <class Pass, class Remake, class Finish>
int goal_seek(int mode, float clip_perc_low, float clip_perc_high, int64_t total, Pass &&counted_pass, Remake &&remake,
              Finish &&finish, const GoalSeekReport &to)
{
    int n_pass = 0;
    auto report = [&](int64_t lo, int64_t hi, float sig_lo, float sig_hi) {
        if (to.clip_low) *to.clip_low = lo;
        if (to.clip_high) *to.clip_high = hi;
        if (to.sigma_low) *to.sigma_low = sig_lo;
        if (to.sigma_high) *to.sigma_high = sig_hi;
        if (to.passes) *to.passes = n_pass;
        return finish();
    };
    int64_t c[2] = {0, 0};
    if (mode == NL_ST_SIGMA || mode == NL_ST_WINSOR_SIGMA) {
        SigmaBisection bis(clip_perc_low, clip_perc_high, total);
        for (;;) {
            const int rc = counted_pass(bis.low_mid, bis.high_mid, c);
            if (rc != NL_OK) return rc;
            n_pass++;
            if (bis.step(c[0], c[1])) return report(c[0], c[1], bis.low_mid, bis.high_mid);
        }
    }
    const bool newton = mode == NL_ST_LINEAR_FIT;
    SigmaNewton nw(clip_perc_low, total);
    for (;;) {
        int rc = counted_pass(newton ? nw.next_low() : 0.0f, newton ? nw.next_high() : 0.0f, c);
        if (rc != NL_OK) return rc;
        n_pass++;
        if (!newton) return report(c[0], c[1], 0.0f, 0.0f);
        const int st = nw.step(c[0], c[1]);
        if (st == 0) continue;
        if (st == 2 && (rc = remake(nw.sig_low, nw.sig_high)) != NL_OK) return rc;
        return report(nw.base_lo, nw.base_hi, nw.sig_low, nw.sig_high);
    }
}

}  // namespace nl
