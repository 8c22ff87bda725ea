// The decision of an identification that is plain functions (depthhead_amd/csrc/dh_fit.h), for
// tests/test_ident_host.py: dh_ident_mean, dh_ident_precedes, dh_ident_status and the picks (dh_ident_pick_add,
// dh_ident_pick_merge) -- a sequential decide over a table of scores, and the decide wave's way (64 lanes striding over the
// candidates, then the xor butterfly of merges), against a brute-force sort of the eligible candidates.  Random tables with many
// exact ties, one candidate, all ineligible, points at min_points and one below, m_best at the limit and one ulp above, m_second
// at min_ratio * m_best and one ulp below.  A stand-alone program: it prints what it checked and exits 0, or says what
// differed and exits 1.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dh_fit.h"

static int failures = 0;
static long checks = 0;
#define EXPECT(cond, ...)                                                                                                       \
    do {                                                                                                                        \
        ++checks;                                                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: " #cond ": ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++failures; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % below);
}

struct Decision {
    uint32_t status, best, second, eligible;
    double m_best, m_second;
};

static bool is_eligible(const dh_fit_record &r, uint32_t min_points) { return r.status == DH_FIT_OK && r.points >= min_points; }

// the definition: sort the eligible candidates by (m, s)
static Decision brute(const std::vector<dh_fit_record> &row, uint32_t min_points, double max_ms, double min_ratio) {
    std::vector<std::pair<double, uint32_t>> e;
    for (uint32_t s = 0; s < row.size(); ++s)
        if (is_eligible(row[s], min_points)) e.push_back({((double)row[s].sum_r2_fixed / 1048576.0) / (double)row[s].points, s});
    std::sort(e.begin(), e.end());
    Decision d{DH_IDENT_OK, DH_IDENT_UNKNOWN, DH_IDENT_UNKNOWN, (uint32_t)e.size(), HUGE_VAL, HUGE_VAL};
    if (e.size() > 0) { d.best = e[0].second; d.m_best = e[0].first; }
    if (e.size() > 1) { d.second = e[1].second; d.m_second = e[1].first; }
    if (e.empty()) d.status = DH_IDENT_NO_CANDIDATE;
    else if (!(d.m_best <= max_ms)) d.status = DH_IDENT_FAR;
    else if (e.size() > 1 && !(d.m_second >= min_ratio * d.m_best)) d.status = DH_IDENT_AMBIGUOUS;
    return d;
}

// one lane after the other
static Decision sequential(const std::vector<dh_fit_record> &row, uint32_t min_points, double max_ms, double min_ratio) {
    IdentPick p = dh_ident_pick_none();
    uint32_t eligible = 0;
    for (uint32_t s = 0; s < row.size(); ++s)
        if (is_eligible(row[s], min_points)) { dh_ident_pick_add(p, dh_ident_mean(row[s].sum_r2_fixed, row[s].points), s); ++eligible; }
    return Decision{dh_ident_status(eligible, p.m_best, p.m_second, max_ms, min_ratio), p.best, p.second, eligible, p.m_best, p.m_second};
}

// the decide wave: lane l takes candidates l, l + 64, ..., then every lane merges with lane ^ o for o = 32 .. 1
static Decision wave(const std::vector<dh_fit_record> &row, uint32_t min_points, double max_ms, double min_ratio) {
    IdentPick lane[64];
    uint32_t count[64];
    for (int l = 0; l < 64; ++l) {
        lane[l] = dh_ident_pick_none();
        count[l] = 0;
        for (uint32_t s = (uint32_t)l; s < row.size(); s += 64)
            if (is_eligible(row[s], min_points)) { dh_ident_pick_add(lane[l], dh_ident_mean(row[s].sum_r2_fixed, row[s].points), s); ++count[l]; }
    }
    for (int o = 32; o; o >>= 1) {
        IdentPick other[64];
        uint32_t oc[64];
        for (int l = 0; l < 64; ++l) { other[l] = lane[l ^ o]; oc[l] = count[l ^ o]; }
        for (int l = 0; l < 64; ++l) { dh_ident_pick_merge(lane[l], other[l]); count[l] += oc[l]; }
    }
    for (int l = 1; l < 64; ++l)
        EXPECT(lane[l].best == lane[0].best && lane[l].second == lane[0].second && count[l] == count[0], "lane %d differs from lane 0", l);
    const IdentPick &p = lane[0];
    return Decision{dh_ident_status(count[0], p.m_best, p.m_second, max_ms, min_ratio), p.best, p.second, count[0], p.m_best, p.m_second};
}

static void same(const char *what, const char *how, const Decision &got, const Decision &want) {
    EXPECT(got.status == want.status && got.best == want.best && got.second == want.second && got.eligible == want.eligible,
           "%s (%s): status %u best %u second %u eligible %u, expected %u %u %u %u", what, how, got.status, got.best, got.second, got.eligible,
           want.status, want.best, want.second, want.eligible);
    EXPECT(memcmp(&got.m_best, &want.m_best, sizeof(double)) == 0 && memcmp(&got.m_second, &want.m_second, sizeof(double)) == 0,
           "%s (%s): m_best %.17g m_second %.17g, expected %.17g %.17g", what, how, got.m_best, got.m_second, want.m_best, want.m_second);
}

static Decision check(const char *what, const std::vector<dh_fit_record> &row, uint32_t min_points, double max_ms, double min_ratio) {
    const Decision want = brute(row, min_points, max_ms, min_ratio);
    same(what, "sequential", sequential(row, min_points, max_ms, min_ratio), want);
    same(what, "wave", wave(row, min_points, max_ms, min_ratio), want);
    return want;
}

static dh_fit_record rec(uint32_t points, int64_t sum, uint32_t status = DH_FIT_OK) {
    dh_fit_record r;
    memset(&r, 0, sizeof r);
    r.points = points; r.status = status; r.sum_r2_fixed = sum; r.steps = 4;
    return r;
}

int main() {
    // ---- the order
    EXPECT(dh_ident_precedes(1.0, 5, 2.0, 0) && !dh_ident_precedes(2.0, 0, 1.0, 5), "smaller m first");
    EXPECT(dh_ident_precedes(1.0, 2, 1.0, 3) && !dh_ident_precedes(1.0, 3, 1.0, 2) && !dh_ident_precedes(1.0, 3, 1.0, 3), "a tie to the lower index");
    EXPECT(dh_ident_precedes(1e300, 7, HUGE_VAL, DH_IDENT_UNKNOWN) && !dh_ident_precedes(HUGE_VAL, DH_IDENT_UNKNOWN, HUGE_VAL, DH_IDENT_UNKNOWN),
           "every candidate precedes none");
    EXPECT(!dh_ident_precedes(NAN, 0, 1.0, 1) && !dh_ident_precedes(1.0, 1, NAN, 0), "a NaN precedes nothing");
    EXPECT(dh_ident_mean(3 << 20, 3) == 1.0 && dh_ident_mean(1, 3) == (1.0 / 1048576.0) / 3.0, "the mean: two divisions");

    // ---- random tables: few distinct values, so ties are everywhere; sizes about the wave's stride
    const uint32_t sizes[] = {1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 256};
    for (uint32_t size : sizes)
        for (int round = 0; round < 200; ++round) {
            std::vector<dh_fit_record> row(size);
            const uint32_t values = 1 + rnd(4), min_points = 6 + rnd(60);
            for (auto &r : row) {
                const uint32_t points = (rnd(4) == 0 ? min_points - 1 - rnd(6) : min_points + rnd(3) * 10);
                r = rec(points, (int64_t)(1 + rnd(values)) * points * 1000, rnd(8) == 0 ? 1u + rnd(2) : DH_FIT_OK);   // m = k * 1000 / 2^20 exactly
                if (rnd(10) == 0) r = rec(0, 0);                                                                   // a pair that did not run
            }
            const double max_ms = rnd(3) ? HUGE_VAL : (double)(1 + rnd(values)) * 1000.0 / 1048576.0;
            const double min_ratio = rnd(2) ? 1.0 : 1.0 + rnd(3);
            check("random", row, min_points, max_ms, min_ratio);
        }

    // ---- exact ties: all equal, the lower indices win, whatever lane they fall on
    for (uint32_t size : sizes) {
        std::vector<dh_fit_record> row(size, rec(100, 100 << 20));
        const Decision d = check("all tied", row, 64, HUGE_VAL, 1.0);
        EXPECT(d.best == 0 && d.second == (size > 1 ? 1u : DH_IDENT_UNKNOWN) && d.status == DH_IDENT_OK, "all tied, %u", size);
        const Decision a = check("all tied, ratio", row, 64, HUGE_VAL, 1.5);
        EXPECT(a.status == (size > 1 ? DH_IDENT_AMBIGUOUS : DH_IDENT_OK), "all tied with a ratio, %u", size);
        if (size > 65) {                                     // the two best on one lane: 1 and 65
            for (auto &r : row) r = rec(100, 200 << 20);
            row[1] = row[65] = rec(100, 100 << 20);
            const Decision t = check("two on one lane", row, 64, HUGE_VAL, 1.0);
            EXPECT(t.best == 1 && t.second == 65, "two on one lane: %u %u", t.best, t.second);
        }
    }
    // ---- one candidate; all ineligible
    {
        const Decision one = check("one candidate", {rec(64, 64 << 20)}, 64, HUGE_VAL, 100.0);
        EXPECT(one.status == DH_IDENT_OK && one.best == 0 && one.second == DH_IDENT_UNKNOWN && one.eligible == 1, "one candidate");
        std::vector<dh_fit_record> none = {rec(63, 1), rec(1000, 1, DH_FIT_FEW_POINTS), rec(1000, 1, DH_FIT_SINGULAR), rec(0, 0)};
        const Decision d = check("all ineligible", none, 64, HUGE_VAL, 1.0);
        EXPECT(d.status == DH_IDENT_NO_CANDIDATE && d.best == DH_IDENT_UNKNOWN && d.second == DH_IDENT_UNKNOWN && d.eligible == 0, "all ineligible");
    }
    // ---- points == min_points takes part, one below does not
    {
        std::vector<dh_fit_record> row = {rec(63, 1), rec(64, 64 << 20)};
        const Decision d = check("points at the limit", row, 64, HUGE_VAL, 1.0);
        EXPECT(d.best == 1 && d.eligible == 1, "points at the limit: best %u eligible %u", d.best, d.eligible);
        EXPECT(check("points below", row, 65, HUGE_VAL, 1.0).status == DH_IDENT_NO_CANDIDATE, "points one below");
    }
    // ---- m_best equal to the limit passes, one ulp above is far
    {
        std::vector<dh_fit_record> row = {rec(100, 283 << 20), rec(100, 400 << 20)};
        const double m = dh_ident_mean(283ll << 20, 100);
        EXPECT(check("at the limit", row, 64, m, 1.0).status == DH_IDENT_OK, "m_best == limit");
        EXPECT(check("above the limit", row, 64, nextafter(m, 0.0), 1.0).status == DH_IDENT_FAR, "m_best one ulp above the limit");
        EXPECT(check("no limit", row, 64, HUGE_VAL, 1.0).status == DH_IDENT_OK, "an infinite limit");
        EXPECT(dh_ident_status(2, NAN, 1.0, HUGE_VAL, 1.0) == DH_IDENT_FAR, "a NaN fails the limit");
    }
    // ---- m_second equal to min_ratio * m_best passes, one ulp below is ambiguous
    {
        const double mb = dh_ident_mean(300ll << 20, 100), ratio = 1.25;
        std::vector<dh_fit_record> row = {rec(100, 300 << 20), rec(100, 375 << 20)};
        EXPECT(dh_ident_mean(375ll << 20, 100) == ratio * mb, "the case is exact");
        EXPECT(check("at the ratio", row, 64, HUGE_VAL, ratio).status == DH_IDENT_OK, "m_second == min_ratio * m_best");
        EXPECT(dh_ident_status(2, mb, nextafter(ratio * mb, 0.0), HUGE_VAL, ratio) == DH_IDENT_AMBIGUOUS, "m_second one ulp below");
        EXPECT(dh_ident_status(2, mb, ratio * mb, HUGE_VAL, nextafter(ratio, 2.0)) == DH_IDENT_AMBIGUOUS, "the ratio one ulp above");
        EXPECT(dh_ident_status(1, mb, HUGE_VAL, HUGE_VAL, 100.0) == DH_IDENT_OK && dh_ident_status(0, HUGE_VAL, HUGE_VAL, HUGE_VAL, 1.0) == DH_IDENT_NO_CANDIDATE,
               "no second, no candidate");
    }
    if (failures) { fprintf(stderr, "%d of %ld checks failed\n", failures, checks); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
