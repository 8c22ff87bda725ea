// The binding lifecycle and the bind-or-retry update that are plain functions (depthhead_amd/csrc/dh_fit.h; DESIGN.md sections 29
// and 30), for tests/test_subject_bind_host.py: dh_sat_inc, dh_subject_unbind, dh_subject_lifecycle and dh_subject_bind_or_retry --
// which k_subject_track.hip and k_rig_subject_track.hip compile as they are -- against the header's text written out a second
// time, over every combination of (tracked, accepted, bound, wait, tries, max_tries) at the edges (0, 1, the limit, 2^32 - 2,
// 2^32 - 1), over every identification status, and over random tracks of 64 steps whose every step is compared; and the decision
// over a row of multi-view scores (dh_view_fit_record) with the picks of dh_fit.h, sequentially and the decide wave's way, against
// a sort.  A stand-alone program: it prints what it checked and exits 0, or says what differed and exits 1.
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

static const uint32_t TOP = 0xffffffffu;

// ---- the header's text once more: rule 2 and the end of rule 3 of section 29
struct Words {
    uint64_t subject, wait, tries, bound_age;      // wider than the words, so that a missing saturation shows
};
static bool lifecycle_text(Words &w, bool tracked, bool accepted, uint32_t max_tries) {
    if (!tracked) { w = Words{TOP, 0, 0, 0}; return false; }
    if (!accepted) return false;                   // a coast: nothing changes
    if (w.subject != TOP) { w.bound_age = std::min<uint64_t>(w.bound_age + 1, TOP); return false; }
    const bool want = w.wait == 0 && (max_tries == 0 || w.tries < max_tries);
    if (!want && w.wait > 0) w.wait -= 1;
    return want;
}
static void ident_text(Words &w, uint32_t status, uint32_t best, uint32_t retry) {
    if (status == DH_IDENT_OK) { w.subject = best; w.bound_age = 0; }
    else { w.tries = std::min<uint64_t>(w.tries + 1, TOP); w.wait = retry; }
}
static bool same(const SubjectBinding &b, const Words &w) {
    return b.subject == w.subject && b.wait == w.wait && b.tries == w.tries && b.bound_age == w.bound_age;
}

static void one(SubjectBinding b, bool tracked, bool accepted, uint32_t max_tries) {
    Words w{b.subject, b.wait, b.tries, b.bound_age};
    const SubjectBinding before = b;
    const bool got = dh_subject_lifecycle(tracked, accepted, max_tries, b.subject, b.wait, b.tries, b.bound_age);
    const bool want = lifecycle_text(w, tracked, accepted, max_tries);
    EXPECT(got == want && same(b, w), "lifecycle(%d, %d, max_tries %u) of (%u, %u, %u, %u): want %d -> (%u, %u, %u, %u)", tracked, accepted, max_tries,
           before.subject, before.wait, before.tries, before.bound_age, got, b.subject, b.wait, b.tries, b.bound_age);
    if (got) EXPECT(before.subject == DH_IDENT_UNKNOWN && memcmp(&b, &before, sizeof b) == 0, "a wanting track is unbound and unchanged");
}

// ---- the decision over multi-view scores: dh_fit.h's picks against a sort
static dh_view_fit_record score(uint32_t points, int64_t sum, uint32_t status = DH_FIT_OK) {
    dh_view_fit_record r;
    memset(&r, 0, sizeof r);
    r.points = points; r.status = status; r.sum_r2_fixed = sum; r.steps = 4; r.views_used = 7;
    return r;
}
static void decide(const std::vector<dh_view_fit_record> &row, uint32_t min_points, double max_ms, double min_ratio) {
    std::vector<std::pair<double, uint32_t>> e;
    for (uint32_t s = 0; s < row.size(); ++s)
        if (row[s].status == DH_FIT_OK && row[s].points >= min_points) e.push_back({((double)row[s].sum_r2_fixed / 1048576.0) / (double)row[s].points, s});
    std::sort(e.begin(), e.end());
    uint32_t status = DH_IDENT_OK;
    if (e.empty()) status = DH_IDENT_NO_CANDIDATE;
    else if (!(e[0].first <= max_ms)) status = DH_IDENT_FAR;
    else if (e.size() > 1 && !(e[1].first >= min_ratio * e[0].first)) status = DH_IDENT_AMBIGUOUS;
    const uint32_t best = e.size() > 0 ? e[0].second : DH_IDENT_UNKNOWN, second = e.size() > 1 ? e[1].second : DH_IDENT_UNKNOWN;
    // the decide wave: lane l takes candidates l, l + 64, ..., then every lane merges with lane ^ o for o = 32 .. 1
    IdentPick lane[64];
    uint32_t count[64];
    for (int l = 0; l < 64; ++l) {
        lane[l] = dh_ident_pick_none();
        count[l] = 0;
        for (uint32_t s = (uint32_t)l; s < row.size(); s += 64)
            if (row[s].status == DH_FIT_OK && row[s].points >= min_points) { dh_ident_pick_add(lane[l], dh_ident_mean(row[s].sum_r2_fixed, row[s].points), s); ++count[l]; }
    }
    for (int o = 32; o; o >>= 1) {
        IdentPick other[64];
        uint32_t oc[64];
        for (int l = 0; l < 64; ++l) { other[l] = lane[l ^ o]; oc[l] = count[l ^ o]; }
        for (int l = 0; l < 64; ++l) { dh_ident_pick_merge(lane[l], other[l]); count[l] += oc[l]; }
    }
    const uint32_t got = dh_ident_status(count[0], lane[0].m_best, lane[0].m_second, max_ms, min_ratio);
    EXPECT(got == status && lane[0].best == best && lane[0].second == second && count[0] == e.size(),
           "decide over %zu scores: status %u best %u second %u eligible %u, expected %u %u %u %zu", row.size(), got, lane[0].best, lane[0].second, count[0],
           status, best, second, e.size());
    // and what the decision makes of an unbound entry's words
    SubjectBinding b{DH_IDENT_UNKNOWN, 0, 3, 9};
    Words w{b.subject, b.wait, b.tries, b.bound_age};
    dh_subject_bind_or_retry(got, lane[0].best, 4, b.subject, b.wait, b.tries, b.bound_age);
    ident_text(w, status, best, 4);
    EXPECT(same(b, w), "bind or retry after status %u", got);
}

int main() {
    const uint32_t edge[] = {0, 1, 2, 4, TOP - 1, TOP};
    // ---- the counters
    EXPECT(dh_sat_inc(0) == 1 && dh_sat_inc(TOP - 1) == TOP && dh_sat_inc(TOP) == TOP, "saturating + 1");
    {
        SubjectBinding b{5, 6, 7, 8};
        dh_subject_unbind(b.subject, b.wait, b.tries, b.bound_age);
        EXPECT(b.subject == DH_IDENT_UNKNOWN && b.wait == 0 && b.tries == 0 && b.bound_age == 0, "unbind");
    }
    // ---- the lifecycle at the edges: every combination
    for (int tracked = 0; tracked < 2; ++tracked)
        for (int accepted = 0; accepted < 2; ++accepted)
            for (uint32_t subject : {0u, 63u, TOP - 1, TOP})
                for (uint32_t wait : edge)
                    for (uint32_t tries : edge)
                        for (uint32_t age : edge)
                            for (uint32_t max_tries : edge) one(SubjectBinding{subject, wait, tries, age}, tracked != 0, accepted != 0, max_tries);
    // ---- the identification's outcome for every status
    for (uint32_t status : {(uint32_t)DH_IDENT_OK, (uint32_t)DH_IDENT_SKIPPED, (uint32_t)DH_IDENT_NO_CANDIDATE, (uint32_t)DH_IDENT_FAR, (uint32_t)DH_IDENT_AMBIGUOUS})
        for (uint32_t tries : edge)
            for (uint32_t retry : edge) {
                SubjectBinding b{DH_IDENT_UNKNOWN, 0, tries, 77};
                Words w{b.subject, b.wait, b.tries, b.bound_age};
                dh_subject_bind_or_retry(status, 5, retry, b.subject, b.wait, b.tries, b.bound_age);
                ident_text(w, status, 5, retry);
                EXPECT(same(b, w), "status %u tries %u retry %u -> (%u, %u, %u, %u)", status, tries, retry, b.subject, b.wait, b.tries, b.bound_age);
                EXPECT((b.subject == 5) == (status == DH_IDENT_OK), "only DH_IDENT_OK binds");
            }
    // ---- random tracks: 64 steps each, every step compared, and what the header promises of (retry, max_tries)
    for (int round = 0; round < 400; ++round) {
        const uint32_t retry = rnd(4), max_tries = rnd(4);
        SubjectBinding b;
        dh_subject_unbind(b.subject, b.wait, b.tries, b.bound_age);
        Words w{b.subject, b.wait, b.tries, b.bound_age};
        uint32_t tried = 0, since = TOP;
        for (int step = 0; step < 64; ++step) {
            const bool tracked = rnd(12) != 0, accepted = tracked && rnd(5) != 0;
            const bool got = dh_subject_lifecycle(tracked, accepted, max_tries, b.subject, b.wait, b.tries, b.bound_age);
            const bool want = lifecycle_text(w, tracked, accepted, max_tries);
            EXPECT(got == want && same(b, w), "round %d step %d", round, step);
            if (!tracked) { tried = 0; since = TOP; }
            if (accepted && since != TOP) ++since;
            if (got) {
                EXPECT(max_tries == 0 || tried < max_tries, "a try past max_tries %u", max_tries);
                EXPECT(since == TOP || since == retry + 1, "a try %u accepted steps after the last, retry %u", since, retry);
                const uint32_t status = rnd(6) == 0 ? DH_IDENT_OK : 1 + rnd(4);
                dh_subject_bind_or_retry(status, rnd(64), retry, b.subject, b.wait, b.tries, b.bound_age);
                w.subject = b.subject;             // (the same best)
                if (status != DH_IDENT_OK) { ident_text(w, status, 0, retry); ++tried; since = 0; }
                else w.bound_age = 0;
                EXPECT(same(b, w), "round %d step %d after the identification", round, step);
            }
        }
    }
    // ---- the decision over rows of multi-view scores, sizes about the wave's stride, few distinct values so ties are everywhere
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 129};
    for (uint32_t size : sizes)
        for (int round = 0; round < 60; ++round) {
            std::vector<dh_view_fit_record> row(size);
            const uint32_t values = 1 + rnd(4), min_points = 6 + rnd(60);
            for (auto &r : row) {
                const uint32_t points = (rnd(4) == 0 ? min_points - 1 - rnd(6) : min_points + rnd(3) * 10);
                r = score(points, (int64_t)(1 + rnd(values)) * points * 1000, rnd(8) == 0 ? 1u + rnd(2) : DH_FIT_OK);
                if (rnd(10) == 0) r = score(0, 0);
            }
            decide(row, min_points, rnd(3) ? HUGE_VAL : (double)(1 + rnd(values)) * 1000.0 / 1048576.0, rnd(2) ? 1.0 : 1.0 + rnd(3));
        }
    if (failures) { fprintf(stderr, "%d of %ld checks failed\n", failures, checks); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
