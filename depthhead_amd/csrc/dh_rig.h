// dh_rig.h -- the step of a rig tracker (dh_rig_tracker_step): the heads of a rig's cameras carried into the rig's world frame,
// fused into persons and matched against the rig's tracks.  Written once: the pieces (world transform, cell, distance, order,
// mean, saturating sums, match key) are what k_rig_fuse (k_rig.hip) is built from, and dh_rig_step below -- the rule in its
// sequential form -- is the definition, and what the host checks run (tests/host/rig_check.cpp).  Plain C++ outside hipcc, as
// dh_track_heads.h.  Integer apart from the three products and three sums of the transform, each rounded on its own: host and
// device agree bit for bit (build the host side with -ffp-contract=off).
//
// Not in the reference (one pose from one camera): the rule is this library's own, stated in include/depthhead_hip.h (section
// "camera rigs") and DESIGN.md section 16.
#pragma once
#include <stdint.h>
#include <string.h>

#include "dh_track_heads.h"

static_assert(sizeof(dh_rig_person) == 56 && alignof(dh_rig_person) == 8, "dh_rig_person: 56 bytes, no padding");
static_assert(sizeof(dh_rig_track) == 72 && alignof(dh_rig_track) == 8, "dh_rig_track: 72 bytes, no padding");
static_assert(sizeof(dh_rig_track_params) == 20, "dh_rig_track_params: 20 bytes");
static_assert(DH_RIG_MAX_CAMERAS == 64, "a person's views are a 64-bit mask");
static_assert(DH_RIG_MAX_PERSONS == 16 && DH_RIG_MAX_TRACKS == 16, "the match key packs person and slot into 4 bits each");

#define DH_RIG_MAX_RIG_HEADS (DH_RIG_MAX_CAMERAS * DH_MAX_HEADS)

// ((R[q][0] m0 + R[q][1] m1) + R[q][2] m2) + t[q], every product and sum rounded on its own
DH_HD inline float dh_rig_world_(const float *R, const float *t, const float *m, int q) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3 * q], m[0]), __fmul_rn(R[3 * q + 1], m[1])), __fmul_rn(R[3 * q + 2], m[2])), t[q]);
#else
    volatile float a = R[3 * q] * m[0], b = R[3 * q + 1] * m[1], c = R[3 * q + 2] * m[2];   // (volatile: no contraction whatever the flags)
    volatile float ab = a + b;
    volatile float abc = ab + c;
    return abc + t[q];
#endif
}
// Chebyshev distance of two cells (int32 values widened), in 64 bits: at most 2^32 - 1
DH_HD inline int64_t dh_rig_cheb_(const int32_t *a, const int32_t *b) {
    int64_t d = 0;
    for (int q = 0; q < 3; ++q) {
        const int64_t dq = (int64_t)a[q] - (int64_t)b[q], aq = dq < 0 ? -dq : dq;
        d = d > aq ? d : aq;
    }
    return d;
}
// head a = (mass, lane) precedes head b in the order of step 1; lane = (camera - rig_begin) * DH_MAX_HEADS + j
DH_HD inline bool dh_rig_before_(uint64_t mass_a, uint32_t lane_a, uint64_t mass_b, uint32_t lane_b) {
    return mass_a > mass_b || (mass_a == mass_b && lane_a < lane_b);
}
DH_HD inline int64_t dh_rig_floor_div_(int64_t s, int64_t n) {   // n > 0
    const int64_t q = s / n;
    return (s % n != 0 && s < 0) ? q - 1 : q;
}
DH_HD inline uint64_t dh_rig_sat_add_(uint64_t a, uint64_t b) { return a + b < a ? UINT64_MAX : a + b; }
// pairs are taken in ascending order of this key; d <= gate <= 2^31 - 1
DH_HD inline uint64_t dh_rig_key_(int64_t d, int person, int slot) { return (uint64_t)d << 8 | (uint64_t)person << 4 | (uint64_t)slot; }

// One rig's step, sequential.  n_cams cameras (1 .. DH_RIG_MAX_CAMERAS), camera k of the rig being camera cam0 + k of the table:
// R [n_cams][9], t [n_cams][3], present nullable [n_cams], n_heads [n_cams], heads [n_cams][max_heads].  tr: the rig's
// DH_RIG_MAX_TRACKS records, *next_id its next id.  Written: ids [n_cams][max_heads], *n_persons, persons [DH_RIG_MAX_PERSONS].
DH_HD inline void dh_rig_step(dh_rig_track *tr, uint32_t *next_id, const float *R, const float *t, const uint8_t *present,
                              const uint32_t *n_heads, const dh_head *heads, int n_cams, uint32_t cam0, int max_heads,
                              uint32_t fuse_gate, uint32_t gate, uint32_t max_misses, uint32_t *ids, uint32_t *n_persons,
                              dh_rig_person *persons) {
    for (int i = 0; i < n_cams * max_heads; ++i) ids[i] = 0;
    *n_persons = 0;
    memset(persons, 0, sizeof(dh_rig_person) * DH_RIG_MAX_PERSONS);
    bool any = false;
    for (int k = 0; k < n_cams; ++k) any = any || !present || present[k];
    if (!any) return;                                           // no present camera: the rig keeps its whole state

    // 0. world midpoints and cells of the present cameras' heads; lane = k * DH_MAX_HEADS + j
    float world[DH_RIG_MAX_RIG_HEADS][3];
    int32_t cell[DH_RIG_MAX_RIG_HEADS][3];
    uint64_t mass[DH_RIG_MAX_RIG_HEADS];
    int order[DH_RIG_MAX_RIG_HEADS], person_of[DH_RIG_MAX_RIG_HEADS], n = 0;
    for (int k = 0; k < n_cams; ++k) {
        if (present && !present[k]) continue;
        uint32_t nh = n_heads[k];
        if (nh > (uint32_t)max_heads) nh = (uint32_t)max_heads;
        for (int j = 0; j < (int)nh; ++j) {
            const dh_head &h = heads[k * max_heads + j];
            const int l = k * DH_MAX_HEADS + j;
            for (int q = 0; q < 3; ++q) {
                world[l][q] = dh_rig_world_(R + 9 * k, t + 3 * k, h.pose.mid_point, q);
                cell[l][q] = (int32_t)dh_th_cell_(world[l][q]);
            }
            mass[l] = h.support.mass;
            person_of[l] = -1;
            // 1. the order: insertion keeps (mass descending, lane ascending)
            int at = n++;
            while (at > 0 && dh_rig_before_(mass[l], (uint32_t)l, mass[order[at - 1]], (uint32_t)order[at - 1])) { order[at] = order[at - 1]; --at; }
            order[at] = l;
        }
    }
    // 2. fuse
    int np = 0, anchor[DH_RIG_MAX_PERSONS];
    int64_t sum[DH_RIG_MAX_PERSONS][3];
    dh_rig_person *P = persons;
    for (int r = 0; r < n; ++r) {
        const int l = order[r], k = l / DH_MAX_HEADS;
        int p = 0;
        for (; p < np; ++p)
            if (dh_rig_cheb_(cell[anchor[p]], cell[l]) <= (int64_t)fuse_gate && !(P[p].views >> k & 1u)) break;
        if (p == np) {
            if (np == DH_RIG_MAX_PERSONS) continue;             // unassigned
            ++np;
            anchor[p] = l;
            for (int q = 0; q < 3; ++q) { sum[p][q] = 0; P[p].world[q] = world[l][q]; }
            P[p].best_cam = cam0 + (uint32_t)k;
            P[p].best_head = (uint32_t)(l % DH_MAX_HEADS);
        }
        person_of[l] = p;
        P[p].views |= (uint64_t)1 << k;
        P[p].n_views += 1u;
        P[p].mass = dh_rig_sat_add_(P[p].mass, mass[l]);
        for (int q = 0; q < 3; ++q) sum[p][q] += cell[l][q];
    }
    // 3. person records
    for (int p = 0; p < np; ++p)
        for (int q = 0; q < 3; ++q) P[p].cell[q] = (int32_t)dh_rig_floor_div_(sum[p][q], (int64_t)P[p].n_views);
    *n_persons = (uint32_t)np;
    // 4. match: each round accepts the least key among the free pairs within the gate
    uint32_t live = 0, t_used = 0, p_used = 0;
    for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) live |= tr[s].id != 0 ? 1u << s : 0u;
    int32_t tcell[DH_RIG_MAX_TRACKS][3];
    for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) for (int q = 0; q < 3; ++q) tcell[s][q] = tr[s].person.cell[q];
    for (int round = 0; round < np; ++round) {
        uint64_t best = UINT64_MAX;
        for (int p = 0; p < np; ++p) {
            if (p_used >> p & 1u) continue;
            for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) {
                if (!(live >> s & 1u) || (t_used >> s & 1u)) continue;
                const int64_t d = dh_rig_cheb_(tcell[s], P[p].cell);
                if (d <= (int64_t)gate && dh_rig_key_(d, p, s) < best) best = dh_rig_key_(d, p, s);
            }
        }
        if (best == UINT64_MAX) break;
        const int p = (int)(best >> 4 & 15u), s = (int)(best & 15u);
        p_used |= 1u << p;
        t_used |= 1u << s;
        P[p].id = tr[s].id;
        tr[s].person = P[p];
        tr[s].hits = dh_th_inc_(tr[s].hits);
        tr[s].age = dh_th_inc_(tr[s].age);
        tr[s].misses = 0;
    }
    for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) {
        if (!(live >> s & 1u) || (t_used >> s & 1u)) continue;
        tr[s].age = dh_th_inc_(tr[s].age);
        tr[s].misses = dh_th_inc_(tr[s].misses);
        if (tr[s].misses > max_misses) memset(&tr[s], 0, sizeof tr[s]);
    }
    for (int p = 0; p < np; ++p) {
        if (p_used >> p & 1u) continue;
        int slot = -1;
        for (int s = DH_RIG_MAX_TRACKS - 1; s >= 0; --s) slot = tr[s].id == 0 ? s : slot;
        if (slot < 0) break;                                    // (no later person finds a slot either: their ids stay 0)
        P[p].id = *next_id;
        *next_id = *next_id == UINT32_MAX ? 1u : *next_id + 1u;
        tr[slot].id = P[p].id;
        tr[slot].age = 1u; tr[slot].hits = 1u; tr[slot].misses = 0u;
        tr[slot].person = P[p];
    }
    // 5. the heads' ids
    for (int r = 0; r < n; ++r) {
        const int l = order[r];
        if (person_of[l] >= 0) ids[(l / DH_MAX_HEADS) * max_heads + l % DH_MAX_HEADS] = P[person_of[l]].id;
    }
}
