// dh_rig_fit.h -- the bind of a rig fit tracker's step (dh_rig_fit_tracker_step*): which of a rig's DH_RIG_MAX_TRACKS slots is
// an entry of the state that a person of this step holds, an entry no person holds, an unbound person, or unused.  Written
// once, in its sequential form: lane 0 of k_rig_fit_seed's workgroup (k_rig_fit_track.hip) runs dh_rig_fit_bind as it stands,
// and so does the host check (tests/host/rig_fit_check.cpp).  Plain C++ outside hipcc, integers only.
//
// Not in the reference: the rule is this library's own, stated in include/depthhead_hip.h (section "carrying each rig person's
// fitted world pose across steps", step 1) and DESIGN.md section 22.
#pragma once
#include <stdint.h>
#include <string.h>

#include "dh_rig.h"

static_assert(sizeof(dh_rig_fit_track_params) == 48, "dh_rig_fit_track_params: 48 bytes");
static_assert(sizeof(dh_rig_fit_state) == 88 && alignof(dh_rig_fit_state) == 8, "dh_rig_fit_state: 88 bytes, no padding");
static_assert(sizeof(dh_rig_fit_record) == 128 && alignof(dh_rig_fit_record) == 8, "dh_rig_fit_record: 128 bytes, no padding");
static_assert(DH_RIG_MAX_PERSONS <= 32 && DH_RIG_MAX_TRACKS <= 32, "the bind keeps persons and slots in 32-bit masks");

// What a slot of the rig is in this step.
#define DH_RIG_FIT_UNUSED 0u        // a free entry that no unbound person took: no record
#define DH_RIG_FIT_SEEN 1u          // an entry, and person[s] holds it
#define DH_RIG_FIT_UNSEEN 2u        // an entry that is tracked and that no person holds
#define DH_RIG_FIT_UNBOUND 3u       // no entry: person[s] is fitted from its detection and reported
#define DH_RIG_FIT_NO_PERSON 0xffffffffu

// Does person p name a head of the step?  n_heads [n_cams] of the whole camera table.
DH_HD inline bool dh_rig_fit_names_head_(const dh_rig_person &p, const uint32_t *n_heads, int n_cams, int max_heads) {
    if (p.best_cam >= (uint32_t)n_cams) return false;
    uint32_t nh = n_heads[p.best_cam];
    if (nh > (uint32_t)max_heads) nh = (uint32_t)max_heads;
    return p.best_head < nh;
}

// Step 1 of the header for one rig.  st: the rig's DH_RIG_MAX_TRACKS entries (new entries get their id, unseen entries that
// are not tracked are zeroed); persons: the rig's DH_RIG_MAX_PERSONS records.  Written: role [DH_RIG_MAX_TRACKS] (DH_RIG_FIT_*)
// and person [DH_RIG_MAX_TRACKS] (the index of the slot's person, or DH_RIG_FIT_NO_PERSON).
DH_HD inline void dh_rig_fit_bind(dh_rig_fit_state *st, const dh_rig_person *persons, uint32_t n_persons, const uint32_t *n_heads,
                                  int n_cams, int max_heads, uint32_t *role, uint32_t *person) {
    for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) {
        role[s] = st[s].id != 0 ? DH_RIG_FIT_UNSEEN : DH_RIG_FIT_UNUSED;
        person[s] = DH_RIG_FIT_NO_PERSON;
    }
    const int np = n_persons > DH_RIG_MAX_PERSONS ? DH_RIG_MAX_PERSONS : (int)n_persons;
    uint32_t unbound = 0;
    for (int i = 0; i < np; ++i) {
        if (!dh_rig_fit_names_head_(persons[i], n_heads, n_cams, max_heads)) continue;
        const uint32_t id = persons[i].id;
        int slot = -1;
        if (id != 0) {
            for (int s = DH_RIG_MAX_TRACKS - 1; s >= 0; --s) slot = st[s].id == id ? s : slot;
            if (slot >= 0) {
                if (role[slot] == DH_RIG_FIT_SEEN) slot = -1;          // an earlier person of this step holds the id
            } else {
                for (int s = DH_RIG_MAX_TRACKS - 1; s >= 0; --s) slot = st[s].id == 0 ? s : slot;
                if (slot >= 0) {
                    memset(&st[slot], 0, sizeof st[slot]);
                    st[slot].id = id;
                }
            }
        }
        if (slot >= 0) { role[slot] = DH_RIG_FIT_SEEN; person[slot] = (uint32_t)i; }
        else unbound |= 1u << i;
    }
    for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s)
        if (role[s] == DH_RIG_FIT_UNSEEN && !st[s].tracked) {
            memset(&st[s], 0, sizeof st[s]);
            role[s] = DH_RIG_FIT_UNUSED;
        }
    for (int i = 0; i < np; ++i) {
        if (!(unbound >> i & 1u)) continue;
        int slot = -1;
        for (int s = DH_RIG_MAX_TRACKS - 1; s >= 0; --s) slot = role[s] == DH_RIG_FIT_UNUSED ? s : slot;
        if (slot < 0) break;                                           // (no later person finds a slot either)
        role[slot] = DH_RIG_FIT_UNBOUND;
        person[slot] = (uint32_t)i;
    }
}
