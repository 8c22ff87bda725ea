// dh_track_heads.h -- the step of a multi-head tracker (dh_multi_tracker_step): the heads of one frame matched against one
// camera's tracks, written once for k_track_heads (k_track_heads.hip) and for the host checks (tests/host/multi_track_check.cpp).
// Plain C++ outside hipcc, as dh_track.h.  Integer only: host and device agree bit for bit.
//
// Not in the reference (it tracks one pose per camera): the rule is this library's own, stated in include/depthhead_hip.h
// (section "several heads per camera with persistent identities") and DESIGN.md section 15.  In short, per present camera:
// cells of the tracks' and heads' midpoints; Chebyshev distances in 64 bits; greedy matching of the pairs within the gate in the
// order (d, head j, slot t); matched tracks take their head; unmatched tracks coast and are freed after max_misses misses;
// unmatched heads are born in the lowest free slots with fresh ids (next_id wraps from UINT32_MAX to 1, so 0 is never an id,
// and ids are unique per camera until 2^32 - 1 births).  The defaults, DH_TRACK_GATE 100 mm and DH_TRACK_MAX_MISSES 3, are
// choices: 100 mm per step admits 3 m/s at 30 Hz and is five times the heads' 20-cell merge distance; 3 misses coast 100 ms.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/depthhead_hip.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define DH_HD __host__ __device__
#else
#define DH_HD
#endif

static_assert(sizeof(dh_head_track) == 96, "dh_head_track: 96 bytes");
static_assert(sizeof(dh_multi_track_params) == 16, "dh_multi_track_params: 16 bytes");

// Rust `f32 as i32` (f32_as_i32 of dh_device.h: truncation toward zero, NaN -> 0, saturating), on host and device
DH_HD inline int64_t dh_th_cell_(float v) {
    if (v != v) return 0;
    if (v >= 2147483648.0f) return INT32_MAX;
    if (v <= -2147483648.0f) return INT32_MIN;
    return (int64_t)(int32_t)v;
}
DH_HD inline uint32_t dh_th_inc_(uint32_t v) { return v == UINT32_MAX ? v : v + 1u; }

// One present camera's step.  tr: its DH_MAX_TRACKS records, *next_id its next id, heads[0 .. n) the step's heads (n is clamped
// to max_heads), ids[0 .. max_heads) written.  gate: 0 .. 2^31 - 1 (the entry points refuse more).
DH_HD inline void dh_track_heads_step(dh_head_track *tr, uint32_t *next_id, const dh_head *heads, uint32_t n, int max_heads,
                                      uint32_t gate, uint32_t max_misses, uint32_t *ids) {
    if (n > (uint32_t)max_heads) n = (uint32_t)max_heads;
    int64_t tc[DH_MAX_TRACKS][3], hc[DH_MAX_HEADS][3];
    uint32_t live = 0, t_used = 0, h_used = 0;     // bit t / bit j (bit masks, not arrays: no dynamic register indexing)
    for (int t = 0; t < DH_MAX_TRACKS; ++t) {
        live |= tr[t].id != 0 ? 1u << t : 0u;
        for (int q = 0; q < 3; ++q) tc[t][q] = dh_th_cell_(tr[t].head.pose.mid_point[q]);
    }
    for (int j = 0; j < DH_MAX_HEADS; ++j)
        for (int q = 0; q < 3; ++q) hc[j][q] = (uint32_t)j < n ? dh_th_cell_(heads[j].pose.mid_point[q]) : 0;
    for (int j = 0; j < max_heads; ++j) ids[j] = 0;
    // greedy matching: each round accepts the least (d, j, t) among the free pairs within the gate; at most n rounds
    for (uint32_t round = 0; round < n; ++round) {
        int64_t best = INT64_MAX;
        int bj = -1, bt = -1;
        for (int j = 0; j < DH_MAX_HEADS; ++j) {
            if ((uint32_t)j >= n || (h_used >> j & 1u)) continue;
            for (int t = 0; t < DH_MAX_TRACKS; ++t) {
                if (!(live >> t & 1u) || (t_used >> t & 1u)) continue;
                int64_t d = 0;
                for (int q = 0; q < 3; ++q) {
                    const int64_t dq = tc[t][q] - hc[j][q];
                    d = d > (dq < 0 ? -dq : dq) ? d : (dq < 0 ? -dq : dq);
                }
                if (d <= (int64_t)gate && d < best) { best = d; bj = j; bt = t; }   // (j, then t, ascending: the first least d wins)
            }
        }
        if (bj < 0) break;
        h_used |= 1u << bj;
        t_used |= 1u << bt;
        dh_head_track &m = tr[bt];
        memcpy(&m.head, &heads[bj], sizeof(dh_head));
        m.hits = dh_th_inc_(m.hits);
        m.age = dh_th_inc_(m.age);
        m.misses = 0;
        ids[bj] = m.id;
    }
    // unmatched live tracks coast, and are freed after max_misses consecutive misses
    for (int t = 0; t < DH_MAX_TRACKS; ++t) {
        if (!(live >> t & 1u) || (t_used >> t & 1u)) continue;
        dh_head_track &m = tr[t];
        m.age = dh_th_inc_(m.age);
        m.misses = dh_th_inc_(m.misses);
        if (m.misses > max_misses) memset(&m, 0, sizeof m);
    }
    // unmatched heads are born in the lowest free slots
    for (int j = 0; j < DH_MAX_HEADS; ++j) {
        if ((uint32_t)j >= n || (h_used >> j & 1u)) continue;
        int slot = -1;
        for (int t = DH_MAX_TRACKS - 1; t >= 0; --t) slot = tr[t].id == 0 ? t : slot;
        if (slot < 0) break;                                  // (every later head finds no slot either: their ids stay 0)
        dh_head_track &m = tr[slot];
        m.id = *next_id;
        m.age = 1u; m.hits = 1u; m.misses = 0u;
        memcpy(&m.head, &heads[j], sizeof(dh_head));
        *next_id = *next_id == UINT32_MAX ? 1u : *next_id + 1u;
        ids[j] = m.id;
    }
}
