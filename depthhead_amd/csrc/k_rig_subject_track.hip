// k_rig_subject_track.hip -- each rig person followed with its own subject's model (the rule is stated in
// include/depthhead_hip.h, section "following each rig person with its own subject's model").  Four kernels around k_fit_views'
// per-instance-schedule instance (k_fit_views.hip), which fits over a table of the set's S models and the generic one at index S,
// over the DH_RIG_MAX_TRACKS slots of every rig:
//   k_rig_subject_seed    one workgroup per rig: section 22's seed (rig_fit_seed_rig, dh_fit_device.h) with the start's model -- the
//                         entry's subject where it is bound, else S.  Where the bind founded or freed an entry (its id changed) the
//                         four words of the binding go back to (DH_IDENT_UNKNOWN, 0, 0, 0); the step's want count is cleared;
//   k_rig_subject_update  one lane per slot: section 22's steps 4 - 6 on the entry's dh_rig_fit_state, the binding lifecycle on the
//                         four words beside it, and the slots that want identification appended to a compact list: a ballot over
//                         the wave, one integer atomic per wave for the wave's share of the list, each wanting lane at its rank.
//                         The list's order is the atomics' and so free; wants[slot] says the same per slot, and every output of
//                         the step is indexed by slot;
//   k_rig_subject_score   the hot path: a fixed grid of workgroups of DH_FIT_THREADS lanes, each looping over the pairs (list entry,
//                         subject) of this step with the subject the fast index.  A trip is k_ident_views_score's body:
//                         ident_views_takes_part and ident_views_run (dh_fit_device.h) on the slot's fitted instance over all its
//                         views, the score and the pose written at [slot][subject] of the tracker's scratch.  The trip count
//                         depends on blockIdx, gridDim and the list's length alone, so it is uniform over the workgroup and every
//                         barrier of fit_views_pass is reached by all lanes; a barrier closes every trip, the early-leaving ones
//                         too, before the next one stages its model over the LDS the last pass read.  A set holds one point count,
//                         so staged or streamed is decided once, by the launcher: each instance of the kernel holds one
//                         instantiation of the pass, which keeps the loop below the 256 registers of two waves per SIMD;
//   k_rig_subject_bind    one wave per slot: for a slot on the list the decision (ident_decide, dh_fit_device.h), then the binding
//                         and the record's identification half by lane 0; for every other slot lane 0 writes the SKIPPED half.
//   k_rig_subject_set     dh_rig_subject_fit_tracker_bind: one wave looks for the entry of a rig that holds an id.
// f32 and f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free; one
// integer atomic per wave: bit-identical run to run and to tests/rig_subject_track_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

static_assert(DH_RIG_MAX_TRACKS <= DH_RIG_FIT_THREADS, "one lane per slot of a rig");
static_assert(DH_RIG_FIT_THREADS == 64, "the update kernel's workgroup is one wave: one ballot, one atomic");

__global__ __launch_bounds__(DH_RIG_FIT_THREADS) void k_rig_subject_seed(const RigSubjectArgs g) {
    __shared__ dh_rig_fit_state s_st[DH_RIG_MAX_TRACKS];
    __shared__ dh_rig_person s_p[DH_RIG_MAX_PERSONS];
    __shared__ uint32_t s_role[DH_RIG_MAX_TRACKS], s_who[DH_RIG_MAX_TRACKS];
    if (blockIdx.x == 0 && threadIdx.x == 0) *g.n_want = 0;
    const uint32_t S = g.q.n_subjects;
    SubjectBinding *bound = g.bound;
    rig_fit_seed_rig(g.a, s_st, s_p, s_role, s_who, [=](size_t slot, const dh_rig_fit_state *old, const dh_rig_fit_state &st, uint32_t role) {
        uint32_t subject = bound[slot].subject;
        if (old->id != st.id) {                          // the bind founded or freed the entry
            SubjectBinding none;
            dh_subject_unbind(none.subject, none.wait, none.tries, none.bound_age);
            bound[slot] = none;
            subject = none.subject;
        }
        return role != DH_RIG_FIT_UNBOUND && subject < S ? subject : S;
    });
}

__global__ __launch_bounds__(DH_RIG_FIT_THREADS) void k_rig_subject_update(const RigSubjectArgs g) {
    const RigFitArgs &a = g.a;
    const int slot = blockIdx.x * DH_RIG_FIT_THREADS + threadIdx.x;
    bool want = false;                                   // (a lane past the slots stays for the ballot)
    if (slot < a.n_rigs * DH_RIG_MAX_TRACKS) {
        const int rig = slot / DH_RIG_MAX_TRACKS;
        const uint32_t seed = a.seed[slot], kind = seed & 0xffu, pi = a.who[slot];
        const bool seen = (seed & DH_RIG_FIT_SEED_IS_SEEN) != 0, entry = (seed & DH_RIG_FIT_SEED_IS_ENTRY) != 0;
        dh_rig_fit_record rec;
        memset(&rec, 0, sizeof rec);
        uint32_t model = DH_IDENT_UNKNOWN;
        if (kind == DH_FIT_SEED_NONE || kind == DH_FIT_SEED_ABSENT) {
            if (kind == DH_FIT_SEED_ABSENT) rec.status = DH_FIT_TRACK_ABSENT;
        } else {
            dh_rig_fit_state st;
            memset(&st, 0, sizeof st);
            if (entry) st = a.state[slot];
            bool free_it = false, accepted = false;
            rec.person = pi;
            if (kind == DH_FIT_SEED_COAST) {
                st.lost = fit_sat_inc(st.lost);
                st.have_prev = 0;
                free_it = st.lost > a.prm.max_coast;
                rec.status = DH_FIT_TRACK_ABSENT;
            } else {
                const dh_view_instance fit = a.fit_out[slot];
                const dh_view_fit_record fr = a.fit_rec[slot];
                uint32_t why = fit_track_why(fr, a.prm.keep_points, a.rms_lim);
                // pi < DH_RIG_MAX_PERSONS: the bind's
                if (seen) why |= fit_track_jump(fit.t, a.persons[(size_t)rig * DH_RIG_MAX_PERSONS + pi].world, a.jump2);
                rec.fit = fr;
                if (fit.model < g.q.n_subjects) model = fit.model;     // (the fit copies the start's model through)
                if (why == 0) {
                    DH_FIT_TRACK_ACCEPT(st, fit);
                    st.views_used = fr.views_used;
                    rec.instance = fit;
                    rec.status = kind == DH_FIT_SEED_CARRIED ? DH_FIT_TRACK_CARRIED : DH_FIT_TRACK_FITTED;
                    accepted = true;
                } else {
                    fit_track_reject(st);
                    rec.instance = a.start[slot];
                    rec.status = DH_FIT_TRACK_REJECTED | why;
                    free_it = !seen;
                }
            }
            rec.id = entry ? st.id : a.persons[(size_t)rig * DH_RIG_MAX_PERSONS + pi].id;   // (an unbound person is always seen)
            rec.age = st.age; rec.lost = st.lost;
            if (entry) {
                if (free_it) memset(&st, 0, sizeof st);
                a.state[slot] = st;
                // ---- the binding lifecycle (a freed entry is zeros: not tracked)
                SubjectBinding b = g.bound[slot];
                want = dh_subject_lifecycle(st.tracked != 0, accepted, g.max_tries, b.subject, b.wait, b.tries, b.bound_age);
                g.bound[slot] = b;
            }
        }
        g.records[slot].track = rec;
        g.records[slot].model = model;
        g.wants[slot] = want ? 1u : 0u;
    }
    // ---- the compact list: one atomic per wave (a workgroup is one wave)
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return;
    uint32_t base = 0;
    if (threadIdx.x == 0) base = atomicAdd(g.n_want, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, 0);
    if (want) g.want[base + (uint32_t)__popcll(mask & ((1ull << threadIdx.x) - 1ull))] = (uint32_t)slot;
}

template <bool STAGED>
__global__ __launch_bounds__(DH_FIT_THREADS) void k_rig_subject_score(const RigSubjectArgs g) {
    __shared__ float s_pts[STAGED ? 6 * DH_FIT_LDS_POINTS : 1];
    __shared__ unsigned long long s_sum[32];
    const IdentViewsArgs &q = g.q;
    const uint32_t S = q.n_subjects, n = q.f.n_inst;
    const uint32_t listed = *g.n_want;
    const size_t total = (size_t)(listed < n ? listed : n) * S;          // <= slots * S <= DH_IDENT_MAX_PAIRS
    for (size_t pair = blockIdx.x; pair < total; pair += gridDim.x) {    // (uniform over the workgroup)
        const uint32_t e = (uint32_t)(pair / S), sj = (uint32_t)(pair - (size_t)e * S);
        const uint32_t i = g.want[e];
        if (i < n) {                                                     // (always: the update kernel wrote a slot)
            const size_t at = (size_t)i * S + sj;
            const dh_view_instance *in = q.f.inst + i;
            uint32_t set;                                                // (0 where the instance takes part: n_sets is 1)
            if (q.enrolled[sj] == 0 || !ident_views_takes_part(q, in, i, &set)) {
                if (threadIdx.x == 0) {
                    dh_view_fit_record rec;
                    rec.points = 0; rec.steps = 0; rec.status = 0; rec.reserved = 0; rec.sum_r2_fixed = 0; rec.views_used = 0;
                    q.score[at] = rec;
                }
            } else {
                const SubjectModel sm = q.models[sj];
                const FitModel m{sm.pts, sm.nrm, q.np, 0};
                if (STAGED)                                              // (the launcher's: np <= DH_FIT_LDS_POINTS)
                    for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {
                        const uint32_t p = k / 3, c = k - p * 3;
                        s_pts[c * DH_FIT_LDS_POINTS + p] = m.pts[k];
                        s_pts[(3 + c) * DH_FIT_LDS_POINTS + p] = m.nrm[k];
                    }
                ident_views_run<STAGED>(q, q.f, in, m, s_pts, s_sum, at);
            }
        }
        __syncthreads();                                                 // the trip's last reads of s_pts and s_sum are done
    }
}

__global__ __launch_bounds__(DH_IDENT_THREADS) void k_rig_subject_bind(const RigSubjectArgs g) {
    const IdentViewsArgs &q = g.q;
    const uint32_t i = blockIdx.x;
    dh_rig_subject_record *out = g.records + i;
    if (g.wants[i] == 0) {                               // uniform over the wave
        if (threadIdx.x != 0) return;
        out->ident = ident_skipped();
        out->subject = g.bound[i].subject; out->identified = 0; out->tries = g.bound[i].tries;
        return;
    }
    const dh_view_instance *in = q.f.inst + i;
    uint32_t set;
    const bool part = ident_views_takes_part(q, in, i, &set);            // uniform over the wave
    const dh_ident_record rec = ident_decide(q.score + (size_t)i * q.n_subjects, q.n_subjects, q.f.min_points, part, q.max_ms, q.min_ratio);
    if (threadIdx.x != 0) return;
    SubjectBinding b = g.bound[i];                       // (a slot on the list is an unbound entry)
    dh_subject_bind_or_retry(rec.status, rec.best, g.retry, b.subject, b.wait, b.tries, b.bound_age);
    g.bound[i] = b;
    out->ident = rec;
    out->subject = b.subject; out->identified = 1; out->tries = b.tries;
}

__global__ __launch_bounds__(DH_RIG_FIT_THREADS) void k_rig_subject_set(const dh_rig_fit_state *state, SubjectBinding *bound, int rig, uint32_t id,
                                                                       uint32_t subject) {
    const int lane = threadIdx.x;
    const size_t slot = (size_t)rig * DH_RIG_MAX_TRACKS + lane;
    if (lane >= DH_RIG_MAX_TRACKS || state[slot].id != id) return;       // (id != 0; an id is held by one entry at most)
    bound[slot] = SubjectBinding{subject, 0u, 0u, 0u};
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_rig_subject_seed(const RigSubjectArgs &g, hipStream_t s) {
    if (g.a.n_rigs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rig_subject_seed, dim3(g.a.n_rigs), dim3(DH_RIG_FIT_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_rig_subject_update(const RigSubjectArgs &g, hipStream_t s) {
    if (g.a.n_rigs <= 0) return hipSuccess;
    const int slots = g.a.n_rigs * DH_RIG_MAX_TRACKS;
    hipLaunchKernelGGL(k_rig_subject_update, dim3((slots + DH_RIG_FIT_THREADS - 1) / DH_RIG_FIT_THREADS), dim3(DH_RIG_FIT_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_rig_subject_score(const RigSubjectArgs &g, hipStream_t s) {
    if (g.a.n_rigs <= 0 || g.grid == 0) return hipSuccess;
    if (g.q.np <= DH_FIT_LDS_POINTS) hipLaunchKernelGGL(k_rig_subject_score<true>, dim3(g.grid), dim3(DH_FIT_THREADS), 0, s, g);
    else hipLaunchKernelGGL(k_rig_subject_score<false>, dim3(g.grid), dim3(DH_FIT_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_rig_subject_bind(const RigSubjectArgs &g, hipStream_t s) {
    if (g.a.n_rigs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rig_subject_bind, dim3(g.a.n_rigs * DH_RIG_MAX_TRACKS), dim3(DH_IDENT_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_rig_subject_set(const dh_rig_fit_state *state, SubjectBinding *bound, int rig, uint32_t id, uint32_t subject, hipStream_t s) {
    hipLaunchKernelGGL(k_rig_subject_set, dim3(1), dim3(DH_RIG_FIT_THREADS), 0, s, state, bound, rig, id, subject);
    return hipGetLastError();
}
