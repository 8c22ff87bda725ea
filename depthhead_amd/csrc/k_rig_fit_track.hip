// k_rig_fit_track.hip -- each rig person's fitted world pose carried across steps (the rule is stated in
// include/depthhead_hip.h, section "carrying each rig person's fitted world pose across steps").  Two small kernels around
// k_fit_views' per-instance-schedule instance (k_fit_views.hip), over the DH_RIG_MAX_TRACKS slots of every rig:
//   k_rig_fit_seed    steps 0 - 2, one workgroup of 64 lanes per rig: the rig's entries and persons are copied to LDS, lane 0
//                     binds persons to entries (dh_rig_fit_bind, dh_rig_fit.h: sequential, 16 x 16 at most), then one lane
//                     per slot composes the slot's start instance, its schedule and its kind;
//   k_rig_fit_update  steps 4 - 6, one lane per slot: acceptance, the entry's state and the slot's record.
// f32 and f64 with + - * /, compares and casts only, every operation rounded on its own; the cosines and sines come from the
// host's 120-entry table (section 19's).  Bit-identical to tests/rig_fit_track_ref.py.  The pieces of the rule that are the
// camera tracker's (k_fit_track.hip) -- the table rotation, the carried start, acceptance, the jump test and the state updates --
// are dh_fit_device.h's; what is here is the bind, the views and the slots.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

static_assert(DH_RIG_MAX_TRACKS <= DH_RIG_FIT_THREADS, "one lane per slot of a rig");
static_assert(sizeof(dh_rig_fit_state) % 4 == 0 && sizeof(dh_rig_person) % 4 == 0, "copied to LDS word by word");

// (the seed of a rig, rig_fit_seed_rig, is dh_fit_device.h's: k_rig_subject_seed runs it with a model word per entry)
__global__ __launch_bounds__(DH_RIG_FIT_THREADS) void k_rig_fit_seed(const RigFitArgs a) {
    __shared__ dh_rig_fit_state s_st[DH_RIG_MAX_TRACKS];
    __shared__ dh_rig_person s_p[DH_RIG_MAX_PERSONS];
    __shared__ uint32_t s_role[DH_RIG_MAX_TRACKS], s_who[DH_RIG_MAX_TRACKS];
    rig_fit_seed_rig(a, s_st, s_p, s_role, s_who, [](size_t, const dh_rig_fit_state *, const dh_rig_fit_state &, uint32_t) { return 0u; });
}

__global__ __launch_bounds__(DH_RIG_FIT_THREADS) void k_rig_fit_update(const RigFitArgs a) {
    const int slot = blockIdx.x * DH_RIG_FIT_THREADS + threadIdx.x;
    if (slot >= a.n_rigs * DH_RIG_MAX_TRACKS) return;
    const int g = slot / DH_RIG_MAX_TRACKS;
    const uint32_t seed = a.seed[slot], kind = seed & 0xffu, pi = a.who[slot];
    const bool seen = (seed & DH_RIG_FIT_SEED_IS_SEEN) != 0, entry = (seed & DH_RIG_FIT_SEED_IS_ENTRY) != 0;
    dh_rig_fit_record rec;
    memset(&rec, 0, sizeof rec);
    if (kind == DH_FIT_SEED_NONE || kind == DH_FIT_SEED_ABSENT) {
        if (kind == DH_FIT_SEED_ABSENT) rec.status = DH_FIT_TRACK_ABSENT;
        a.records[slot] = rec;
        return;
    }
    dh_rig_fit_state st;
    memset(&st, 0, sizeof st);
    if (entry) st = a.state[slot];
    bool free_it = false;
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
        if (seen) why |= fit_track_jump(fit.t, a.persons[(size_t)g * DH_RIG_MAX_PERSONS + pi].world, a.jump2);
        rec.fit = fr;
        if (why == 0) {
            DH_FIT_TRACK_ACCEPT(st, fit);
            st.views_used = fr.views_used;
            rec.instance = fit;
            rec.status = kind == DH_FIT_SEED_CARRIED ? DH_FIT_TRACK_CARRIED : DH_FIT_TRACK_FITTED;
        } else {
            fit_track_reject(st);
            rec.instance = a.start[slot];
            rec.status = DH_FIT_TRACK_REJECTED | why;
            free_it = !seen;
        }
    }
    rec.id = entry ? st.id : a.persons[(size_t)g * DH_RIG_MAX_PERSONS + pi].id;   // (an unbound person is always seen)
    rec.age = st.age; rec.lost = st.lost;
    if (entry) {
        if (free_it) memset(&st, 0, sizeof st);
        a.state[slot] = st;
    }
    a.records[slot] = rec;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_rig_fit_seed(const RigFitArgs &a, hipStream_t s) {
    if (a.n_rigs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rig_fit_seed, dim3(a.n_rigs), dim3(DH_RIG_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_rig_fit_update(const RigFitArgs &a, hipStream_t s) {
    if (a.n_rigs <= 0) return hipSuccess;
    const int slots = a.n_rigs * DH_RIG_MAX_TRACKS;
    hipLaunchKernelGGL(k_rig_fit_update, dim3((slots + DH_RIG_FIT_THREADS - 1) / DH_RIG_FIT_THREADS), dim3(DH_RIG_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
