// k_fit_track.hip -- each camera's fitted pose carried across steps (the rule is stated in
// include/depthhead_hip.h, section "carrying each camera's fitted pose across steps").  Two kernels of one lane per camera around
// k_fit's per-instance-schedule instance (k_fit.hip):
//   k_fit_track_seed    steps 0 - 2: absent / detection valid / the start instance, its schedule and its kind;
//   k_fit_track_update  steps 4 - 6: acceptance, the camera's state and its record.
// f32 and f64 with + - * /, compares and casts only, every operation rounded on its own; the cosines and sines come from the
// host's 120-entry table.  Bit-identical to tests/fit_track_ref.py.  The rule's pieces that the rig tracker (k_rig_fit_track.hip)
// applies too -- the table rotation, the carried start, acceptance, the jump test and the state updates -- are dh_fit_device.h's.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_fit_track_seed(const FitTrackArgs a) {
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    if (c >= a.n) return;
    dh_render_instance in;
    in.frame = (uint32_t)c; in.mesh = 0; in.scale = a.scale; in.flags = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) in.R[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < 3; ++q) in.t[q] = 0.0f;
    uint32_t kind = DH_FIT_SEED_NONE, coarse = 0, full = 0;
    if (a.present && a.present[c] == 0) kind = DH_FIT_SEED_ABSENT;
    else {
        const dh_support sp = a.support[c];
        // mass * conf_den >= total_mass * conf_num: the 96-bit products as (high, low) words
        const unsigned long long den = a.prm.conf_den, num = a.prm.conf_num;
        const unsigned long long lh = __umul64hi(sp.mass, den), ll = sp.mass * den;
        const unsigned long long rh = __umul64hi(sp.total_mass, num), rl = sp.total_mass * num;
        const bool valid = sp.total_mass > 0 && (lh > rh || (lh == rh && ll >= rl)) && sp.windows >= a.prm.min_windows;
        const dh_fit_track_state &st = a.state[c];
        if (st.tracked) {
            kind = DH_FIT_SEED_CARRIED;
            full = a.prm.iterations_tracked;
            fit_track_carried_start(st, a.flags, in);
        } else if (valid) {
            kind = DH_FIT_SEED_DETECTED;
            coarse = a.coarse; full = a.full;
            const dh_pose po = a.poses[c];
            double R[9];
            fit_track_rotation(po.rotation, a.angles, R);
#pragma unroll
            for (int q = 0; q < 9; ++q) in.R[q] = (float)R[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) in.t[q] = po.mid_point[q];
        }
        if (valid) kind |= DH_FIT_SEED_VALID;
    }
    a.start[c] = in;
    a.sched[2 * c] = coarse; a.sched[2 * c + 1] = full;
    a.seed[c] = kind;
}

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_fit_track_update(const FitTrackArgs a) {
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    if (c >= a.n) return;
    const uint32_t seed = a.seed[c], kind = seed & 0xffu;
    dh_fit_track_state st = a.state[c];
    dh_fit_track_record rec;
    rec.reserved = 0;
    if (kind == DH_FIT_SEED_ABSENT || kind == DH_FIT_SEED_NONE) {
        rec.instance.frame = 0; rec.instance.mesh = 0; rec.instance.scale = 0.0f; rec.instance.flags = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q) rec.instance.R[q] = 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) rec.instance.t[q] = 0.0f;
        rec.fit.points = 0; rec.fit.steps = 0; rec.fit.status = 0; rec.fit.reserved = 0; rec.fit.sum_r2_fixed = 0;
        st.lost = fit_sat_inc(st.lost);
        st.have_prev = 0;
        if (kind == DH_FIT_SEED_ABSENT) {
            if (st.lost > a.prm.max_coast) { st.tracked = 0; st.age = 0; }
            rec.status = DH_FIT_TRACK_ABSENT;
        } else {
            st.tracked = 0; st.age = 0;
            rec.status = DH_FIT_TRACK_NONE;
        }
    } else {
        const dh_render_instance fit = a.fit_out[c];
        const dh_fit_record fr = a.fit_rec[c];
        uint32_t why = fit_track_why(fr, a.prm.keep_points, a.rms_lim);
        if (seed & DH_FIT_SEED_VALID) why |= fit_track_jump(fit.t, a.poses[c].mid_point, a.jump2);
        rec.fit = fr;
        if (why == 0) {
            DH_FIT_TRACK_ACCEPT(st, fit);
            rec.instance = fit;
            rec.status = kind == DH_FIT_SEED_CARRIED ? DH_FIT_TRACK_CARRIED : DH_FIT_TRACK_FITTED;
        } else {
            fit_track_reject(st);
            rec.instance = a.start[c];
            rec.status = DH_FIT_TRACK_REJECTED | why;
        }
    }
    rec.age = st.age; rec.lost = st.lost;
    a.state[c] = st;
    a.records[c] = rec;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_fit_track_seed(const FitTrackArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_track_seed, dim3((a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_fit_track_update(const FitTrackArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_track_update, dim3((a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, a);
    return hipGetLastError();
}
