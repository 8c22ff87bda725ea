// k_subject_track.hip -- each tracked head followed with its own subject's model (the rule is stated in
// include/depthhead_hip.h, section "following each tracked head with its own subject's model").  Four kernels around k_fit's
// per-instance-schedule instance (k_fit.hip), which fits over a table of the set's S models and the generic one at index S:
//   k_subject_track_seed    one lane per camera: section 19's steps 0 - 2 with the start's mesh -- the camera's subject where it
//                           is bound, else S -- and the step's want count cleared;
//   k_subject_track_update  one lane per camera: section 19's steps 4 - 6 on the first 76 bytes of the state, the binding
//                           lifecycle, and the cameras that want identification appended to a compact list: a ballot over the
//                           wave, one integer atomic per wave for the wave's share of the list, each wanting lane at its rank.
//                           The list's order is the atomics' and so free; wants[c] says the same per camera, and every output
//                           of the step is indexed by camera;
//   k_subject_track_score   the hot path: a fixed grid of workgroups of DH_FIT_THREADS lanes, each looping over the pairs
//                           (list entry, subject) of this step with the subject the fast index, so that the workgroups of one
//                           camera run together.  A trip is k_ident_score's body: ident_takes_part and ident_run
//                           (dh_fit_device.h) on the camera's fitted instance, the score and the pose written at [camera][subject]
//                           of the tracker's scratch.  The trip count depends on blockIdx and the list's length alone, so it
//                           is uniform over the workgroup; a barrier closes every trip before the next one stages its model
//                           over the LDS the last pass read;
//   k_subject_track_bind    one wave per camera: for a camera on the list the decision (ident_decide, dh_fit_device.h), then the
//                           binding (dh_subject_bind_or_retry, dh_fit.h) and the record's identification half by lane 0; for
//                           every other camera lane 0 writes the SKIPPED record.
// f32 and f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free; one
// integer atomic per wave: bit-identical run to run and to tests/subject_track_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_subject_track_seed(const SubjectTrackArgs g) {
    const FitTrackArgs &a = g.a;
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    if (c == 0) *g.n_want = 0;
    if (c >= a.n) return;
    const dh_subject_track_state &ss = g.state[c];
    const dh_fit_track_state &st = ss.fit;
    const uint32_t S = g.q.n_subjects;
    dh_render_instance in;
    in.frame = (uint32_t)c; in.mesh = ss.subject < S ? ss.subject : S; in.scale = a.scale; in.flags = 0;
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

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_subject_track_update(const SubjectTrackArgs g) {
    const FitTrackArgs &a = g.a;
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    bool want = false;                                   // (a lane past the cameras stays for the ballot)
    if (c < a.n) {
        const uint32_t seed = a.seed[c], kind = seed & 0xffu;
        dh_subject_track_state ss = g.state[c];
        dh_fit_track_state &st = ss.fit;
        dh_fit_track_record rec;
        rec.reserved = 0;
        uint32_t model = DH_IDENT_UNKNOWN;
        bool accepted = false;
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
            if (fit.mesh < g.q.n_subjects) model = fit.mesh;      // (the fit copies the start's mesh through)
            if (why == 0) {
                DH_FIT_TRACK_ACCEPT(st, fit);
                rec.instance = fit;
                rec.status = kind == DH_FIT_SEED_CARRIED ? DH_FIT_TRACK_CARRIED : DH_FIT_TRACK_FITTED;
                accepted = true;
            } else {
                fit_track_reject(st);
                rec.instance = a.start[c];
                rec.status = DH_FIT_TRACK_REJECTED | why;
            }
        }
        rec.age = st.age; rec.lost = st.lost;
        // ---- the binding lifecycle
        want = dh_subject_lifecycle(st.tracked != 0, accepted, g.max_tries, ss.subject, ss.wait, ss.tries, ss.bound_age);
        g.state[c] = ss;
        g.records[c].track = rec;
        g.records[c].model = model;
        g.wants[c] = want ? 1u : 0u;
    }
    // ---- the compact list: one atomic per wave (a workgroup is one wave)
    const unsigned long long mask = __ballot(want);
    if (mask == 0) return;
    uint32_t base = 0;
    if (threadIdx.x == 0) base = atomicAdd(g.n_want, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, 0);
    if (want) g.want[base + (uint32_t)__popcll(mask & ((1ull << threadIdx.x) - 1ull))] = (uint32_t)c;
}

__global__ __launch_bounds__(DH_FIT_THREADS) void k_subject_track_score(const SubjectTrackArgs g) {
    __shared__ float s_pts[6 * DH_FIT_LDS_POINTS];
    __shared__ unsigned long long s_sum[32];
    const IdentArgs &q = g.q;
    const uint32_t S = q.n_subjects, n = q.f.n_inst;
    const uint32_t listed = *g.n_want;
    const size_t total = (size_t)(listed < n ? listed : n) * S;          // <= cameras * S <= DH_IDENT_MAX_PAIRS
    for (size_t pair = blockIdx.x; pair < total; pair += gridDim.x) {    // (uniform over the workgroup)
        const uint32_t e = (uint32_t)(pair / S), sj = (uint32_t)(pair - (size_t)e * S);
        const uint32_t i = g.want[e];
        if (i < n) {                                                     // (always: the update kernel wrote a camera)
            const size_t at = (size_t)i * S + sj;
            const dh_render_instance *in = q.f.inst + i;
            if (q.enrolled[sj] == 0 || !ident_takes_part(q, in, i)) {
                if (threadIdx.x == 0) {
                    dh_fit_record rec;
                    rec.points = 0; rec.steps = 0; rec.status = 0; rec.reserved = 0; rec.sum_r2_fixed = 0;
                    q.score[at] = rec;
                }
            } else {
                const SubjectModel sm = q.models[sj];
                const FitModel m{sm.pts, sm.nrm, q.np, 0};
                if (m.n <= DH_FIT_LDS_POINTS) {
                    for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {
                        const uint32_t p = k / 3, c = k - p * 3;
                        s_pts[c * DH_FIT_LDS_POINTS + p] = m.pts[k];
                        s_pts[(3 + c) * DH_FIT_LDS_POINTS + p] = m.nrm[k];
                    }
                    ident_run<true>(q, in, m, s_pts, s_sum, at);
                } else ident_run<false>(q, in, m, s_pts, s_sum, at);
            }
        }
        __syncthreads();                                                 // the trip's last reads of s_pts and s_sum are done
    }
}

__global__ __launch_bounds__(DH_IDENT_THREADS) void k_subject_track_bind(const SubjectTrackArgs g) {
    const IdentArgs &q = g.q;
    const uint32_t i = blockIdx.x;
    dh_subject_track_record *out = g.records + i;
    if (g.wants[i] == 0) {                               // uniform over the wave
        if (threadIdx.x != 0) return;
        out->ident = ident_skipped();
        out->subject = g.state[i].subject; out->identified = 0; out->tries = g.state[i].tries;
        return;
    }
    const dh_render_instance *in = q.f.inst + i;
    const bool part = ident_takes_part(q, in, i);        // uniform over the wave
    const dh_ident_record rec = ident_decide(q.score + (size_t)i * q.n_subjects, q.n_subjects, q.f.min_points, part, q.max_ms, q.min_ratio);
    if (threadIdx.x != 0) return;
    dh_subject_track_state *ss = g.state + i;            // (a camera on the list is unbound)
    SubjectBinding b{ss->subject, ss->wait, ss->tries, ss->bound_age};
    dh_subject_bind_or_retry(rec.status, rec.best, g.retry, b.subject, b.wait, b.tries, b.bound_age);
    ss->subject = b.subject; ss->wait = b.wait; ss->tries = b.tries; ss->bound_age = b.bound_age;
    out->ident = rec;
    out->subject = b.subject; out->identified = 1; out->tries = b.tries;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_subject_track_seed(const SubjectTrackArgs &g, hipStream_t s) {
    if (g.a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_subject_track_seed, dim3((g.a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_subject_track_update(const SubjectTrackArgs &g, hipStream_t s) {
    if (g.a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_subject_track_update, dim3((g.a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_subject_track_score(const SubjectTrackArgs &g, hipStream_t s) {
    if (g.a.n <= 0 || g.grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_subject_track_score, dim3(g.grid), dim3(DH_FIT_THREADS), 0, s, g);
    return hipGetLastError();
}
hipError_t dh_launch_subject_track_bind(const SubjectTrackArgs &g, hipStream_t s) {
    if (g.a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_subject_track_bind, dim3(g.a.n), dim3(DH_IDENT_THREADS), 0, s, g);
    return hipGetLastError();
}
