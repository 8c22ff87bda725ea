// k_ident.hip -- which enrolled subject a fitted head belongs to (the rule is stated in
// include/depthhead_hip.h, section "identifying the subject of a fitted head").  Two kernels:
//   k_ident_score   one workgroup of DH_FIT_THREADS lanes per (instance, subject) pair, the subject the fast index of the grid so
//                   that the workgroups of one instance run together and read the same few kilobytes of its frame from L2.  A
//                   pair whose subject is no candidate or whose instance takes no part (uniform over the workgroup) writes a
//                   score of zeros and leaves before anything is staged.  Otherwise the body is the fit's own: the subject's
//                   model staged into LDS up to DH_FIT_LDS_POINTS and streamed above, fit_pass<FIT_FULL> and fit_pass<FIT_LAST>
//                   (dh_fit_device.h, with DH_FIT_CORRESPOND), fit_solve_tri<6, 6> and fit_cayley, on the schedule of full steps
//                   alone; lane 0 writes the pair's dh_fit_record and its pose rounded to f32.
//   k_ident_decide  one wave per instance.  Lanes stride over the candidates, each keeps the best and the second (m, s) of its
//                   own (IdentPick, dh_fit.h), a shuffle reduction merges the picks under the lexicographic order, and lane 0
//                   writes subjects_out, the record and poses_out.  The order and the status are dh_fit.h's __host__ __device__
//                   functions, which tests/host/ident_check.cpp compiles as they are.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/ident_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

// (ident_takes_part and ident_run, one pair's refit, are dh_fit_device.h's: k_subject_track.hip runs them over its compact list)
__global__ __launch_bounds__(DH_FIT_THREADS) void k_ident_score(const IdentArgs q) {
    __shared__ float s_pts[6 * DH_FIT_LDS_POINTS];
    __shared__ unsigned long long s_sum[32];
    const size_t pair = blockIdx.x;                  // < n_inst * n_subjects <= DH_IDENT_MAX_PAIRS
    const uint32_t i = (uint32_t)(pair / q.n_subjects), sj = (uint32_t)(pair - (size_t)i * q.n_subjects);
    const dh_render_instance *in = q.f.inst + i;
    if ((q.enrolled && q.enrolled[sj] == 0) || !ident_takes_part(q, in, i)) {
        if (threadIdx.x == 0) {
            dh_fit_record rec;
            rec.points = 0; rec.steps = 0; rec.status = 0; rec.reserved = 0; rec.sum_r2_fixed = 0;
            q.score[pair] = rec;
        }
        return;
    }
    const SubjectModel sm = q.models[sj];
    const FitModel m{sm.pts, sm.nrm, q.np, 0};
    if (m.n <= DH_FIT_LDS_POINTS) {
        for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {
            const uint32_t p = k / 3, c = k - p * 3;
            s_pts[c * DH_FIT_LDS_POINTS + p] = m.pts[k];
            s_pts[(3 + c) * DH_FIT_LDS_POINTS + p] = m.nrm[k];
        }
        ident_run<true>(q, in, m, s_pts, s_sum, pair);
    } else ident_run<false>(q, in, m, s_pts, s_sum, pair);
}

// (the strided picks, the shuffle reduction and the record are ident_decide, dh_fit_device.h's, for every kernel that decides)
__global__ __launch_bounds__(DH_IDENT_THREADS) void k_ident_decide(const IdentArgs q) {
    const uint32_t i = blockIdx.x;
    const dh_render_instance *in = q.f.inst + i;
    const bool part = ident_takes_part(q, in, i);    // uniform over the wave
    const dh_ident_record rec = ident_decide(q.score + (size_t)i * q.n_subjects, q.n_subjects, q.f.min_points, part, q.max_ms, q.min_ratio);
    if (threadIdx.x != 0) return;
    q.rec[i] = rec;
    q.subjects_out[i] = rec.status == DH_IDENT_OK ? rec.best : DH_IDENT_UNKNOWN;
    if (q.poses_out) {
        dh_render_instance o = *in;
        if (rec.best != DH_IDENT_UNKNOWN) {
            const float *p = q.pose + ((size_t)i * q.n_subjects + rec.best) * 12;
#pragma unroll
            for (int c = 0; c < 9; ++c) o.R[c] = p[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) o.t[c] = p[9 + c];
        }
        q.poses_out[i] = o;
    }
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_ident_score(const IdentArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ident_score, dim3(a.f.n_inst * a.n_subjects), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_ident_decide(const IdentArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ident_decide, dim3(a.f.n_inst), dim3(DH_IDENT_THREADS), 0, s, a);
    return hipGetLastError();
}
