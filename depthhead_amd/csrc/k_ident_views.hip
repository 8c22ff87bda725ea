// k_ident_views.hip -- which enrolled subject a rig's fitted head belongs to, decided from all the cameras that see it (DESIGN.md
// section 28; the rule is stated in include/depthhead_hip.h, section "identifying enrolled subjects across the views of a rig").
// k_ident.hip's two kernels with section 21's pass in place of section 18's:
//   k_ident_views_score   one workgroup of DH_FIT_THREADS lanes per (instance, subject) pair, the subject the fast index of the
//                         grid.  A pair whose subject is no candidate or whose instance takes no part (dh_ident_views_part, dh_fit.h;
//                         uniform over the workgroup) writes a score of zeros and leaves before anything is staged.  Otherwise
//                         the subject's model is staged into LDS up to DH_FIT_LDS_POINTS and streamed above, and the pair runs
//                         the full steps of k_fit_views' schedule (no coarse ones) and the last pass -- fit_views_pass<FIT_FULL>,
//                         fit_solve_tri<6, 6>, fit_cayley, fit_small, fit_views_pass<FIT_LAST>, all dh_fit_device.h's -- over the
//                         frames of the instance's set: the pass gets a copy of the FitViewsArgs whose `frames` is advanced by
//                         set * n * h * w and is itself what k_fit_views runs.  Lane 0 writes the pair's dh_view_fit_record and
//                         its world pose rounded to f32.
//   k_ident_views_decide  one wave per instance over its row of 32-byte scores: ident_decide (dh_fit_device.h: the strided picks and
//                         the shuffle reduction every deciding kernel runs) with dh_fit.h's __host__ __device__ order and status
//                         (tests/host/ident_check.cpp compiles them as they are); lane 0 writes subjects_out, the record and
//                         poses_out, a dh_view_instance.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/ident_views_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

// (ident_views_takes_part and ident_views_run, one pair's refit, are dh_fit_device.h's: k_rig_subject_track.hip runs them over its
// compact list)
__global__ __launch_bounds__(DH_FIT_THREADS) void k_ident_views_score(const IdentViewsArgs q) {
    __shared__ float s_pts[6 * DH_FIT_LDS_POINTS];
    __shared__ unsigned long long s_sum[32];
    const size_t pair = blockIdx.x;                  // < n_inst * n_subjects <= DH_IDENT_MAX_PAIRS
    const uint32_t i = (uint32_t)(pair / q.n_subjects), sj = (uint32_t)(pair - (size_t)i * q.n_subjects);
    const dh_view_instance *in = q.f.inst + i;
    uint32_t set;
    if ((q.enrolled && q.enrolled[sj] == 0) || !ident_views_takes_part(q, in, i, &set)) {
        if (threadIdx.x == 0) {
            dh_view_fit_record rec;
            rec.points = 0; rec.steps = 0; rec.status = 0; rec.reserved = 0; rec.sum_r2_fixed = 0; rec.views_used = 0;
            q.score[pair] = rec;
        }
        return;
    }
    FitViewsArgs a = q.f;
    a.frames = q.f.frames + ((size_t)set * (size_t)a.n) * ((size_t)a.h * (size_t)a.w);     // set < n_sets: inside the call's frames
    const SubjectModel sm = q.models[sj];
    const FitModel m{sm.pts, sm.nrm, q.np, 0};
    if (m.n <= DH_FIT_LDS_POINTS) {
        for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {
            const uint32_t p = k / 3, c = k - p * 3;
            s_pts[c * DH_FIT_LDS_POINTS + p] = m.pts[k];
            s_pts[(3 + c) * DH_FIT_LDS_POINTS + p] = m.nrm[k];
        }
        ident_views_run<true>(q, a, in, m, s_pts, s_sum, pair);
    } else ident_views_run<false>(q, a, in, m, s_pts, s_sum, pair);
}

__global__ __launch_bounds__(DH_IDENT_THREADS) void k_ident_views_decide(const IdentViewsArgs q) {
    const uint32_t i = blockIdx.x;
    const dh_view_instance *in = q.f.inst + i;
    uint32_t set;
    const bool part = ident_views_takes_part(q, in, i, &set);    // uniform over the wave
    const dh_ident_record rec = ident_decide(q.score + (size_t)i * q.n_subjects, q.n_subjects, q.f.min_points, part, q.max_ms, q.min_ratio);
    if (threadIdx.x != 0) return;
    q.rec[i] = rec;
    q.subjects_out[i] = rec.status == DH_IDENT_OK ? rec.best : DH_IDENT_UNKNOWN;
    if (q.poses_out) {
        dh_view_instance o = *in;
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
hipError_t dh_launch_ident_views_score(const IdentViewsArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ident_views_score, dim3(a.f.n_inst * a.n_subjects), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_ident_views_decide(const IdentViewsArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ident_views_decide, dim3(a.f.n_inst), dim3(DH_IDENT_THREADS), 0, s, a);
    return hipGetLastError();
}
