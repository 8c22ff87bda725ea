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
//   k_ident_views_decide  one wave per instance over its row of 32-byte scores: k_ident_decide's strided picks and shuffle
//                         reduction with dh_fit.h's __host__ __device__ order and status (tests/host/ident_check.cpp compiles them
//                         as they are); lane 0 writes subjects_out, the record and poses_out, a dh_view_instance.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/ident_views_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

// Whether instance `in` (number i) takes part, and in *set the set its frames are in (< n_sets where it does).
__device__ __forceinline__ bool ident_views_takes_part(const IdentViewsArgs &q, const dh_view_instance *in, uint32_t i, uint32_t *set) {
    *set = q.sets ? q.sets[i] : 0u;
    return dh_ident_views_part(*in, *set, q.fit_rec ? q.fit_rec + i : nullptr, (uint32_t)q.f.n, q.n_sets, q.np, q.radius, q.largest).why ==
           DH_IDENT_VIEWS_OK;
}

// One pair's refit over the views of its instance: the full steps, then the last pass; the score and the pose written by lane 0.
// a: the call's FitViewsArgs with the frames of the instance's set.
template <bool STAGED>
__device__ __forceinline__ void ident_views_run(const IdentViewsArgs &q, const FitViewsArgs &a, const dh_view_instance *in, const FitModel &m,
                                                const float *s_pts, unsigned long long *s_sum, size_t pair) {
    const uint32_t first_cam = in->first_cam;
    const uint64_t views = in->views;
    const uint64_t mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(views >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)views);
    FitPose pose;
#pragma unroll
    for (int c = 0; c < 9; ++c) pose.R[c] = (double)in->R[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) pose.t[c] = (double)in->t[c];
    const double scale = (double)in->scale;
    uint32_t steps = 0, status = DH_FIT_OK;
    for (uint32_t it = 0; it < a.full; ++it) {
        fit_views_pass<FIT_FULL, STAGED>(a, m, s_pts, first_cam, mask, scale, pose, a.gate[1], s_sum);
        if ((uint32_t)s_sum[DH_FIT_COUNT] < a.min_points) { status = DH_FIT_FEW_POINTS; break; }
        double x[6];
        if (!fit_solve_tri<6, 6>(s_sum, DH_FIT_B, a.lam1, x)) { status = DH_FIT_SINGULAR; break; }
#pragma unroll
        for (int j = 0; j < 3; ++j) pose.t[j] = pose.t[j] + x[j];
        fit_cayley(pose.R, x + 3);
        ++steps;
        if (fit_small(x, 6)) break;
    }
    fit_views_pass<FIT_LAST, STAGED>(a, m, s_pts, first_cam, mask, scale, pose, a.gate[1], s_sum);
    if (threadIdx.x == 0) {
        dh_view_fit_record rec;
        rec.points = (uint32_t)s_sum[DH_FIT_COUNT];
        rec.steps = steps;
        rec.status = status;
        rec.reserved = 0;
        rec.sum_r2_fixed = (int64_t)s_sum[DH_FIT_E];
        rec.views_used = (uint64_t)s_sum[DH_FIT_USED];
        q.score[pair] = rec;
        float *o = q.pose + pair * 12;
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = (float)pose.R[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[9 + c] = (float)pose.t[c];
    }
}

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
    const dh_view_fit_record *row = q.score + (size_t)i * q.n_subjects;
    IdentPick pick = dh_ident_pick_none();
    uint32_t eligible = 0;
    if (part)
        for (uint32_t sj = threadIdx.x; sj < q.n_subjects; sj += DH_IDENT_THREADS) {
            const dh_view_fit_record r = row[sj];    // a pair that did not run holds zeros: 0 points, never eligible
            if (r.status != DH_FIT_OK || r.points < q.f.min_points) continue;
            dh_ident_pick_add(pick, dh_ident_mean(r.sum_r2_fixed, r.points), sj);
            ++eligible;
        }
#pragma unroll
    for (int o = WAVE / 2; o; o >>= 1) {
        IdentPick other;
        other.m_best = shfl_xor_f64(pick.m_best, o);
        other.m_second = shfl_xor_f64(pick.m_second, o);
        other.best = (uint32_t)__shfl_xor((int)pick.best, o);
        other.second = (uint32_t)__shfl_xor((int)pick.second, o);
        dh_ident_pick_merge(pick, other);
        eligible += (uint32_t)__shfl_xor((int)eligible, o);
    }
    if (threadIdx.x != 0) return;
    dh_ident_record rec;
    rec.status = part ? dh_ident_status(eligible, pick.m_best, pick.m_second, q.max_ms, q.min_ratio) : DH_IDENT_SKIPPED;
    rec.best = pick.best; rec.second = pick.second;
    rec.eligible = eligible;
    rec.points_best = 0; rec.points_second = 0; rec.sum_r2_best = 0; rec.sum_r2_second = 0;
    if (pick.best != DH_IDENT_UNKNOWN) { rec.points_best = row[pick.best].points; rec.sum_r2_best = row[pick.best].sum_r2_fixed; }
    if (pick.second != DH_IDENT_UNKNOWN) { rec.points_second = row[pick.second].points; rec.sum_r2_second = row[pick.second].sum_r2_fixed; }
    q.rec[i] = rec;
    q.subjects_out[i] = rec.status == DH_IDENT_OK ? pick.best : DH_IDENT_UNKNOWN;
    if (q.poses_out) {
        dh_view_instance o = *in;
        if (pick.best != DH_IDENT_UNKNOWN) {
            const float *p = q.pose + ((size_t)i * q.n_subjects + pick.best) * 12;
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
