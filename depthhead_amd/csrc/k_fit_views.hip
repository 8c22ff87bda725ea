// k_fit_views.hip -- one posed model fitted to the depth frames of several cameras at once (the rule is
// stated in include/depthhead_hip.h, section "fitting one model to several views").  k_fit's structure with one loop more: one
// workgroup of 256 lanes per instance runs the whole schedule -- every pass, every step, the last pass -- inside one launch, and
// a pass walks the instance's views (outer loop, uniform over the workgroup) and for each view the model's points (inner loop).
//   view   every lane composes the view's camera pose (R_v, t_v) = (V R_w, V t_w + u) from the world pose it carries, once per
//          view and pass; the composite, V and K are the same in every lane and are moved to scalar registers (uni), so the
//          point loop holds no more vector registers than k_fit's;
//   point  DH_FIT_CORRESPOND as it stands at (scale, R_v, t_v, K_c, frame c); the row of a point that passed is turned back
//          into the world frame, J = (V^T n, V^T m), and its products go to the lane's int64 partial sums, which run on over
//          the views; one wave reduction and one LDS atomic per wave and sum finish a pass, as in k_fit;
//   step   every lane solves the same system redundantly in f64 (fit_solve_tri) and carries the world pose in registers.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/view_fit_ref.py.  With one view, V = I and u = 0 every sum equals k_fit's.  One kernel body,
// FIT_VIEWS_BLOCK, in two instances: k_fit_views, and k_fit_views_sched with a schedule per instance.
// The pose (FitPose), the modes of a pass and the step's helpers (fit_small, fit_cayley) are k_fit's very ones, in dh_fit_device.h;
// uni() is there too (k_shape_accumulate_views moves its composite to scalar registers with it), and so is the pass itself,
// fit_views_pass, which k_ident_views.hip runs as well.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

template <bool STAGED>
__device__ __forceinline__ void fit_views_run(const FitViewsArgs &a, uint32_t b, const dh_view_instance *in, const FitModel &m,
                                              const float *s_pts, unsigned long long *s_sum) {
    const uint32_t first_cam = in->first_cam;
    const uint64_t views = in->views;
    const uint64_t mask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(views >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)views);
    FitPose pose;
#pragma unroll
    for (int q = 0; q < 9; ++q) pose.R[q] = (double)in->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) pose.t[q] = (double)in->t[q];
    const double scale = (double)in->scale;
    uint32_t steps = 0, status = DH_FIT_OK;
    bool stop = false;
    for (uint32_t it = 0; it < a.coarse; ++it) {
        fit_views_pass<FIT_COARSE, STAGED>(a, m, s_pts, first_cam, mask, scale, pose, a.gate[0], s_sum);
        if ((uint32_t)s_sum[DH_FIT_COUNT] < a.min_points) { status = DH_FIT_FEW_POINTS; stop = true; break; }
        double x[6] = {0, 0, 0, 0, 0, 0};
        if (!fit_solve_tri<3, 6>(s_sum, DH_FIT_B, a.lam1, x)) { status = DH_FIT_SINGULAR; stop = true; break; }
#pragma unroll
        for (int j = 0; j < 3; ++j) pose.t[j] = pose.t[j] + x[j];
        ++steps;
        if (fit_small(x, 3)) break;
    }
    for (uint32_t it = 0; it < a.full && !stop; ++it) {
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
        dh_view_instance o = *in;
#pragma unroll
        for (int q = 0; q < 9; ++q) o.R[q] = (float)pose.R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) o.t[q] = (float)pose.t[q];
        a.out[b] = o;
        dh_view_fit_record rec;
        rec.points = (uint32_t)s_sum[DH_FIT_COUNT];
        rec.steps = steps;
        rec.status = status;
        rec.reserved = 0;
        rec.sum_r2_fixed = (int64_t)s_sum[DH_FIT_E];
        rec.views_used = (uint64_t)s_sum[DH_FIT_USED];
        a.rec[b] = rec;
    }
}

// One instance's whole fit, the body of both kernels: the model staged into LDS where it fits (the first pass's barriers order
// the staging before its reads), then the schedule of `a` over the instance's views.  A macro, as FIT_BLOCK is in k_fit.hip: both
// kernels compile from the very tokens, and the __shared__ arrays are each kernel's own.  b: the instance of this workgroup.
#define FIT_VIEWS_BLOCK(a, b)                                                                                                    \
    __shared__ float s_pts[6 * DH_FIT_LDS_POINTS];                                                                             \
    __shared__ unsigned long long s_sum[32];                                                                                   \
    const dh_view_instance *in = (a).inst + (b);                                                                              \
    const FitModel m = (a).models[in->model];                                                                                  \
    if (m.n <= DH_FIT_LDS_POINTS) {                                                                                            \
        for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {                                                     \
            const uint32_t i = k / 3, c = k - i * 3;                                                                           \
            s_pts[c * DH_FIT_LDS_POINTS + i] = m.pts[k];                                                                       \
            s_pts[(3 + c) * DH_FIT_LDS_POINTS + i] = m.nrm[k];                                                                 \
        }                                                                                                                      \
        fit_views_run<true>(a, b, in, m, s_pts, s_sum);                                                                        \
    } else fit_views_run<false>(a, b, in, m, s_pts, s_sum)

__global__ __launch_bounds__(DH_FIT_THREADS) void k_fit_views(const FitViewsArgs a) { FIT_VIEWS_BLOCK(a, blockIdx.x); }

// The per-instance-schedule instance (dh_rig_fit_tracker_step*): slot b runs (sched[b][0], sched[b][1]); a workgroup whose slot
// has no start (uniform over the workgroup: one word read by every lane) leaves before the model is staged and writes nothing.
// The slots come in groups of `group` (a rig's) of which the first ones are the busy ones, and workgroups are dealt to the
// XCDs round-robin by blockIdx: workgroup w takes slot (w mod G) * group + w / G of the G = n_inst / group groups, so that
// the first slots of all groups are consecutive workgroups and spread over the XCDs (w -> slot w put them all on one XCD
// when `group` is a multiple of the XCD count, and the step took as long as twenty steps).  n_inst is a multiple of group.
__global__ __launch_bounds__(DH_FIT_THREADS) void k_fit_views_sched(const FitViewsSchedArgs q) {
    const uint32_t groups = q.f.n_inst / q.group;
    const uint32_t b = (blockIdx.x % groups) * q.group + blockIdx.x / groups;      // < n_inst: blockIdx.x / groups < group
    if (dh_fit_seed_no_start(q.seed[b])) return;
    FitViewsArgs a = q.f;
    a.coarse = q.sched[2 * b]; a.full = q.sched[2 * b + 1];
    FIT_VIEWS_BLOCK(a, b);
}

// ------------------------------------------------------------------ launcher
hipError_t dh_launch_fit_views(const FitViewsArgs &a, hipStream_t s) {
    if (a.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_views, dim3(a.n_inst), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_fit_views_sched(const FitViewsSchedArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0 || a.group == 0 || a.f.n_inst % a.group != 0) return a.f.n_inst == 0 ? hipSuccess : hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fit_views_sched, dim3(a.f.n_inst), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
