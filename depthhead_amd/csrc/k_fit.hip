// k_fit.hip -- posed point models fitted to depth frames: point-to-plane ICP with projective association (DESIGN.md section 18;
// the rule is stated in include/depthhead_hip.h, section "fitting posed models to depth frames").  One kernel body, DH_FIT_BLOCK,
// in two instances (k_fit, and k_fit_sched with a schedule per instance): one workgroup of 256 lanes per instance runs the whole
// schedule -- every pass, every step, the last pass -- inside one launch.
//   pass   each lane strides over the model's points (staged in LDS up to DH_FIT_LDS_POINTS, else streamed), finds each point's
//          correspondence (DH_FIT_CORRESPOND, dh_fit_device.h: transform, project, gather the depth pixel, gate, residual) and
//          adds the point's products to its int64 partial sums in registers; a coarse pass keeps only the 9 sums of the
//          translation block, the last pass only e; the sums are reduced across the wave with shuffles and one LDS atomic per
//          wave and sum finishes them;
//   step   after a barrier every lane solves the same system redundantly in f64 (fit_solve_tri, dh_fit_device.h: deterministic,
//          cheaper than a broadcast) and carries the pose (R, t: 12 doubles) in registers.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/fit_ref.py.  The pose (FitPose), the modes of a pass and the step's helpers (fit_small, fit_cayley) are
// dh_fit_device.h's, which k_fit_views.hip shares; so is the pass itself (fit_pass), which k_ident.hip shares; the offsets of the
// sums are dh_fit.h's.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

template <bool STAGED>
__device__ __forceinline__ void fit_run(const FitArgs &a, const dh_render_instance *in, const FitModel &m, const float *s_pts,
                                        unsigned long long *s_sum) {
    const uint32_t fr = in->frame;
    const uint16_t *frame = a.frames + (size_t)fr * a.h * a.w;
    double K[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = (double)(a.cams ? a.cams[fr].k[q] : a.k[q]);
    FitPose pose;
#pragma unroll
    for (int q = 0; q < 9; ++q) pose.R[q] = (double)in->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) pose.t[q] = (double)in->t[q];
    const double scale = (double)in->scale;
    uint32_t steps = 0, status = DH_FIT_OK;
    bool stop = false;
    for (uint32_t it = 0; it < a.coarse; ++it) {
        fit_pass<FIT_COARSE, STAGED>(a, m, s_pts, frame, K, scale, pose, a.gate[0], s_sum);
        if ((uint32_t)s_sum[DH_FIT_COUNT] < a.min_points) { status = DH_FIT_FEW_POINTS; stop = true; break; }
        double x[6] = {0, 0, 0, 0, 0, 0};
        if (!fit_solve_tri<3, 6>(s_sum, DH_FIT_B, a.lam1, x)) { status = DH_FIT_SINGULAR; stop = true; break; }
#pragma unroll
        for (int j = 0; j < 3; ++j) pose.t[j] = pose.t[j] + x[j];
        ++steps;
        if (fit_small(x, 3)) break;
    }
    for (uint32_t it = 0; it < a.full && !stop; ++it) {
        fit_pass<FIT_FULL, STAGED>(a, m, s_pts, frame, K, scale, pose, a.gate[1], s_sum);
        if ((uint32_t)s_sum[DH_FIT_COUNT] < a.min_points) { status = DH_FIT_FEW_POINTS; break; }
        double x[6];
        if (!fit_solve_tri<6, 6>(s_sum, DH_FIT_B, a.lam1, x)) { status = DH_FIT_SINGULAR; break; }
#pragma unroll
        for (int j = 0; j < 3; ++j) pose.t[j] = pose.t[j] + x[j];
        fit_cayley(pose.R, x + 3);
        ++steps;
        if (fit_small(x, 6)) break;
    }
    fit_pass<FIT_LAST, STAGED>(a, m, s_pts, frame, K, scale, pose, a.gate[1], s_sum);
    if (threadIdx.x == 0) {
        dh_render_instance o = *in;
#pragma unroll
        for (int q = 0; q < 9; ++q) o.R[q] = (float)pose.R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) o.t[q] = (float)pose.t[q];
        a.out[blockIdx.x] = o;
        dh_fit_record rec;
        rec.points = (uint32_t)s_sum[DH_FIT_COUNT];
        rec.steps = steps;
        rec.status = status;
        rec.reserved = 0;
        rec.sum_r2_fixed = (int64_t)s_sum[DH_FIT_E];
        a.rec[blockIdx.x] = rec;
    }
}

// One instance's whole fit, the body of both kernels: the model staged into LDS where it fits, then the schedule of `a` (the
// first pass's barriers order the staging before its reads).  A macro: both kernels compile from the very tokens, and the
// __shared__ arrays are each kernel's own.
#define DH_FIT_BLOCK(a)                                                                                                           \
    __shared__ float s_pts[6 * DH_FIT_LDS_POINTS];                                                                             \
    __shared__ unsigned long long s_sum[32];                                                                                   \
    const dh_render_instance *in = (a).inst + blockIdx.x;                                                                      \
    const FitModel m = (a).models[in->mesh];                                                                                   \
    if (m.n <= DH_FIT_LDS_POINTS) {                                                                                            \
        for (uint32_t k = threadIdx.x; k < m.n * 3; k += DH_FIT_THREADS) {                                                     \
            const uint32_t i = k / 3, c = k - i * 3;                                                                           \
            s_pts[c * DH_FIT_LDS_POINTS + i] = m.pts[k];                                                                       \
            s_pts[(3 + c) * DH_FIT_LDS_POINTS + i] = m.nrm[k];                                                                 \
        }                                                                                                                      \
        fit_run<true>(a, in, m, s_pts, s_sum);                                                                                 \
    } else fit_run<false>(a, in, m, s_pts, s_sum)

__global__ __launch_bounds__(DH_FIT_THREADS) void k_fit(const FitArgs a) { DH_FIT_BLOCK(a); }

// The per-instance-schedule instance (dh_fit_tracker_step*): instance b runs (sched[b][0], sched[b][1]); a workgroup whose
// instance has no start (uniform over the workgroup) leaves before the model is staged and writes nothing.
__global__ __launch_bounds__(DH_FIT_THREADS) void k_fit_sched(const FitSchedArgs q) {
    if (dh_fit_seed_no_start(q.seed[blockIdx.x])) return;
    FitArgs a = q.f;
    a.coarse = q.sched[2 * blockIdx.x]; a.full = q.sched[2 * blockIdx.x + 1];
    DH_FIT_BLOCK(a);
}

// ------------------------------------------------------------------ launcher
hipError_t dh_launch_fit(const FitArgs &a, hipStream_t s) {
    if (a.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit, dim3(a.n_inst), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_fit_sched(const FitSchedArgs &a, hipStream_t s) {
    if (a.f.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_sched, dim3(a.f.n_inst), dim3(DH_FIT_THREADS), 0, s, a);
    return hipGetLastError();
}
