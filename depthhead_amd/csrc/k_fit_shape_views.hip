// k_fit_shape_views.hip -- the accumulation of a shape step over the views of a rig (the rule is stated in
// include/depthhead_hip.h, section "adapting a model's shape across views").  One kernel; the clear before it and the solve after
// it are k_fit_shape.hip's.
//   k_shape_accumulate_views  one workgroup of 256 lanes per (instance, view) PAIR, not a loop over views: a subject's sums land
//          by integer atomics whose order is free, so the views of an instance can go to separate workgroups at no cost to
//          exactness.  The grid is n_inst * ranks workgroups, ranks = min(64, n cameras): workgroup g takes rank r = g / n_inst
//          of instance i = g mod n_inst, so that the r-th views of all instances are consecutive workgroups and spread over the
//          XCDs (the order k_fit_views_sched deals its slots in).  It leaves at once when the instance has r set bits or fewer,
//          or takes no part (dh_shape_views_skip, dh_fit.h: the host form's refusals, decided on the device).  Otherwise it
//          finds the r-th set bit (dh_shape_view_bit), composes the view's camera pose (R_v, t_v) = (V R_w, V t_w + u) as
//          k_fit_views does -- the same in every lane, moved to scalar registers, V and u dead after it -- and runs
//          DH_SHAPE_BLOCK (dh_fit_device.h), the point loop and reduction k_shape_accumulate expands, at (scale, R_v, t_v),
//          camera c's K and frame set * n + c.  (g -> (i, r) is a bijection onto the pairs whatever the hardware does with
//          the workgroups: correctness does not depend on placement.)
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/shape_views_ref.py.  With one view, V = I, u = 0 and one set every sum equals k_shape_accumulate's.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

template <int NK>
__global__ __launch_bounds__(DH_SHAPE_THREADS) void k_shape_accumulate_views(const ShapeViewsArgs args) {
    __shared__ long long s_part[DH_SHAPE_THREADS / 64][DH_SHAPE_STRIDE];
    const ShapeArgs &a = args.s;
    const uint32_t b = blockIdx.x % a.n_inst, rank = blockIdx.x / a.n_inst;          // b < n_inst, rank < ranks
    const dh_view_instance *in = args.inst + b;
    const uint64_t mask = in->views;
    if (rank >= (uint32_t)__builtin_popcountll(mask)) return;                         // (uniform over the workgroup, as all below)
    const uint32_t subject = a.subjects ? a.subjects[b] : 0u;
    const uint32_t set = args.sets ? args.sets[b] : 0u;
    if (dh_shape_views_skip(*in, set, subject, (uint32_t)a.n, args.n_sets, a.n_subjects, a.radius, a.largest).why != DH_SHAPE_VIEWS_OK) return;
    // the instance passed: every set bit names a camera < n and set < n_sets, and rank < popcount(mask) gives a bit < 64
    const uint32_t cam = in->first_cam + dh_shape_view_bit(mask, rank);
    const uint16_t *frame = a.frames + ((size_t)set * a.n + cam) * a.h * a.w;
    const FitView *vw = args.views + cam;
    double K[9], R[9], t[3];
    {
        double V[9], Rw[9], tw[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            V[j] = (double)vw->V[j];
            Rw[j] = (double)in->R[j];
            K[j] = uni((double)a.cams[cam].k[j]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) tw[j] = (double)in->t[j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = uni((V[3 * i] * Rw[j] + V[3 * i + 1] * Rw[3 + j]) + V[3 * i + 2] * Rw[6 + j]);
            t[i] = uni(((V[3 * i] * tw[0] + V[3 * i + 1] * tw[1]) + V[3 * i + 2] * tw[2]) + (double)vw->u[i]);
        }
    }
    const double scale = uni((double)in->scale);
    DH_SHAPE_BLOCK(a, NK, frame, K, R, t, scale, subject, s_part);
}

// ------------------------------------------------------------------ launcher
template <int NK>
static hipError_t launch_accumulate_views(const ShapeViewsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_shape_accumulate_views<NK>, dim3(a.s.n_inst * a.ranks), dim3(DH_SHAPE_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_shape_accumulate_views(const ShapeViewsArgs &a, hipStream_t s) {
    if (a.s.n_inst == 0 || a.ranks == 0) return hipSuccess;
    switch (a.s.nk) {
    case 1: return launch_accumulate_views<1>(a, s); case 2: return launch_accumulate_views<2>(a, s);
    case 3: return launch_accumulate_views<3>(a, s); case 4: return launch_accumulate_views<4>(a, s);
    case 5: return launch_accumulate_views<5>(a, s); case 6: return launch_accumulate_views<6>(a, s);
    case 7: return launch_accumulate_views<7>(a, s); case 8: return launch_accumulate_views<8>(a, s);
    default: return hipErrorInvalidValue;
    }
}
