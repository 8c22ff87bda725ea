// k_fit_shape.hip -- one Gauss-Newton step of a model's shape coefficients over the fitted instances of each subject (DESIGN.md
// section 20; the rule is stated in include/depthhead_hip.h, section "adapting a model's shape to a subject").  Three kernels:
//   k_shape_accumulate  one workgroup of 256 lanes per instance; an instance that takes no part leaves at once.  Lanes stride
//          over the model's points: the fit's correspondence (DH_FIT_CORRESPOND, dh_fit_device.h: the statement fit_pass
//          expands too), then the point's K shape derivatives and its products into int64 partial sums in registers.  A single
//          pass reads every model and basis value once, so nothing is staged in LDS; the basis lies one plane per field and
//          axis, so a wave reads consecutive words.  The sums are reduced across the wave with shuffles, across the four waves
//          through LDS, and one 64-bit global atomic add per sum and workgroup lands them in the subject's row.  The loop
//          and the reduction are DH_SHAPE_BLOCK (dh_fit_device.h), which k_shape_accumulate_views (k_fit_shape_views.hip)
//          expands too; the clear and the solve below serve both.
//   k_shape_clear       zeroes the rows of the call's subjects, before the accumulation on the same stream.
//   k_shape_solve       one lane per subject: the fit's solve (fit_solve_tri, dh_fit_device.h) on the subject's row, the record.
// K is a template argument (1 .. 8): every array is indexed at compile time and stays in registers.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/shape_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

template <int NK>
__global__ __launch_bounds__(DH_SHAPE_THREADS) void k_shape_accumulate(const ShapeArgs a) {
    __shared__ long long s_part[DH_SHAPE_THREADS / 64][DH_SHAPE_STRIDE];
    const dh_render_instance *in = a.inst + blockIdx.x;
    const uint32_t subject = a.subjects ? a.subjects[blockIdx.x] : 0u;
    if (!shape_takes_part(a, in, subject)) return;                    // (uniform over the workgroup)
    const uint32_t fr = in->frame;
    const uint16_t *frame = a.frames + (size_t)fr * a.h * a.w;
    double K[9], R[9], t[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = (double)(a.cams ? a.cams[fr].k[q] : a.k[q]);
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = (double)in->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = (double)in->t[q];
    const double scale = (double)in->scale;
    DH_SHAPE_BLOCK(a, NK, frame, K, R, t, scale, subject, s_part);
}

template <int NK>
__global__ __launch_bounds__(64) void k_shape_solve(const ShapeArgs a) {
    const uint32_t sj = blockIdx.x * 64 + threadIdx.x;
    if (sj >= a.n_subjects) return;
    const unsigned long long *row = a.sums + (size_t)sj * DH_SHAPE_STRIDE;
    dh_shape_record rec;
#pragma unroll
    for (int k = 0; k < 8; ++k) rec.delta[k] = 0.0;
    const long long count = (long long)row[DH_SHAPE_COUNT];
    rec.points = (uint32_t)count;
    rec.instances = (uint32_t)row[DH_SHAPE_USED];
    rec.reserved = 0;
    rec.sum_r2_fixed = (int64_t)row[DH_SHAPE_E];
    rec.status = DH_SHAPE_OK;
    if (count < (long long)a.min_points) rec.status = DH_SHAPE_FEW_POINTS;
    else if (!fit_solve_tri<NK, 8>(row, DH_SHAPE_B, a.lam1, rec.delta)) rec.status = DH_SHAPE_SINGULAR;
    a.rec[sj] = rec;
}

// The rows of the call's subjects back to zero (a kernel, not a memset: the three operations of a call are three kernel nodes
// when a caller captures them in a graph).
__global__ __launch_bounds__(DH_SHAPE_THREADS) void k_shape_clear(unsigned long long *sums, uint32_t words) {
    const uint32_t i = blockIdx.x * DH_SHAPE_THREADS + threadIdx.x;
    if (i < words) sums[i] = 0;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_shape_clear(const ShapeArgs &a, hipStream_t s) {
    const uint32_t words = a.n_subjects * DH_SHAPE_STRIDE;
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_shape_clear, dim3((words + DH_SHAPE_THREADS - 1) / DH_SHAPE_THREADS), dim3(DH_SHAPE_THREADS), 0, s, a.sums, words);
    return hipGetLastError();
}
template <int NK>
static hipError_t launch_accumulate(const ShapeArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_shape_accumulate<NK>, dim3(a.n_inst), dim3(DH_SHAPE_THREADS), 0, s, a);
    return hipGetLastError();
}
template <int NK>
static hipError_t launch_solve(const ShapeArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_shape_solve<NK>, dim3((a.n_subjects + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}
#define SHAPE_DISPATCH(fn)                                                                                                     \
    switch (a.nk) {                                                                                                            \
    case 1: return fn<1>(a, s); case 2: return fn<2>(a, s); case 3: return fn<3>(a, s); case 4: return fn<4>(a, s);             \
    case 5: return fn<5>(a, s); case 6: return fn<6>(a, s); case 7: return fn<7>(a, s); case 8: return fn<8>(a, s);             \
    default: return hipErrorInvalidValue;                                                                                      \
    }
hipError_t dh_launch_shape_accumulate(const ShapeArgs &a, hipStream_t s) {
    if (a.n_inst == 0) return hipSuccess;
    SHAPE_DISPATCH(launch_accumulate)
}
hipError_t dh_launch_shape_solve(const ShapeArgs &a, hipStream_t s) {
    if (a.n_subjects == 0) return hipSuccess;
    SHAPE_DISPATCH(launch_solve)
}
