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
// dh_fit_device.h's, which k_fit_views.hip shares; the offsets of the sums are dh_fit.h's.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

// One pass at `pose` with gate `gate`: the sums of MODE into s_sum (zeroed here; valid for every lane after the return).
template <int MODE, bool STAGED>
__device__ __forceinline__ void fit_pass(const FitArgs &a, const FitModel &m, const float *s_pts, const uint16_t *frame, const double K[9],
                                         double scale, const FitPose &pose, double gate, unsigned long long *s_sum) {
    constexpr int NJ = MODE == FIT_COARSE ? 3 : MODE == FIT_FULL ? 6 : 0;
    constexpr int NA = NJ * (NJ + 1) / 2;
    long long accA[NA > 0 ? NA : 1], accB[NJ > 0 ? NJ : 1];
#pragma unroll
    for (int k = 0; k < (NA > 0 ? NA : 1); ++k) accA[k] = 0;
#pragma unroll
    for (int k = 0; k < (NJ > 0 ? NJ : 1); ++k) accB[k] = 0;
    long long e = 0, cnt = 0;
    __syncthreads();                               // every lane has read the sums of the pass before
    if (threadIdx.x < DH_FIT_SUMS) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const double dw = (double)a.w, dh = (double)a.h;
    for (uint32_t i = threadIdx.x; i < m.n; i += DH_FIT_THREADS) {
        double v[3], nm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = (double)(STAGED ? s_pts[c * DH_FIT_LDS_POINTS + i] : m.pts[(size_t)i * 3 + c]);
            nm[c] = (double)(STAGED ? s_pts[(3 + c) * DH_FIT_LDS_POINTS + i] : m.nrm[(size_t)i * 3 + c]);
        }
        DH_FIT_CORRESPOND(v, nm, scale, pose.R, pose.t, K, frame, a.w, dw, dh, gate);
        if (MODE == FIT_LAST) e += (long long)((res * res) * DH_FIT_S);
        else {
            double J[6];
            J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
            if (MODE == FIT_FULL) {
                const double q0 = p[0] - pose.t[0], q1 = p[1] - pose.t[1], q2 = p[2] - pose.t[2];
                J[3] = q1 * n[2] - q2 * n[1];
                J[4] = q2 * n[0] - q0 * n[2];
                J[5] = q0 * n[1] - q1 * n[0];
            }
            int k = 0;
#pragma unroll
            for (int ja = 0; ja < NJ; ++ja) {
#pragma unroll
                for (int jb = ja; jb < NJ; ++jb) accA[k++] += (long long)((J[ja] * J[jb]) * DH_FIT_S);
                accB[ja] += (long long)((J[ja] * res) * DH_FIT_S);
            }
        }
        cnt += 1;
    }
    const bool lead = (threadIdx.x & 63) == 0;
    {
        int k = 0;
#pragma unroll
        for (int ja = 0; ja < NJ; ++ja) {
#pragma unroll
            for (int jb = ja; jb < NJ; ++jb) {
                const unsigned long long s = wave_sum_u64((uint64_t)accA[k++]);
                if (lead) atomicAdd(&s_sum[DH_FIT_PAIR(6, ja, jb)], s);
            }
            const unsigned long long s = wave_sum_u64((uint64_t)accB[ja]);
            if (lead) atomicAdd(&s_sum[DH_FIT_B + ja], s);
        }
    }
    if (MODE == FIT_LAST) {
        const unsigned long long s = wave_sum_u64((uint64_t)e);
        if (lead) atomicAdd(&s_sum[DH_FIT_E], s);
    }
    {
        const unsigned long long s = wave_sum_u64((uint64_t)cnt);
        if (lead) atomicAdd(&s_sum[DH_FIT_COUNT], s);
    }
    __syncthreads();
}

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
