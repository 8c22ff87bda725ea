// k_calib_views.hip -- one Gauss-Newton step of every camera's extrinsics over the fitted instances it sees (DESIGN.md section 24;
// the rule is stated in include/depthhead_hip.h, section "calibrating a view table").  Three kernels:
//   k_calib_clear       zeroes the rows of the table's cameras, before the accumulation on the same stream.
//   k_calib_accumulate  one workgroup of 256 lanes per (instance, view) PAIR over section 23's grid: n_inst * ranks workgroups,
//          ranks = min(64, n cameras), workgroup g taking rank r = g / n_inst of instance i = g mod n_inst.  It leaves at once
//          when the instance has r set bits or fewer or takes no part (dh_calib_skip, dh_fit.h: the host form's refusals,
//          decided on the device), or when the pair does (dh_calib_pair: the camera is held, or the arm limit).  Otherwise the
//          composite (R_v, t_v) and the camera's pivot g_c -- the same in every lane -- move to scalar registers, lanes stride
//          over the model's points (DH_FIT_CORRESPOND, then the fit's row about g_c with the rotation columns in units of
//          DH_CALIB_ARM_UNIT), 29 int64 partial sums stay in registers, are reduced across the wave with shuffles and across
//          the four waves through LDS, and one 64-bit global atomic add per word and workgroup lands them in the CAMERA's row.
//          (g -> (i, r) is a bijection onto the pairs whatever the hardware does with the workgroups: correctness does not
//          depend on placement; integer atomics make the order free.)
//   k_calib_solve       one lane per camera: the fit's damped 6 x 6 solve (fit_solve_tri), the Cayley update of (V, u) about the
//          pivot (fit_cayley's expressions), the orthonormality test of the rounded V', the record.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/calib_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(DH_CALIB_THREADS) void k_calib_clear(unsigned long long *sums, uint32_t words) {
    const uint32_t i = blockIdx.x * DH_CALIB_THREADS + threadIdx.x;
    if (i < words) sums[i] = 0;
}

__global__ __launch_bounds__(DH_CALIB_THREADS) void k_calib_accumulate(const CalibArgs a) {
    __shared__ long long s_part[DH_CALIB_THREADS / 64][DH_CALIB_STRIDE];
    const uint32_t b = blockIdx.x % a.n_inst, rank = blockIdx.x / a.n_inst;          // b < n_inst, rank < ranks
    const dh_view_instance *in = a.inst + b;
    const uint64_t mask = in->views;
    if (rank >= (uint32_t)__builtin_popcountll(mask)) return;                         // (uniform over the workgroup, as all below)
    const uint32_t take = a.take ? a.take[b] : 0u;
    const uint32_t set = a.sets ? a.sets[b] : 0u;
    if (dh_calib_skip(*in, set, take, (uint32_t)a.n, a.n_sets, a.radius).why != DH_SHAPE_VIEWS_OK) return;
    // the instance passed: every set bit names a camera < n and set < n_sets, and rank < popcount(mask) gives a bit < 64
    const uint32_t cam = in->first_cam + dh_shape_view_bit(mask, rank);
    const CalibPair pr = dh_calib_pair(*in, a.views[cam], a.pivot, a.hold && a.hold[cam] != 0);
    if (pr.why != DH_CALIB_PAIR_OK) return;
    const uint16_t *frame = a.frames + ((size_t)set * a.n + cam) * a.h * a.w;
    double K[9], R[9], t[3], g[3];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        K[j] = uni((double)a.cams[cam].k[j]);
        R[j] = uni(pr.R[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) { t[j] = uni(pr.t[j]); g[j] = uni(pr.g[j]); }
    const double scale = uni((double)in->scale);
    const double dw = (double)a.w, dh = (double)a.h, gate = a.gate;

    long long accA[21], accB[6], e = 0, cnt = 0;
#pragma unroll
    for (int k = 0; k < 21; ++k) accA[k] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) accB[k] = 0;
    for (uint32_t i = threadIdx.x; i < a.np; i += DH_CALIB_THREADS) {
        double v[3], nm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = (double)a.pts[(size_t)i * 3 + c];
            nm[c] = (double)a.nrm[(size_t)i * 3 + c];
        }
        DH_FIT_CORRESPOND(v, nm, scale, R, t, K, frame, a.w, dw, dh, gate);
        const double q0 = p[0] - g[0], q1 = p[1] - g[1], q2 = p[2] - g[2];
        double J[6];
        J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
        J[3] = (q1 * n[2] - q2 * n[1]) / DH_CALIB_ARM_UNIT;
        J[4] = (q2 * n[0] - q0 * n[2]) / DH_CALIB_ARM_UNIT;
        J[5] = (q0 * n[1] - q1 * n[0]) / DH_CALIB_ARM_UNIT;
        int k = 0;
#pragma unroll
        for (int ja = 0; ja < 6; ++ja) {
#pragma unroll
            for (int jb = ja; jb < 6; ++jb) accA[k++] += (long long)((J[ja] * J[jb]) * DH_FIT_S);
            accB[ja] += (long long)((J[ja] * res) * DH_FIT_S);
        }
        e += (long long)((res * res) * DH_FIT_S);
        cnt += 1;
    }
    // ---- across the wave in registers, across the waves in LDS, then one global atomic per word
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    {
        int k = 0;
#pragma unroll
        for (int ja = 0; ja < 6; ++ja) {
#pragma unroll
            for (int jb = ja; jb < 6; ++jb) {
                const long long s = (long long)wave_sum_u64((uint64_t)accA[k++]);
                if (lead) s_part[wave][DH_FIT_PAIR(6, ja, jb)] = s;
            }
            const long long s = (long long)wave_sum_u64((uint64_t)accB[ja]);
            if (lead) s_part[wave][DH_FIT_B + ja] = s;
        }
        const long long se = (long long)wave_sum_u64((uint64_t)e), sc = (long long)wave_sum_u64((uint64_t)cnt);
        if (lead) { s_part[wave][DH_FIT_E] = se; s_part[wave][DH_FIT_COUNT] = sc; }
    }
    __syncthreads();
    const int word = threadIdx.x;
    if (word > DH_FIT_USED) return;
    unsigned long long *row = a.sums + (size_t)cam * DH_CALIB_STRIDE;                 // cam < n
    long long s = 0;
#pragma unroll
    for (int wv = 0; wv < DH_CALIB_THREADS / 64; ++wv) s += s_part[wv][word == DH_FIT_USED ? DH_FIT_COUNT : word];
    if (word == DH_FIT_USED) {
        if (s > 0) atomicAdd(&row[DH_FIT_USED], 1ull);
        return;
    }
    atomicAdd(&row[word], (unsigned long long)s);
}

__global__ __launch_bounds__(64) void k_calib_solve(const CalibArgs a) {
    const uint32_t cam = blockIdx.x * 64 + threadIdx.x;
    if (cam >= (uint32_t)a.n) return;
    const unsigned long long *row = a.sums + (size_t)cam * DH_CALIB_STRIDE;
    const FitView vw = a.views[cam];
    dh_calib_record rec;
#pragma unroll
    for (int q = 0; q < 9; ++q) rec.V[q] = vw.V[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) rec.u[q] = vw.u[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) rec.delta[q] = 0.0;
    const long long count = (long long)row[DH_FIT_COUNT];
    rec.points = (uint32_t)count;
    rec.pairs = (uint32_t)row[DH_FIT_USED];
    rec.reserved = 0;
    rec.sum_r2_fixed = (int64_t)row[DH_FIT_E];
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (a.hold && a.hold[cam] != 0) rec.status = DH_CALIB_HELD;
    else if (count < (long long)a.min_points) rec.status = DH_CALIB_FEW_POINTS;
    else if (!fit_solve_tri<6, 6>(row, DH_FIT_B, a.lam1, x)) rec.status = DH_CALIB_SINGULAR;
    else {
        double g[3];
        dh_calib_pivot(vw, a.pivot, g);
        const double w[3] = {x[3] / DH_CALIB_ARM_UNIT, x[4] / DH_CALIB_ARM_UNIT, x[5] / DH_CALIB_ARM_UNIT};
        // V' = C V, and C s for s = u - g_c as the first column of a matrix whose others are zero: fit_cayley's expressions
        // form C from w alike both times and o[i][0] = (C[i][0] * s0 + C[i][1] * s1) + C[i][2] * s2
        double V[9], Cs[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) { V[q] = (double)vw.V[q]; Cs[q] = 0.0; }
#pragma unroll
        for (int q = 0; q < 3; ++q) Cs[3 * q] = (double)vw.u[q] - g[q];
        fit_cayley(V, w);
        fit_cayley(Cs, w);
        float Vf[9], uf[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) Vf[q] = (float)V[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) uf[q] = (float)((Cs[3 * q] + g[q]) + x[q]);
        bool ortho = true;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) {
                const double gm = ((double)Vf[3 * r] * (double)Vf[3 * c] + (double)Vf[3 * r + 1] * (double)Vf[3 * c + 1]) +
                                  (double)Vf[3 * r + 2] * (double)Vf[3 * c + 2];
                const double d = gm - (r == c ? 1.0 : 0.0);
                ortho = ortho && (d < 0.0 ? -d : d) <= DH_FIT_VIEW_TOLERANCE;
            }
        if (!ortho) rec.status = DH_CALIB_NOT_ORTHONORMAL;
        else {
            rec.status = DH_CALIB_OK;
#pragma unroll
            for (int q = 0; q < 9; ++q) rec.V[q] = Vf[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) { rec.u[q] = uf[q]; rec.delta[q] = x[q]; rec.delta[3 + q] = w[q]; }
        }
    }
    a.rec[cam] = rec;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_calib_clear(const CalibArgs &a, hipStream_t s) {
    const uint32_t words = (uint32_t)a.n * DH_CALIB_STRIDE;                           // n <= 65535
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_calib_clear, dim3((words + DH_CALIB_THREADS - 1) / DH_CALIB_THREADS), dim3(DH_CALIB_THREADS), 0, s, a.sums, words);
    return hipGetLastError();
}
hipError_t dh_launch_calib_accumulate(const CalibArgs &a, hipStream_t s) {
    if (a.n_inst == 0 || a.ranks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_calib_accumulate, dim3(a.n_inst * a.ranks), dim3(DH_CALIB_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_calib_solve(const CalibArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_calib_solve, dim3(((uint32_t)a.n + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}
