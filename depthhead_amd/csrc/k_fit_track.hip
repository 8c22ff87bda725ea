// k_fit_track.hip -- each camera's fitted pose carried across steps (the rule is stated in
// include/depthhead_hip.h, section "carrying each camera's fitted pose across steps").  Two kernels of one lane per camera around
// k_fit's per-instance-schedule instance (k_fit.hip):
//   k_fit_track_seed    steps 0 - 2: absent / detection valid / the start instance, its schedule and its kind;
//   k_fit_track_update  steps 4 - 6: acceptance, the camera's state and its record.
// f32 and f64 with + - * /, compares and casts only, every operation rounded on its own; the cosines and sines come from the
// host's 120-entry table.  Bit-identical to tests/fit_track_ref.py.
#include "dh_device.h"
#include "dh_fit.h"

#pragma clang fp contract(off)

__device__ __forceinline__ uint32_t sat_inc(uint32_t v) { return v == 0xffffffffu ? v : v + 1u; }

// o = A B, each element as (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]
__device__ __forceinline__ void mat3_mul(const double A[9], const double B[9], double o[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_fit_track_seed(const FitTrackArgs a) {
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    if (c >= a.n) return;
    dh_render_instance in;
    in.frame = (uint32_t)c; in.mesh = 0; in.scale = a.scale; in.flags = 0;
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
        const dh_fit_track_state &st = a.state[c];
        if (st.tracked) {
            kind = DH_FIT_SEED_CARRIED;
            full = a.prm.iterations_tracked;
#pragma unroll
            for (int q = 0; q < 9; ++q) in.R[q] = st.R[q];
            const bool motion = (a.flags & DH_FIT_TRACK_MOTION) && st.have_prev;
#pragma unroll
            for (int q = 0; q < 3; ++q) in.t[q] = motion ? st.t[q] + (st.t[q] - st.t_prev[q]) : st.t[q];
        } else if (valid) {
            kind = DH_FIT_SEED_FOREST;
            coarse = a.coarse; full = a.full;
            const dh_pose po = a.poses[c];
            double cs[3], sn[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double x = po.rotation[j] / 3.14159 * 60.0 + 60.5;
                const int ri = !(x >= 0.0) ? 0 : x >= 119.0 ? 119 : (int)x;
                cs[j] = a.angles[2 * ri]; sn[j] = a.angles[2 * ri + 1];
            }
            const double Z[9] = {cs[0], sn[0], 0.0, -sn[0], cs[0], 0.0, 0.0, 0.0, 1.0};
            const double Y[9] = {cs[1], 0.0, sn[1], 0.0, 1.0, 0.0, -sn[1], 0.0, cs[1]};
            const double X[9] = {1.0, 0.0, 0.0, 0.0, cs[2], -sn[2], 0.0, sn[2], cs[2]};
            double M[9], R[9];
            mat3_mul(Y, Z, M);
            mat3_mul(X, M, R);
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

__global__ __launch_bounds__(DH_FIT_TRACK_THREADS) void k_fit_track_update(const FitTrackArgs a) {
    const int c = blockIdx.x * DH_FIT_TRACK_THREADS + threadIdx.x;
    if (c >= a.n) return;
    const uint32_t seed = a.seed[c], kind = seed & 0xffu;
    dh_fit_track_state st = a.state[c];
    dh_fit_track_record rec;
    rec.reserved = 0;
    if (kind == DH_FIT_SEED_ABSENT || kind == DH_FIT_SEED_NONE) {
        rec.instance.frame = 0; rec.instance.mesh = 0; rec.instance.scale = 0.0f; rec.instance.flags = 0;
#pragma unroll
        for (int q = 0; q < 9; ++q) rec.instance.R[q] = 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) rec.instance.t[q] = 0.0f;
        rec.fit.points = 0; rec.fit.steps = 0; rec.fit.status = 0; rec.fit.reserved = 0; rec.fit.sum_r2_fixed = 0;
        st.lost = sat_inc(st.lost);
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
        uint32_t why = 0;
        if (fr.status != DH_FIT_OK) why |= DH_FIT_TRACK_BAD_STATUS;
        if (fr.points < a.prm.keep_points) why |= DH_FIT_TRACK_BAD_POINTS;
        if (fr.sum_r2_fixed > a.rms_lim * (long long)fr.points) why |= DH_FIT_TRACK_BAD_RMS;
        if (seed & DH_FIT_SEED_VALID) {
            const dh_pose po = a.poses[c];
            const double dx = (double)fit.t[0] - (double)po.mid_point[0], dy = (double)fit.t[1] - (double)po.mid_point[1],
                         dz = (double)fit.t[2] - (double)po.mid_point[2];
            if (!((dx * dx + dy * dy) + dz * dz <= a.jump2)) why |= DH_FIT_TRACK_BAD_JUMP;
        }
        rec.fit = fr;
        if (why == 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { st.t_prev[q] = st.t[q]; st.t[q] = fit.t[q]; }
#pragma unroll
            for (int q = 0; q < 9; ++q) st.R[q] = fit.R[q];
            st.have_prev = st.tracked;
            st.tracked = 1;
            st.age = sat_inc(st.age);
            st.lost = 0;
            rec.instance = fit;
            rec.status = kind == DH_FIT_SEED_CARRIED ? DH_FIT_TRACK_CARRIED : DH_FIT_TRACK_FITTED;
        } else {
            st.tracked = 0; st.have_prev = 0; st.age = 0;
            st.lost = sat_inc(st.lost);
            rec.instance = a.start[c];
            rec.status = DH_FIT_TRACK_REJECTED | why;
        }
    }
    rec.age = st.age; rec.lost = st.lost;
    a.state[c] = st;
    a.records[c] = rec;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_fit_track_seed(const FitTrackArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_track_seed, dim3((a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_fit_track_update(const FitTrackArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_track_update, dim3((a.n + DH_FIT_TRACK_THREADS - 1) / DH_FIT_TRACK_THREADS), dim3(DH_FIT_TRACK_THREADS), 0, s, a);
    return hipGetLastError();
}
