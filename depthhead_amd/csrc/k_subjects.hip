// k_subjects.hip -- a shape per subject on the device (the rule is stated in include/depthhead_hip.h, section
// "a shape per subject").  A dh_fit_subjects holds S deformable models of one base mesh; the kernels here evaluate each subject's
// coefficients into its model and take the shape step of section 20 with every instance at its own subject's model.
//   k_subjects_apply    one lane per subject: the record's increment into the subject's coefficients (the finite test, the sum,
//          the clamp, the counters and flags), and the subject's zero-normal count back to 0 for the normals pass.
//   k_subjects_points   one lane per (subject, vertex), the subject in blockIdx.y: v + sum_k c_k B_k[i] from the BASE mesh in f64,
//          rounded to f32 once.  The basis lies one plane per field and axis, so a wave reads consecutive words.
//   k_subjects_normals  one lane per (subject, vertex): the face products of the vertex's incident corners, each recomputed from
//          the f32 points that k_subjects_points wrote, summed in the order of the vertex's corner list -- a gather, no atomic on
//          a float anywhere -- then the one square root and the division.  A zero normal stays (0, 0, 0) and is counted (one
//          integer atomic per wave).
//   k_fit_carry         one lane per instance of a fit call's table: R and t from the device output of an earlier fit, where
//          they pass the finite and orthonormal tests of dh_fit_instance_fault; the uploaded (checked) instance stays otherwise.
//   k_shape_accumulate_subjects   k_shape_accumulate (k_fit_shape.hip) with `a` bound to a ShapeArgs whose pts / nrm are those of
//          the workgroup's subject, and the instances of a fit that did not end DH_FIT_OK left out: DH_SHAPE_BLOCK from the very
//          tokens.  k_shape_clear and k_shape_solve (k_fit_shape.hip) serve it unchanged.
// The face products are recomputed per corner rather than kept in a scratch array [S][n_tris][3] f64: the scratch would be 24 bytes
// a triangle and subject (805 MB at the limits), written once and read three times, where the recomputation reads nine f32 that
// the points pass has just left in L2; it also saves a launch.
// f64 with + - * /, one square root, compares and casts, every operation rounded on its own: bit-identical run to run and to
// tests/subjects_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(64) void k_subjects_apply(const SubjectsArgs a) {
    const uint32_t sj = a.first + blockIdx.x * 64 + threadIdx.x;
    if (sj >= a.first + a.count) return;
    dh_subject_state st = a.state[sj];
    st.zero_normals = 0;
    if (a.rec && a.rec[sj].status == DH_SHAPE_OK) {
        const dh_shape_record r = a.rec[sj];
        bool finite = true;
#pragma unroll
        for (uint32_t k = 0; k < DH_SHAPE_MAX_FIELDS; ++k)
            if (k < a.nk) finite = finite && r.delta[k] - r.delta[k] == 0.0;                       // (x - x is 0.0 for a finite x alone)
        if (!finite) {
            st.rejected = fit_sat_inc(st.rejected);
            st.flags |= DH_SUBJECT_NONFINITE;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < DH_SHAPE_MAX_FIELDS; ++k) {
                if (k >= a.nk) continue;
                double c = st.coeffs[k] + r.delta[k];
                if (c > a.max_coeff) { c = a.max_coeff; st.flags |= DH_SUBJECT_CLAMPED; }
                if (c < -a.max_coeff) { c = -a.max_coeff; st.flags |= DH_SUBJECT_CLAMPED; }
                st.coeffs[k] = c;
            }
            st.applied = fit_sat_inc(st.applied);
        }
    }
    a.state[sj] = st;
}

__global__ __launch_bounds__(DH_SUBJECTS_THREADS) void k_subjects_points(const SubjectsArgs a) {
    const uint32_t sj = a.first + blockIdx.y;
    const uint32_t i = blockIdx.x * DH_SUBJECTS_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const double *coeffs = a.state[sj].coeffs;                        // (uniform over the workgroup)
    const size_t n = a.n;
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (double)a.base[(size_t)i * 3 + c];
    for (uint32_t k = 0; k < a.nk; ++k) {
        const double ck = coeffs[k];
        const float *plane = a.basis + (size_t)k * 3 * n + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = v[c] + ck * (double)plane[(size_t)c * n];
    }
    float *out = a.models[sj].pts + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (float)v[c];
}

__global__ __launch_bounds__(DH_SUBJECTS_THREADS) void k_subjects_normals(const SubjectsArgs a) {
    const uint32_t sj = a.first + blockIdx.y;
    const uint32_t i = blockIdx.x * DH_SUBJECTS_THREADS + threadIdx.x;
    bool zero = false;
    if (i < a.n) {
        const float *pts = a.models[sj].pts;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        const uint32_t end = a.corner_begin[i + 1];
        for (uint32_t j = a.corner_begin[i]; j < end; ++j) {
            const uint32_t *tri = a.tris + (size_t)(a.corners[j] / 3u) * 3;
            const float *pa = pts + (size_t)tri[0] * 3, *pb = pts + (size_t)tri[1] * 3, *pc = pts + (size_t)tri[2] * 3;
            const double a0 = (double)pa[0], a1 = (double)pa[1], a2 = (double)pa[2];
            const double u0 = (double)pb[0] - a0, u1 = (double)pb[1] - a1, u2 = (double)pb[2] - a2;
            const double w0 = (double)pc[0] - a0, w1 = (double)pc[1] - a1, w2 = (double)pc[2] - a2;
            s0 = s0 + (u1 * w2 - u2 * w1);
            s1 = s1 + (u2 * w0 - u0 * w2);
            s2 = s2 + (u0 * w1 - u1 * w0);
        }
        const double q = (s0 * s0 + s1 * s1) + s2 * s2;
        const double ln = __dsqrt_rn(q);
        zero = !(ln > 0.0);
        const double d = zero ? 1.0 : ln;
        float *out = a.models[sj].nrm + (size_t)i * 3;
        out[0] = (float)(s0 / d); out[1] = (float)(s1 / d); out[2] = (float)(s2 / d);
    }
    // (every lane of the wave is here: the vertices past n vote false)
    const uint32_t zeros = (uint32_t)__builtin_popcountll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd(&a.state[sj].zero_normals, zeros);
}

__global__ __launch_bounds__(64) void k_fit_carry(dh_render_instance *inst, const dh_render_instance *carried, uint32_t n_inst) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_inst) return;
    dh_render_instance in = inst[i];
#pragma unroll
    for (int q = 0; q < 9; ++q) in.R[q] = carried[i].R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) in.t[q] = carried[i].t[q];
    // (radius and largest 0.0: the scale is the uploaded instance's, whose extent the host has checked)
    if (dh_fit_instance_fault(in, 0.0, 0.0).why == DH_FIT_INST_OK) inst[i] = in;
}

template <int NK>
__global__ __launch_bounds__(DH_SHAPE_THREADS) void k_shape_accumulate_subjects(const ShapeSubjectsArgs g) {
    __shared__ long long s_part[DH_SHAPE_THREADS / 64][DH_SHAPE_STRIDE];
    const dh_render_instance *in = g.s.inst + blockIdx.x;
    const uint32_t subject = g.s.subjects ? g.s.subjects[blockIdx.x] : 0u;
    if (g.fit_rec && g.fit_rec[blockIdx.x].status != DH_FIT_OK) return;   // (uniform over the workgroup, as what follows)
    if (!shape_takes_part(g.s, in, subject)) return;
    ShapeArgs a = g.s;
    a.pts = g.models[subject].pts; a.nrm = g.models[subject].nrm;
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

// ------------------------------------------------------------------ launchers
// The three kernels of one evaluation of subjects a.first .. a.first + a.count - 1, stream-ordered on `s`.
hipError_t dh_launch_subjects_update(const SubjectsArgs &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_subjects_apply, dim3((a.count + 63) / 64), dim3(64), 0, s, a);
    const dim3 grid((a.n + DH_SUBJECTS_THREADS - 1) / DH_SUBJECTS_THREADS, a.count);
    hipLaunchKernelGGL(k_subjects_points, grid, dim3(DH_SUBJECTS_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_subjects_normals, grid, dim3(DH_SUBJECTS_THREADS), 0, s, a);
    return hipGetLastError();
}
// The same kernels one by one: a surface set (k_surface.hip) evaluates its points with a kernel of its own between them.
hipError_t dh_launch_subjects_apply(const SubjectsArgs &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    hipLaunchKernelGGL(k_subjects_apply, dim3((a.count + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_subjects_normals(const SubjectsArgs &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    const dim3 grid((a.n + DH_SUBJECTS_THREADS - 1) / DH_SUBJECTS_THREADS, a.count);
    hipLaunchKernelGGL(k_subjects_normals, grid, dim3(DH_SUBJECTS_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_fit_carry(dh_render_instance *inst, const dh_render_instance *carried, uint32_t n_inst, hipStream_t s) {
    if (n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fit_carry, dim3((n_inst + 63) / 64), dim3(64), 0, s, inst, carried, n_inst);
    return hipGetLastError();
}
template <int NK>
static hipError_t launch_accumulate_subjects(const ShapeSubjectsArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(k_shape_accumulate_subjects<NK>, dim3(a.s.n_inst), dim3(DH_SHAPE_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_shape_accumulate_subjects(const ShapeSubjectsArgs &a, hipStream_t s) {
    if (a.s.n_inst == 0) return hipSuccess;
    switch (a.s.nk) {
    case 1: return launch_accumulate_subjects<1>(a, s); case 2: return launch_accumulate_subjects<2>(a, s);
    case 3: return launch_accumulate_subjects<3>(a, s); case 4: return launch_accumulate_subjects<4>(a, s);
    case 5: return launch_accumulate_subjects<5>(a, s); case 6: return launch_accumulate_subjects<6>(a, s);
    case 7: return launch_accumulate_subjects<7>(a, s); case 8: return launch_accumulate_subjects<8>(a, s);
    default: return hipErrorInvalidValue;
    }
}
