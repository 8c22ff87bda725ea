// dh_fit_device.h -- the device arithmetic that the fit family's kernels must agree on bit for bit, each piece stated once:
//   the per-point correspondence and the damped solve     k_fit.hip, k_fit_views.hip, k_fit_shape.hip, k_fit_shape_views.hip
//   the shape step's point loop and reduction              k_fit_shape.hip, k_fit_shape_views.hip, k_subjects.hip
//   the pose, the modes of a pass, the step's helpers      k_fit.hip, k_fit_views.hip (each with its *_sched instance)
//   the single-view pass                                   k_fit.hip, k_ident.hip, k_subject_track.hip
//   a pair of the identification                           k_ident.hip, k_subject_track.hip
//   the multi-view pass                                    k_fit_views.hip, k_ident_views.hip, k_rig_subject_track.hip
//   a pair of the multi-view identification                k_ident_views.hip, k_rig_subject_track.hip
//   the decision of an identification by one wave          k_ident.hip, k_ident_views.hip, k_subject_track.hip, k_rig_subject_track.hip
//   the trackers' rule: table rotation, carried start,
//   acceptance, jump test and the state updates            k_fit_track.hip, k_rig_fit_track.hip, k_subject_track.hip, k_rig_subject_track.hip
//   the seed of one rig                                    k_rig_fit_track.hip, k_rig_subject_track.hip
// f64 (the trackers: f32 too) with + - * /, compares and casts only; every operation is rounded on its own, so the expression
// trees below are the contract (tests/fit_ref.py, shape_ref.py, view_fit_ref.py, fit_track_ref.py and rig_fit_track_ref.py and
// shape_views_ref.py restate them).  Not part of the ABI.
#pragma once
#include "dh_device.h"
#include "dh_fit.h"

#pragma clang fp contract(off)

// The rule for one model point (the header's "one pass"), stated once for fit_pass (k_fit.hip) and k_shape_accumulate
// (k_fit_shape.hip).  Expanded in the body of the loop over the points: the point v[3] and its normal nm[3] (doubles) are posed
// by (scale, R[9], t[3]), culled behind z = 1 and where they face away, projected by K[9], matched with the depth pixel of
// `frame` (row length w; dw, dh: the frame's size as doubles) they fall on, and gated.  A point that takes no part `continue`s
// the loop; past the expansion p[3], n[3] (the posed point and normal) and res = c * (d / p.z - 1) are in scope.  A macro, so
// that both kernels compile from the very tokens: every parenthesis is the contract, and NaN fails every test.
// It is a run of statements with `continue`s in it, so it must be expanded directly in the body of the loop over the points
// (not in a nested loop, a lambda or a braceless if).  Besides p, n and res it declares, in that body's scope, sv0, sv1, sv2,
// c, r, x, y, px, py, di, d and gap: the caller can declare none of these names there before or after the expansion.
#define DH_FIT_CORRESPOND(v, nm, scale, R, t, K, frame, w, dw, dh, gate)                                                       \
    const double sv0 = (v)[0] * (scale), sv1 = (v)[1] * (scale), sv2 = (v)[2] * (scale);                                       \
    double p[3], n[3];                                                                                                         \
    _Pragma("unroll") for (int j = 0; j < 3; ++j) {                                                                            \
        p[j] = (((R)[3 * j] * sv0 + (R)[3 * j + 1] * sv1) + (R)[3 * j + 2] * sv2) + (t)[j];                                    \
        n[j] = ((R)[3 * j] * (nm)[0] + (R)[3 * j + 1] * (nm)[1]) + (R)[3 * j + 2] * (nm)[2];                                   \
    }                                                                                                                          \
    if (!(p[2] >= 1.0)) continue;                                                                                              \
    const double c = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2];                                                                \
    if (!(c < 0.0)) continue;                                                                                                  \
    double r[3];                                                                                                               \
    _Pragma("unroll") for (int j = 0; j < 3; ++j) r[j] = (p[0] * (K)[3 * j] + p[1] * (K)[3 * j + 1]) + p[2] * (K)[3 * j + 2];  \
    const double x = r[0] / r[2], y = r[1] / r[2];                                                                             \
    if (!(x >= 0.0 && x < (dw) && y >= 0.0 && y < (dh))) continue;                                                             \
    const int px = (int)x, py = (int)y; /* 0 <= px < w, 0 <= py < h */                                                         \
    const uint32_t di = (frame)[(size_t)py * (w) + px];                                                                        \
    if (di == 0) continue;                                                                                                     \
    const double d = (double)di;                                                                                               \
    const double gap = d - p[2];                                                                                               \
    if (!((gap < 0.0 ? -gap : gap) <= (gate))) continue;                                                                       \
    const double res = c * (d / p[2] - 1.0)

// A step's system from sums laid out as the upper triangle of a W x W matrix (DH_FIT_PAIR) with b at b_offset: damped, solved on
// its leading N x N block into x[0 .. N - 1].  false: a pivot was not > 0.0, and x is left as it was.
template <int N, int W>
__device__ __forceinline__ bool fit_solve_tri(const unsigned long long *sums, int b_offset, double lam1, double *x) {
    double A[N][N], b[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = i; j < N; ++j) {
            const double v = (double)(long long)sums[DH_FIT_PAIR(W, i, j)] / DH_FIT_S;
            A[i][j] = v; A[j][i] = v;
        }
        A[i][i] = A[i][i] * lam1 + 1e-9;
        b[i] = (double)(long long)sums[b_offset + i] / DH_FIT_S;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double piv = A[k][k];
        ok = ok && piv > 0.0;                      // (in the fit uniform over the workgroup: every lane holds the same numbers)
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double f = A[i][k] / piv;
#pragma unroll
            for (int j = k + 1; j < N; ++j) A[i][j] = A[i][j] - f * A[k][j];
            b[i] = b[i] - f * b[k];
        }
    }
    if (!ok) return false;                         // (what was computed past a bad pivot is dropped)
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int j = i + 1; j < N; ++j) s = s - A[i][j] * x[j];
        x[i] = s / A[i][i];
    }
    return true;
}

// A value that every lane of the workgroup holds alike, moved to scalar registers.
__device__ __forceinline__ double uni(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// A double from lane (this lane ^ o) of the wave (the decide kernels of k_ident.hip and k_ident_views.hip merge their picks with it).
__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)b, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(b >> 32), o);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- the shape step's accumulation (k_fit_shape.hip, k_fit_shape_views.hip and k_subjects.hip; DESIGN.md sections 20, 23 and 25)
// Whether instance `in` of a single-view step (k_shape_accumulate, k_shape_accumulate_subjects) takes part: the header's per-instance refusals, decided on the device (a NaN fails each test).
__device__ __forceinline__ bool shape_takes_part(const ShapeArgs &a, const dh_render_instance *in, uint32_t subject) {
    if (subject >= a.n_subjects) return false;                       // DH_SHAPE_SKIP among them
    if (in->frame >= (uint32_t)a.n) return false;
    return dh_fit_instance_fault(*in, a.radius, a.largest).why == DH_FIT_INST_OK;
}

// What one workgroup of DH_SHAPE_THREADS lanes adds to the row of `subject`: the tail of both accumulate kernels, a macro as
// DH_FIT_CORRESPOND is, so that both compile from the very tokens.  a: the ShapeArgs; NK: the fields, a compile-time constant;
// frame, K[9], R[9], t[3], scale: the depth frame and the camera pose the points are posed by (doubles, uniform over the
// workgroup; the multi-view step passes the composite of a view); s_part: the kernel's own __shared__ long long
// [DH_SHAPE_THREADS / 64][DH_SHAPE_STRIDE].  Lanes stride over the model's points: the correspondence, then sb, w and J_k in the
// header's operation order and the products into int64 partial sums in registers.  The sums are reduced across the wave with
// shuffles, across the four waves through LDS, and one 64-bit global atomic add per word and workgroup lands them in the row;
// `used` grows by one where the workgroup passed a point.  It returns from the kernel: nothing may follow the expansion.
// It is a run of statements expanded in the kernel's outermost scope and it claims names there: besides what
// DH_FIT_CORRESPOND declares in the loop body it declares NA, dw, dh, gate, accA, accB, e, cnt, np, wave, lead, word, row,
// mine and s, and in inner scopes i, v, nm, J, q, k, l, c, se, sc, base and wv.  The kernel can use none of these names for
// anything the expansion has to see (its arguments are evaluated inside it), so the kernels call their argument block `a`
// (or bind `a` to the ShapeArgs inside it) and their own locals by other names.
#define DH_SHAPE_BLOCK(a, NK, frame, K, R, t, scale, subject, s_part)                                                          \
    constexpr int NA = (NK) * ((NK) + 1) / 2;                                                                                  \
    const double dw = (double)(a).w, dh = (double)(a).h, gate = (a).gate;                                                      \
    long long accA[NA], accB[NK], e = 0, cnt = 0;                                                                              \
    _Pragma("unroll") for (int k = 0; k < NA; ++k) accA[k] = 0;                                                                \
    _Pragma("unroll") for (int k = 0; k < (NK); ++k) accB[k] = 0;                                                              \
    const size_t np = (a).np;                                                                                                  \
    for (uint32_t i = threadIdx.x; i < (a).np; i += DH_SHAPE_THREADS) {                                                        \
        double v[3], nm[3];                                                                                                    \
        _Pragma("unroll") for (int c = 0; c < 3; ++c) {                                                                        \
            v[c] = (double)(a).pts[(size_t)i * 3 + c];                                                                         \
            nm[c] = (double)(a).nrm[(size_t)i * 3 + c];                                                                        \
        }                                                                                                                      \
        DH_FIT_CORRESPOND(v, nm, scale, R, t, K, frame, (a).w, dw, dh, gate);                                                  \
        double J[NK];                                                                                                          \
        _Pragma("unroll") for (int k = 0; k < (NK); ++k) {                                                                     \
            const float *plane = (a).basis + (size_t)k * 3 * np + i;                                                           \
            const double sb0 = (double)plane[0] * (scale), sb1 = (double)plane[np] * (scale), sb2 = (double)plane[2 * np] * (scale); \
            const double w0 = ((R)[0] * sb0 + (R)[1] * sb1) + (R)[2] * sb2;                                                    \
            const double w1 = ((R)[3] * sb0 + (R)[4] * sb1) + (R)[5] * sb2;                                                    \
            const double w2 = ((R)[6] * sb0 + (R)[7] * sb1) + (R)[8] * sb2;                                                    \
            J[k] = (n[0] * w0 + n[1] * w1) + n[2] * w2;                                                                        \
        }                                                                                                                      \
        int q = 0;                                                                                                             \
        _Pragma("unroll") for (int k = 0; k < (NK); ++k) {                                                                     \
            _Pragma("unroll") for (int l = k; l < (NK); ++l) accA[q++] += (long long)((J[k] * J[l]) * DH_FIT_S);               \
            accB[k] += (long long)((J[k] * res) * DH_FIT_S);                                                                   \
        }                                                                                                                      \
        e += (long long)((res * res) * DH_FIT_S);                                                                              \
        cnt += 1;                                                                                                              \
    }                                                                                                                          \
    /* ---- across the wave in registers, across the waves in LDS, then one global atomic per sum */                          \
    const int wave = threadIdx.x >> 6;                                                                                         \
    const bool lead = (threadIdx.x & 63) == 0;                                                                                 \
    {                                                                                                                          \
        int q = 0;                                                                                                             \
        _Pragma("unroll") for (int k = 0; k < (NK); ++k) {                                                                     \
            _Pragma("unroll") for (int l = k; l < (NK); ++l) {                                                                 \
                const long long s = (long long)wave_sum_u64((uint64_t)accA[q++]);                                              \
                if (lead) (s_part)[wave][DH_FIT_PAIR(8, k, l)] = s;                                                            \
            }                                                                                                                  \
            const long long s = (long long)wave_sum_u64((uint64_t)accB[k]);                                                    \
            if (lead) (s_part)[wave][DH_SHAPE_B + k] = s;                                                                      \
        }                                                                                                                      \
        const long long se = (long long)wave_sum_u64((uint64_t)e), sc = (long long)wave_sum_u64((uint64_t)cnt);                \
        if (lead) { (s_part)[wave][DH_SHAPE_E] = se; (s_part)[wave][DH_SHAPE_COUNT] = sc; }                                    \
    }                                                                                                                          \
    __syncthreads();                                                                                                           \
    const int word = threadIdx.x;                                                                                              \
    if (word > DH_SHAPE_USED) return;                                                                                          \
    unsigned long long *row = (a).sums + (size_t)(subject) * DH_SHAPE_STRIDE;                                                  \
    if (word == DH_SHAPE_USED) {                                                                                               \
        long long c = 0;                                                                                                       \
        _Pragma("unroll") for (int wv = 0; wv < DH_SHAPE_THREADS / 64; ++wv) c += (s_part)[wv][DH_SHAPE_COUNT];                \
        if (c > 0) atomicAdd(&row[DH_SHAPE_USED], 1ull);                                                                       \
        return;                                                                                                                \
    }                                                                                                                          \
    /* a word of A that this K does not use was never written: the words of an NK x NK block are those with l < NK */          \
    bool mine = word >= DH_SHAPE_E;                                                                                            \
    if (word >= DH_SHAPE_B && word < DH_SHAPE_E) mine = word - DH_SHAPE_B < (NK);                                              \
    if (word < DH_SHAPE_B) {                                                                                                   \
        int k = 0, base = 0;                                                                                                   \
        while (word >= base + (8 - k)) { base += 8 - k; ++k; } /* row k of the 8 x 8 upper triangle starts at `base` */        \
        mine = k < (NK) && k + (word - base) < (NK);                                                                           \
    }                                                                                                                          \
    if (!mine) return;                                                                                                         \
    long long s = 0;                                                                                                           \
    _Pragma("unroll") for (int wv = 0; wv < DH_SHAPE_THREADS / 64; ++wv) s += (s_part)[wv][word];                              \
    atomicAdd(&row[word], (unsigned long long)s)

// ---- the fit's pose, pass modes and step helpers (k_fit.hip and k_fit_views.hip; DESIGN.md sections 18 and 21)
#define FIT_COARSE 0
#define FIT_FULL 1
#define FIT_LAST 2
// The pose a fit carries in registers (the multi-view fit: the world pose).
struct FitPose {
    double R[9];
    double t[3];
};

// The step's early exit: every one of the first n elements of x is below 1e-6 in magnitude.
__device__ __forceinline__ bool fit_small(const double x[6], int n) {
    bool small = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (i < n) small = small && ((x[i] < 0.0 ? -x[i] : x[i]) < 1e-6);
    return small;
}

// R = C R with C the Cayley rotation of a = w / 2 (the element order of the header)
__device__ __forceinline__ void fit_cayley(double R[9], const double w[3]) {
    const double a0 = w[0] / 2.0, a1 = w[1] / 2.0, a2 = w[2] / 2.0;
    const double q = (a0 * a0 + a1 * a1) + a2 * a2;
    const double s = 1.0 + q, d = 1.0 - q;
    const double u0 = 2.0 * a0, u1 = 2.0 * a1, u2 = 2.0 * a2;
    double C[9];
    C[0] = (d + u0 * a0) / s;  C[1] = (u0 * a1 - u2) / s; C[2] = (u0 * a2 + u1) / s;
    C[3] = (u1 * a0 + u2) / s; C[4] = (d + u1 * a1) / s;  C[5] = (u1 * a2 - u0) / s;
    C[6] = (u2 * a0 - u1) / s; C[7] = (u2 * a1 + u0) / s; C[8] = (d + u2 * a2) / s;
    double o[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (C[3 * i] * R[j] + C[3 * i + 1] * R[3 + j]) + C[3 * i + 2] * R[6 + j];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = o[i];
}

// ---- the single-view fit's pass (k_fit.hip and k_ident.hip; DESIGN.md sections 18 and 27)
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

// ---- a pair of the identification (k_ident.hip and k_subject_track.hip; DESIGN.md sections 27 and 29)
// Whether instance `in` (number i) takes part: the rule of dh_fit_shape_subjects* without a subject (a NaN fails each test).
__device__ __forceinline__ bool ident_takes_part(const IdentArgs &q, const dh_render_instance *in, uint32_t i) {
    if (in->frame >= (uint32_t)q.f.n) return false;
    if (q.fit_rec && q.fit_rec[i].status != DH_FIT_OK) return false;
    return dh_fit_instance_fault(*in, q.radius, q.largest).why == DH_FIT_INST_OK;
}

// One pair's refit: the full steps of k_fit's schedule (no coarse ones), then the last pass; the score and the pose written by lane 0.
template <bool STAGED>
__device__ __forceinline__ void ident_run(const IdentArgs &q, const dh_render_instance *in, const FitModel &m, const float *s_pts,
                                          unsigned long long *s_sum, size_t pair) {
    const FitArgs &a = q.f;
    const uint32_t fr = in->frame;
    const uint16_t *frame = a.frames + (size_t)fr * a.h * a.w;
    double K[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) K[c] = (double)(a.cams ? a.cams[fr].k[c] : a.k[c]);
    FitPose pose;
#pragma unroll
    for (int c = 0; c < 9; ++c) pose.R[c] = (double)in->R[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) pose.t[c] = (double)in->t[c];
    const double scale = (double)in->scale;
    uint32_t steps = 0, status = DH_FIT_OK;
    for (uint32_t it = 0; it < a.full; ++it) {
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
        dh_fit_record rec;
        rec.points = (uint32_t)s_sum[DH_FIT_COUNT];
        rec.steps = steps;
        rec.status = status;
        rec.reserved = 0;
        rec.sum_r2_fixed = (int64_t)s_sum[DH_FIT_E];
        q.score[pair] = rec;
        float *o = q.pose + pair * 12;
#pragma unroll
        for (int c = 0; c < 9; ++c) o[c] = (float)pose.R[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[9 + c] = (float)pose.t[c];
    }
}

// ---- the multi-view fit's pass (k_fit_views.hip and k_ident_views.hip; DESIGN.md sections 21 and 28)
// One pass at the world pose `pose` with gate `gate` over the views of `mask` (bit k: camera first_cam + k): the sums of MODE
// into s_sum (zeroed here; valid for every lane after the return).
template <int MODE, bool STAGED>
__device__ __forceinline__ void fit_views_pass(const FitViewsArgs &a, const FitModel &m, const float *s_pts, uint32_t first_cam, uint64_t mask,
                                               double scale, const FitPose &pose, double gate, unsigned long long *s_sum) {
    constexpr int NJ = MODE == FIT_COARSE ? 3 : MODE == FIT_FULL ? 6 : 0;
    constexpr int NA = NJ * (NJ + 1) / 2;
    long long accA[NA > 0 ? NA : 1], accB[NJ > 0 ? NJ : 1];
#pragma unroll
    for (int k = 0; k < (NA > 0 ? NA : 1); ++k) accA[k] = 0;
#pragma unroll
    for (int k = 0; k < (NJ > 0 ? NJ : 1); ++k) accB[k] = 0;
    long long e = 0, cnt = 0;
    uint64_t used = 0;                             // (uniform over the wave)
    __syncthreads();                               // every lane has read the sums of the pass before
    if (threadIdx.x < 32) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const double dw = (double)a.w, dh = (double)a.h;
    for (uint64_t rest = mask; rest; rest &= rest - 1) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(rest);
        const uint32_t cam = first_cam + bit;      // < a.n: the host refused the call otherwise
        const uint16_t *frame = a.frames + (size_t)cam * a.h * a.w;
        const FitView *vw = a.views + cam;
        double V[9], K[9], Rv[9], tv[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            V[q] = uni((double)vw->V[q]);
            K[q] = uni((double)a.cams[cam].k[q]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Rv[3 * i + j] = uni((V[3 * i] * pose.R[j] + V[3 * i + 1] * pose.R[3 + j]) + V[3 * i + 2] * pose.R[6 + j]);
            tv[i] = uni(((V[3 * i] * pose.t[0] + V[3 * i + 1] * pose.t[1]) + V[3 * i + 2] * pose.t[2]) + (double)vw->u[i]);
        }
        const long long before = cnt;
        for (uint32_t i = threadIdx.x; i < m.n; i += DH_FIT_THREADS) {
            double v[3], nm[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                v[ax] = (double)(STAGED ? s_pts[ax * DH_FIT_LDS_POINTS + i] : m.pts[(size_t)i * 3 + ax]);
                nm[ax] = (double)(STAGED ? s_pts[(3 + ax) * DH_FIT_LDS_POINTS + i] : m.nrm[(size_t)i * 3 + ax]);
            }
            DH_FIT_CORRESPOND(v, nm, scale, Rv, tv, K, frame, a.w, dw, dh, gate);
            if (MODE == FIT_LAST) e += (long long)((res * res) * DH_FIT_S);
            else {
                double J[6];
#pragma unroll
                for (int j = 0; j < 3; ++j) J[j] = (V[j] * n[0] + V[3 + j] * n[1]) + V[6 + j] * n[2];
                if (MODE == FIT_FULL) {
                    const double q0 = p[0] - tv[0], q1 = p[1] - tv[1], q2 = p[2] - tv[2];
                    const double m0 = q1 * n[2] - q2 * n[1];
                    const double m1 = q2 * n[0] - q0 * n[2];
                    const double m2 = q0 * n[1] - q1 * n[0];
#pragma unroll
                    for (int j = 0; j < 3; ++j) J[3 + j] = (V[j] * m0 + V[3 + j] * m1) + V[6 + j] * m2;
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
        if (MODE == FIT_LAST && __ballot(cnt != before) != 0) used |= 1ull << bit;
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
        if (lead) {
            atomicAdd(&s_sum[DH_FIT_E], s);
            atomicOr(&s_sum[DH_FIT_USED], (unsigned long long)used);
        }
    }
    {
        const unsigned long long s = wave_sum_u64((uint64_t)cnt);
        if (lead) atomicAdd(&s_sum[DH_FIT_COUNT], s);
    }
    __syncthreads();
}

// ---- a pair of the multi-view identification (k_ident_views.hip and k_rig_subject_track.hip; DESIGN.md sections 28 and 30)
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

// ---- the decision of an identification by one wave (k_ident_decide, k_ident_views_decide, k_subject_track_bind and
// k_rig_subject_bind; DESIGN.md sections 27 - 30).  row: the instance's n_subjects scores (Score: dh_fit_record or
// dh_view_fit_record; a pair that did not run holds zeros: 0 points, never eligible); part: whether the instance takes part
// (uniform over the wave).  Lanes stride over the candidates with dh_fit.h's picks, the picks are merged by an xor butterfly, and
// every lane returns the instance's dh_ident_record.
template <typename Score>
__device__ __forceinline__ dh_ident_record ident_decide(const Score *row, uint32_t n_subjects, uint32_t min_points, bool part, double max_ms,
                                                        double min_ratio) {
    IdentPick pick = dh_ident_pick_none();
    uint32_t eligible = 0;
    if (part)
        for (uint32_t sj = threadIdx.x; sj < n_subjects; sj += DH_IDENT_THREADS) {
            const Score r = row[sj];
            if (r.status != DH_FIT_OK || r.points < min_points) continue;
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
    dh_ident_record rec;
    rec.status = part ? dh_ident_status(eligible, pick.m_best, pick.m_second, max_ms, min_ratio) : DH_IDENT_SKIPPED;
    rec.best = pick.best; rec.second = pick.second;
    rec.eligible = eligible;
    rec.points_best = 0; rec.points_second = 0; rec.sum_r2_best = 0; rec.sum_r2_second = 0;
    if (pick.best != DH_IDENT_UNKNOWN) { rec.points_best = row[pick.best].points; rec.sum_r2_best = row[pick.best].sum_r2_fixed; }
    if (pick.second != DH_IDENT_UNKNOWN) { rec.points_second = row[pick.second].points; rec.sum_r2_second = row[pick.second].sum_r2_fixed; }
    return rec;
}
// The record of an instance for which no identification ran.
__device__ __forceinline__ dh_ident_record ident_skipped() {
    dh_ident_record rec;
    rec.status = DH_IDENT_SKIPPED; rec.best = 0; rec.second = 0; rec.eligible = 0;
    rec.points_best = 0; rec.points_second = 0; rec.sum_r2_best = 0; rec.sum_r2_second = 0;
    return rec;
}

// ---- the trackers' rule (k_fit_track.hip: one lane per camera; k_rig_fit_track.hip: one lane per slot of a rig; DESIGN.md
// sections 19 and 22).  State: dh_fit_track_state or dh_rig_fit_state; Instance: dh_render_instance or dh_view_instance.
__device__ __forceinline__ uint32_t fit_sat_inc(uint32_t v) { return dh_sat_inc(v); }

// o = A B, each element as (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]
__device__ __forceinline__ void fit_mat3_mul(const double A[9], const double B[9], double o[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// The forest's rotation as a matrix: each of the three angles picks its cosine and sine from the 120-entry table `angles`
// ([120][2]: cos, sin), and R = X (Y Z) in f64.  The caller casts it.
__device__ __forceinline__ void fit_track_rotation(const double rotation[3], const double *angles, double R[9]) {
    double cs[3], sn[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double x = rotation[j] / 3.14159 * 60.0 + 60.5;
        const int ri = !(x >= 0.0) ? 0 : x >= 119.0 ? 119 : (int)x;
        cs[j] = angles[2 * ri]; sn[j] = angles[2 * ri + 1];
    }
    const double Z[9] = {cs[0], sn[0], 0.0, -sn[0], cs[0], 0.0, 0.0, 0.0, 1.0};
    const double Y[9] = {cs[1], 0.0, sn[1], 0.0, 1.0, 0.0, -sn[1], 0.0, cs[1]};
    const double X[9] = {1.0, 0.0, 0.0, 0.0, cs[2], -sn[2], 0.0, sn[2], cs[2]};
    double M[9];
    fit_mat3_mul(Y, Z, M);
    fit_mat3_mul(X, M, R);
}

// The carried start: the state's R, and its t moved on at constant velocity where the tracker's flags ask for it and the state
// has a step before its last.
template <typename State, typename Instance>
__device__ __forceinline__ void fit_track_carried_start(const State &st, uint32_t flags, Instance &in) {
#pragma unroll
    for (int q = 0; q < 9; ++q) in.R[q] = st.R[q];
    const bool motion = (flags & DH_FIT_TRACK_MOTION) && st.have_prev;
#pragma unroll
    for (int q = 0; q < 3; ++q) in.t[q] = motion ? st.t[q] + (st.t[q] - st.t_prev[q]) : st.t[q];
}

// Why a fit is not accepted, from its record alone (DH_FIT_TRACK_BAD_STATUS | BAD_POINTS | BAD_RMS; 0: nothing).
// Record: dh_fit_record or dh_view_fit_record.
template <typename Record>
__device__ __forceinline__ uint32_t fit_track_why(const Record &fr, uint32_t keep_points, int64_t rms_lim) {
    uint32_t why = 0;
    if (fr.status != DH_FIT_OK) why |= DH_FIT_TRACK_BAD_STATUS;
    if (fr.points < keep_points) why |= DH_FIT_TRACK_BAD_POINTS;
    if (fr.sum_r2_fixed > rms_lim * (long long)fr.points) why |= DH_FIT_TRACK_BAD_RMS;
    return why;
}

// DH_FIT_TRACK_BAD_JUMP where the fitted midpoint lies further than sqrt(jump2) from the detection's (NaN fails), else 0.
__device__ __forceinline__ uint32_t fit_track_jump(const float fitted[3], const float detected[3], double jump2) {
    const double dx = (double)fitted[0] - (double)detected[0], dy = (double)fitted[1] - (double)detected[1],
                 dz = (double)fitted[2] - (double)detected[2];
    return !((dx * dx + dy * dy) + dz * dz <= jump2) ? DH_FIT_TRACK_BAD_JUMP : 0u;
}

// The state after an accepted fit (a macro, as DH_FIT_CORRESPOND is), and after a rejected one.
#define DH_FIT_TRACK_ACCEPT(st, fit)                                                                                           \
    do {                                                                                                                       \
        _Pragma("unroll") for (int q = 0; q < 3; ++q) { (st).t_prev[q] = (st).t[q]; (st).t[q] = (fit).t[q]; }                  \
        _Pragma("unroll") for (int q = 0; q < 9; ++q) (st).R[q] = (fit).R[q];                                                  \
        (st).have_prev = (st).tracked;                                                                                         \
        (st).tracked = 1;                                                                                                      \
        (st).age = fit_sat_inc((st).age);                                                                                      \
        (st).lost = 0;                                                                                                         \
    } while (0)
template <typename State>
__device__ __forceinline__ void fit_track_reject(State &st) {
    st.tracked = 0; st.have_prev = 0; st.age = 0;
    st.lost = fit_sat_inc(st.lost);
}

// ---- the seed of one rig (k_rig_fit_seed and k_rig_subject_seed; DESIGN.md sections 22 and 30): section 22's steps 0 - 2 by the
// one workgroup of DH_RIG_FIT_THREADS lanes of rig blockIdx.x (the grid is n_rigs).  s_st, s_p, s_role, s_who: the kernel's own
// __shared__ arrays of DH_RIG_MAX_TRACKS entries, DH_RIG_MAX_PERSONS persons and two words per slot.  The rig's entries and persons
// are copied to LDS, lane 0 binds persons to entries (dh_rig_fit_bind, dh_rig_fit.h), then one lane per slot composes the slot's
// start instance, its schedule and its kind.  model_of(slot, old, st, role) gives the start's `model`: old points at the entry as
// it stood before the bind (still in global memory), st is what the bind made of it, role the slot's DH_RIG_FIT_*.
template <typename ModelOf>
__device__ __forceinline__ void rig_fit_seed_rig(const RigFitArgs &a, dh_rig_fit_state *s_st, dh_rig_person *s_p, uint32_t *s_role, uint32_t *s_who,
                                                 ModelOf model_of) {
    const int g = blockIdx.x, lane = threadIdx.x;                  // g < n_rigs: the grid is n_rigs
    const int c0 = a.rig_begin[g], nc = a.rig_begin[g + 1] - c0;   // 1 .. DH_RIG_MAX_CAMERAS cameras (dh_rig_create)
    // pm: one present camera per lane (nc <= 64 = the lanes of the one wave)
    const bool here = lane < nc && (!a.present || a.present[c0 + lane] != 0);
    const uint64_t pm = __ballot(here);
    const size_t slot = (size_t)g * DH_RIG_MAX_TRACKS + lane;
    if (pm == 0) {                                                 // (uniform) step 0: the state is kept
        if (lane < DH_RIG_MAX_TRACKS) {
            a.seed[slot] = DH_FIT_SEED_ABSENT;
            a.who[slot] = DH_RIG_FIT_NO_PERSON;
            a.sched[2 * slot] = 0; a.sched[2 * slot + 1] = 0;
        }
        return;
    }
    dh_rig_fit_state *gst = a.state + (size_t)g * DH_RIG_MAX_TRACKS;
    {
        const uint32_t *src = (const uint32_t *)gst;
        uint32_t *dst = (uint32_t *)s_st;
        for (uint32_t k = lane; k < DH_RIG_MAX_TRACKS * sizeof(dh_rig_fit_state) / 4; k += DH_RIG_FIT_THREADS) dst[k] = src[k];
        src = (const uint32_t *)(a.persons + (size_t)g * DH_RIG_MAX_PERSONS);
        dst = (uint32_t *)s_p;
        for (uint32_t k = lane; k < DH_RIG_MAX_PERSONS * sizeof(dh_rig_person) / 4; k += DH_RIG_FIT_THREADS) dst[k] = src[k];
    }
    __syncthreads();
    if (lane == 0) dh_rig_fit_bind(s_st, s_p, a.n_persons[g], a.n_heads, a.n_cams, a.max_heads, s_role, s_who);
    __syncthreads();
    if (lane >= DH_RIG_MAX_TRACKS) return;
    const uint32_t role = s_role[lane], pi = s_who[lane];
    const dh_rig_fit_state st = s_st[lane];
    dh_view_instance in;
    in.first_cam = (uint32_t)c0; in.model = model_of(slot, gst + lane, st, role); in.views = 0; in.scale = a.scale; in.flags = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) in.R[q] = 0.0f;
#pragma unroll
    for (int q = 0; q < 3; ++q) in.t[q] = 0.0f;
    uint32_t kind = DH_FIT_SEED_NONE, coarse = 0, full = 0;
    if (role != DH_RIG_FIT_UNUSED) {
        const bool seen = pi != DH_RIG_FIT_NO_PERSON;
        const bool entry = role != DH_RIG_FIT_UNBOUND;
        if (entry && st.tracked) {
            in.views = (st.views_used | (seen ? s_p[pi].views : 0ull)) & pm;
            if (in.views == 0) kind = DH_FIT_SEED_COAST;
            else {
                kind = DH_FIT_SEED_CARRIED;
                full = a.prm.iterations_tracked;
                fit_track_carried_start(st, a.flags, in);
            }
        } else {                                                   // detected: the slot has a person (the bind freed the rest)
            const dh_rig_person &p = s_p[pi];
            kind = DH_FIT_SEED_DETECTED;
            coarse = a.coarse; full = a.full;
            in.views = p.views & pm;
            // best_cam < n_cams and best_head < max_heads: the bind ignores every other person
            const dh_pose &po = a.heads[(size_t)p.best_cam * a.max_heads + p.best_head].pose;
            double R[9], Rh[9], V[9];
            fit_track_rotation(po.rotation, a.angles, R);
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                Rh[q] = (double)(float)R[q];
                V[q] = (double)a.views[p.best_cam].V[q];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) in.R[3 * i + j] = (float)((V[i] * Rh[j] + V[3 + i] * Rh[3 + j]) + V[6 + i] * Rh[6 + j]);
#pragma unroll
            for (int q = 0; q < 3; ++q) in.t[q] = p.world[q];
        }
        if (seen) kind |= DH_RIG_FIT_SEED_IS_SEEN;
        if (entry) kind |= DH_RIG_FIT_SEED_IS_ENTRY;
    }
    gst[lane] = st;                                                // what the bind made of the entry
    a.start[slot] = in;
    a.sched[2 * slot] = coarse; a.sched[2 * slot + 1] = full;
    a.seed[slot] = kind;
    a.who[slot] = pi;
}
