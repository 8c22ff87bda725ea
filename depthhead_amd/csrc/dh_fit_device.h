// dh_fit_device.h -- the device arithmetic that the fit (k_fit.hip, with its per-instance-schedule instance) and the shape step
// (k_fit_shape.hip) must agree on bit for bit, each stated once: the per-point correspondence and the damped solve.  f64 with
// + - * /, compares and casts only; every operation is rounded on its own, so the expression trees below are the contract
// (tests/fit_ref.py and tests/shape_ref.py restate them).  Not part of the ABI.
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
