// k_fit_shape.hip -- one Gauss-Newton step of a model's shape coefficients over the fitted instances of each subject (DESIGN.md
// section 20; the rule is stated in include/depthhead_hip.h, section "adapting a model's shape to a subject").  Three kernels:
//   k_shape_accumulate  one workgroup of 256 lanes per instance; an instance that takes no part leaves at once.  Lanes stride
//          over the model's points: the fit's one pass (transform, project, gather the depth pixel, gate, residual), then the
//          point's K shape derivatives and its products into int64 partial sums in registers.  A single pass reads every model
//          and basis value once, so nothing is staged in LDS; the basis lies one plane per field and axis, so a wave reads
//          consecutive words.  The sums are reduced across the wave with 64-bit shuffles, across the four waves through LDS,
//          and one 64-bit global atomic add per sum and workgroup lands them in the subject's row.
//   k_shape_clear       zeroes the rows of the call's subjects, before the accumulation on the same stream.
//   k_shape_solve       one lane per subject: damping, elimination, back substitution, the record.
// K is a template argument (1 .. 8): every array is indexed at compile time and stays in registers.
// f64 with + - * /, compares and casts only, every operation rounded on its own; int64 sums whose order is free: bit-identical
// run to run and to tests/shape_ref.py.
#include "dh_device.h"
#include "dh_fit.h"

#pragma clang fp contract(off)

__device__ __forceinline__ long long shape_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Whether instance `in` takes part: the header's per-instance refusals, decided on the device (a NaN fails each test).
__device__ __forceinline__ bool shape_takes_part(const ShapeArgs &a, const dh_render_instance *in, uint32_t subject) {
    if (subject >= a.n_subjects) return false;                       // DH_SHAPE_SKIP among them
    if (in->frame >= (uint32_t)a.n) return false;
    const double sc = (double)in->scale;
    const double as = sc < 0.0 ? -sc : sc;
    if (!(as * a.radius <= DH_FIT_MAX_EXTENT) || !(as * a.largest <= DH_SHAPE_MAX_FIELD)) return false;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double t = (double)in->t[q];
        ok = ok && (t - t == 0.0);                                   // finite
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double g = ((double)in->R[3 * i] * (double)in->R[3 * j] + (double)in->R[3 * i + 1] * (double)in->R[3 * j + 1]) +
                             (double)in->R[3 * i + 2] * (double)in->R[3 * j + 2];
            const double d = g - (i == j ? 1.0 : 0.0);
            ok = ok && ((d < 0.0 ? -d : d) <= DH_FIT_R_TOLERANCE);
        }
    return ok;
}

template <int NK>
__global__ __launch_bounds__(DH_SHAPE_THREADS) void k_shape_accumulate(const ShapeArgs a) {
    constexpr int NA = NK * (NK + 1) / 2;
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
    const double dw = (double)a.w, dh = (double)a.h, gate = a.gate;
    long long accA[NA], accB[NK], e = 0, cnt = 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) accA[k] = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) accB[k] = 0;
    const size_t np = a.np;
    for (uint32_t i = threadIdx.x; i < a.np; i += DH_SHAPE_THREADS) {
        double v[3], nm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = (double)a.pts[(size_t)i * 3 + c];
            nm[c] = (double)a.nrm[(size_t)i * 3 + c];
        }
        const double sv0 = v[0] * scale, sv1 = v[1] * scale, sv2 = v[2] * scale;
        double p[3], n[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            p[j] = ((R[3 * j] * sv0 + R[3 * j + 1] * sv1) + R[3 * j + 2] * sv2) + t[j];
            n[j] = (R[3 * j] * nm[0] + R[3 * j + 1] * nm[1]) + R[3 * j + 2] * nm[2];
        }
        if (!(p[2] >= 1.0)) continue;
        const double c = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2];
        if (!(c < 0.0)) continue;
        double r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[j] = (p[0] * K[3 * j] + p[1] * K[3 * j + 1]) + p[2] * K[3 * j + 2];
        const double x = r[0] / r[2], y = r[1] / r[2];
        if (!(x >= 0.0 && x < dw && y >= 0.0 && y < dh)) continue;          // (NaN fails)
        const int px = (int)x, py = (int)y;                                 // 0 <= px < w, 0 <= py < h
        const uint32_t di = frame[(size_t)py * a.w + px];
        if (di == 0) continue;
        const double d = (double)di;
        const double gap = d - p[2];
        if (!((gap < 0.0 ? -gap : gap) <= gate)) continue;
        const double res = c * (d / p[2] - 1.0);
        double J[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float *plane = a.basis + (size_t)k * 3 * np + i;
            const double sb0 = (double)plane[0] * scale, sb1 = (double)plane[np] * scale, sb2 = (double)plane[2 * np] * scale;
            const double w0 = (R[0] * sb0 + R[1] * sb1) + R[2] * sb2;
            const double w1 = (R[3] * sb0 + R[4] * sb1) + R[5] * sb2;
            const double w2 = (R[6] * sb0 + R[7] * sb1) + R[8] * sb2;
            J[k] = (n[0] * w0 + n[1] * w1) + n[2] * w2;
        }
        int q = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int l = k; l < NK; ++l) accA[q++] += (long long)((J[k] * J[l]) * DH_FIT_S);
            accB[k] += (long long)((J[k] * res) * DH_FIT_S);
        }
        e += (long long)((res * res) * DH_FIT_S);
        cnt += 1;
    }
    // ---- across the wave in registers, across the waves in LDS, then one global atomic per sum
    const int wave = threadIdx.x >> 6;
    const bool lead = (threadIdx.x & 63) == 0;
    {
        int q = 0;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
#pragma unroll
            for (int l = k; l < NK; ++l) {
                const long long s = shape_wave_sum(accA[q++]);
                if (lead) s_part[wave][DH_SHAPE_PAIR(k, l)] = s;
            }
            const long long s = shape_wave_sum(accB[k]);
            if (lead) s_part[wave][DH_SHAPE_B + k] = s;
        }
        const long long se = shape_wave_sum(e), sc = shape_wave_sum(cnt);
        if (lead) { s_part[wave][DH_SHAPE_E] = se; s_part[wave][DH_SHAPE_COUNT] = sc; }
    }
    __syncthreads();
    const int word = threadIdx.x;
    if (word > DH_SHAPE_USED) return;
    unsigned long long *row = a.sums + (size_t)subject * DH_SHAPE_STRIDE;
    if (word == DH_SHAPE_USED) {
        long long c = 0;
#pragma unroll
        for (int wv = 0; wv < DH_SHAPE_THREADS / 64; ++wv) c += s_part[wv][DH_SHAPE_COUNT];
        if (c > 0) atomicAdd(&row[DH_SHAPE_USED], 1ull);
        return;
    }
    // a word of A that this K does not use was never written: the words of an NK x NK block are those with l < NK
    bool mine = word >= DH_SHAPE_E;
    if (word >= DH_SHAPE_B && word < DH_SHAPE_E) mine = word - DH_SHAPE_B < NK;
    if (word < DH_SHAPE_B) {
        int k = 0, base = 0;
        while (word >= base + (8 - k)) { base += 8 - k; ++k; }          // row k of the 8 x 8 upper triangle starts at `base`
        mine = k < NK && k + (word - base) < NK;
    }
    if (!mine) return;
    long long s = 0;
#pragma unroll
    for (int wv = 0; wv < DH_SHAPE_THREADS / 64; ++wv) s += s_part[wv][word];
    atomicAdd(&row[word], (unsigned long long)s);
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
    else {
        double A[NK][NK], b[NK], x[NK];
#pragma unroll
        for (int i = 0; i < NK; ++i) {
#pragma unroll
            for (int j = i; j < NK; ++j) {
                const double v = (double)(long long)row[DH_SHAPE_PAIR(i, j)] / DH_FIT_S;
                A[i][j] = v; A[j][i] = v;
            }
            A[i][i] = A[i][i] * a.lam1 + 1e-9;
            b[i] = (double)(long long)row[DH_SHAPE_B + i] / DH_FIT_S;
        }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const double piv = A[k][k];
            ok = ok && piv > 0.0;
#pragma unroll
            for (int i = k + 1; i < NK; ++i) {
                const double f = A[i][k] / piv;
#pragma unroll
                for (int j = k + 1; j < NK; ++j) A[i][j] = A[i][j] - f * A[k][j];
                b[i] = b[i] - f * b[k];
            }
        }
        if (!ok) rec.status = DH_SHAPE_SINGULAR;                      // (what was computed past a bad pivot is dropped)
        else {
#pragma unroll
            for (int i = NK - 1; i >= 0; --i) {
                double s = b[i];
#pragma unroll
                for (int j = i + 1; j < NK; ++j) s = s - A[i][j] * x[j];
                x[i] = s / A[i][i];
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) rec.delta[k] = x[k];
        }
    }
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
