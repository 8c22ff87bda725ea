// k_surface.hip -- a surface per subject (the rule is stated in include/depthhead_hip.h, section "a surface per
// subject").  A surface set holds one offset per (subject, vertex) along the base mesh's vertex normal; the kernels here evaluate
// the offsets into the models and re-estimate them from fitted frames.
//   k_subjects_points_surface   k_subjects_points' tree (k_subjects.hip), then x = x + o_i * nb_i, rounded to f32 once.
//   k_surface_clear        zeroes the rows and tallies of the call's subjects.
//   k_surface_accumulate   one workgroup of 256 lanes per instance; an instance that takes no part leaves at once.  Lanes stride
//          over the points of the instance's subject's model: the fit's correspondence (DH_FIT_CORRESPOND, the very tokens), the
//          grazing test, J along the base normal, and three 64-bit integer atomics into the vertex's row -- no two lanes of a
//          workgroup hold the same vertex.  The subject's e and point count are reduced with shuffles, through LDS, and land with
//          one atomic per word and workgroup.
//   k_surface_solve        one workgroup per subject: the vertex's constants once, then `iterations` Jacobi sweeps between two
//          buffers with a barrier per sweep -- in LDS up to DH_SURFACE_LDS_POINTS vertices, in the set's scratch above, the same
//          arithmetic on both paths -- then the finite test, the clamp, the offsets and the record.  Nothing crosses workgroups.
// f64 with + - * /, compares and casts, every operation rounded on its own; int64 sums whose order is free: bit-identical run to
// run and to tests/surface_ref.py.
#include "dh_fit_device.h"

#pragma clang fp contract(off)

__global__ __launch_bounds__(DH_SUBJECTS_THREADS) void k_subjects_points_surface(const SurfacePointsArgs g) {
    const SubjectsArgs &a = g.a;
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
    const double o = g.offsets[(size_t)sj * n + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = v[c] + o * (double)g.nb[(size_t)i * 3 + c];
    float *out = a.models[sj].pts + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = (float)v[c];
}

__global__ __launch_bounds__(DH_SURFACE_THREADS) void k_surface_clear(unsigned long long *rows, uint32_t row_words, unsigned long long *tally, uint32_t tally_words) {
    const uint32_t i = blockIdx.x * DH_SURFACE_THREADS + threadIdx.x;
    if (i < row_words) rows[i] = 0;
    else if (i - row_words < tally_words) tally[i - row_words] = 0;
}

__global__ __launch_bounds__(DH_SURFACE_THREADS) void k_surface_accumulate(const SurfaceArgs g) {
    __shared__ long long s_part[DH_SURFACE_THREADS / 64][2];
    const dh_render_instance *in = g.s.inst + blockIdx.x;
    const uint32_t subject = g.s.subjects ? g.s.subjects[blockIdx.x] : 0u;
    if (g.fit_rec && g.fit_rec[blockIdx.x].status != DH_FIT_OK) return;   // (uniform over the workgroup, as what follows)
    if (!shape_takes_part(g.s, in, subject)) return;
    const double scale = (double)in->scale;
    if (!((scale < 0.0 ? -scale : scale) <= DH_SURFACE_MAX_SCALE)) return;
    const uint32_t fr = in->frame;
    const uint16_t *frame = g.s.frames + (size_t)fr * g.s.h * g.s.w;
    double K[9], R[9], t[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) K[q] = (double)(g.s.cams ? g.s.cams[fr].k[q] : g.s.k[q]);
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = (double)in->R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = (double)in->t[q];
    const float *pts = g.models[subject].pts, *nrm = g.models[subject].nrm;
    const double dw = (double)g.s.w, dh = (double)g.s.h, gate = g.s.gate, min_cos2 = g.min_cos2;
    unsigned long long *rows = g.rows + (size_t)subject * g.s.np * DH_SURFACE_ROW;
    long long e = 0, cnt = 0;
    for (uint32_t i = threadIdx.x; i < g.s.np; i += DH_SURFACE_THREADS) {
        double v[3], nm[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            v[q] = (double)pts[(size_t)i * 3 + q];
            nm[q] = (double)nrm[(size_t)i * 3 + q];
        }
        DH_FIT_CORRESPOND(v, nm, scale, R, t, K, frame, g.s.w, dw, dh, gate);
        if (!(c * c >= min_cos2 * ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]))) continue;
        const double sb0 = (double)g.nb[(size_t)i * 3] * scale, sb1 = (double)g.nb[(size_t)i * 3 + 1] * scale, sb2 = (double)g.nb[(size_t)i * 3 + 2] * scale;
        const double w0 = (R[0] * sb0 + R[1] * sb1) + R[2] * sb2;
        const double w1 = (R[3] * sb0 + R[4] * sb1) + R[5] * sb2;
        const double w2 = (R[6] * sb0 + R[7] * sb1) + R[8] * sb2;
        const double J = (n[0] * w0 + n[1] * w1) + n[2] * w2;
        unsigned long long *row = rows + (size_t)i * DH_SURFACE_ROW;
        atomicAdd(&row[DH_SURFACE_A], (unsigned long long)(long long)((J * J) * DH_FIT_S));
        atomicAdd(&row[DH_SURFACE_B], (unsigned long long)(long long)((J * res) * DH_FIT_S));
        atomicAdd(&row[DH_SURFACE_CNT], 1ull);
        e += (long long)((res * res) * DH_FIT_S);
        cnt += 1;
    }
    // ---- the subject's words: across the wave in registers, across the waves in LDS, then one global atomic per word
    const int wave = threadIdx.x >> 6;
    const long long se = (long long)wave_sum_u64((uint64_t)e), sc = (long long)wave_sum_u64((uint64_t)cnt);
    if ((threadIdx.x & 63) == 0) { s_part[wave][0] = se; s_part[wave][1] = sc; }
    __syncthreads();
    if (threadIdx.x > 1) return;
    long long sum = 0;
#pragma unroll
    for (int wv = 0; wv < DH_SURFACE_THREADS / 64; ++wv) sum += s_part[wv][threadIdx.x];
    unsigned long long *tally = g.tally + (size_t)subject * DH_SURFACE_TALLY;
    if (threadIdx.x == 0) atomicAdd(&tally[DH_SURFACE_E], (unsigned long long)sum);
    else if (sum > 0) {
        atomicAdd(&tally[DH_SURFACE_POINTS], (unsigned long long)sum);
        atomicAdd(&tally[DH_SURFACE_USED], 1ull);
    }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = WAVE / 2; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// IN_LDS: u and u' are the kernel's dynamic LDS, [2][n] f64; else the subject's [2][n] of the set's scratch.
template <bool IN_LDS>
__global__ __launch_bounds__(DH_SURFACE_SOLVE_THREADS) void k_surface_solve(const SurfaceArgs g) {
    extern __shared__ double s_u[];
    __shared__ uint32_t s_count[3];                                   // observed, clamped, rejected
    __shared__ unsigned long long s_max;                              // the largest |o| as its bit pattern (monotone for values >= 0)
    const uint32_t sj = blockIdx.x;
    const uint32_t n = g.s.np;
    double *o = g.offsets + (size_t)sj * n;
    unsigned long long *rows = g.rows + (size_t)sj * n * DH_SURFACE_ROW;
    const unsigned long long *tally = g.tally + (size_t)sj * DH_SURFACE_TALLY;
    if (threadIdx.x == 0) {
        s_count[0] = 0; s_count[1] = 0; s_count[2] = 0; s_max = 0;
        g.state[sj].zero_normals = 0;                                 // (the normals pass that follows counts anew)
    }
    __syncthreads();
    const unsigned long long points = tally[DH_SURFACE_POINTS];
    const bool few = points < (unsigned long long)g.s.min_points;       // (uniform over the workgroup)
    uint32_t observed = 0, clamped = 0, rejected = 0;
    unsigned long long largest = 0;
    if (few) {
        for (uint32_t i = threadIdx.x; i < n; i += DH_SURFACE_SOLVE_THREADS) {
            const unsigned long long m = (unsigned long long)__double_as_longlong(o[i]) & 0x7fffffffffffffffull;
            largest = m > largest ? m : largest;
        }
    } else {
        double *u0, *u1;
        if constexpr (IN_LDS) { u0 = s_u; u1 = s_u + n; }
        else { u0 = g.scratch + (size_t)sj * 2 * n; u1 = u0 + n; }
        const double mu = g.mu, eps = g.eps;
        // ---- what no sweep changes, per vertex: (A o + B) and the denominator, kept in the row's spent words
        for (uint32_t i = threadIdx.x; i < n; i += DH_SURFACE_SOLVE_THREADS) {
            unsigned long long *row = rows + (size_t)i * DH_SURFACE_ROW;
            const bool seen = row[DH_SURFACE_CNT] >= (unsigned long long)g.min_count;
            const double A = seen ? (double)(long long)row[DH_SURFACE_A] / DH_FIT_S : 0.0;
            const double B = seen ? (double)(long long)row[DH_SURFACE_B] / DH_FIT_S : 0.0;
            const double oi = o[i];
            const uint32_t deg = g.nbr_begin[i + 1] - g.nbr_begin[i];
            row[DH_SURFACE_A] = (unsigned long long)__double_as_longlong(A * oi + B);
            row[DH_SURFACE_B] = (unsigned long long)__double_as_longlong((A + mu * (double)deg) + eps);
            u0[i] = oi;
            observed += seen ? 1u : 0u;
        }
        __syncthreads();
        // ---- Jacobi: every u' of a sweep from the u of the sweep before
        for (uint32_t it = 0; it < g.iterations; ++it) {
            const double *cur = (it & 1u) ? u1 : u0;
            double *nxt = (it & 1u) ? u0 : u1;
            for (uint32_t i = threadIdx.x; i < n; i += DH_SURFACE_SOLVE_THREADS) {
                const unsigned long long *row = rows + (size_t)i * DH_SURFACE_ROW;
                double sum = 0.0;
                const uint32_t end = g.nbr_begin[i + 1];
                for (uint32_t j = g.nbr_begin[i]; j < end; ++j) sum = sum + cur[g.nbr[j]];
                const double c0 = __longlong_as_double((long long)row[DH_SURFACE_A]), den = __longlong_as_double((long long)row[DH_SURFACE_B]);
                nxt[i] = (c0 + mu * sum) / den;
            }
            __syncthreads();
        }
        const double *fin = (g.iterations & 1u) ? u1 : u0;
        const double hi = g.max_offset;
        for (uint32_t i = threadIdx.x; i < n; i += DH_SURFACE_SOLVE_THREADS) {
            double u = fin[i];
            if (!(u - u == 0.0)) { u = o[i]; rejected += 1; }         // (x - x is 0.0 for a finite x alone)
            else {
                if (u > hi) { u = hi; clamped += 1; }
                if (u < -hi) { u = -hi; clamped += 1; }
            }
            o[i] = u;
            const unsigned long long m = (unsigned long long)__double_as_longlong(u) & 0x7fffffffffffffffull;
            largest = m > largest ? m : largest;
        }
    }
    // ---- the record: across the wave in registers, across the waves with integer atomics in LDS
    const uint64_t counts = wave_sum_u64((uint64_t)observed | ((uint64_t)clamped << 32));   // (each below 2^15: no carry between the halves)
    const uint32_t rej = (uint32_t)wave_sum_u64((uint64_t)rejected);
    largest = wave_max_u64(largest);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_count[0], (uint32_t)counts);
        atomicAdd(&s_count[1], (uint32_t)(counts >> 32));
        atomicAdd(&s_count[2], rej);
        atomicMax(&s_max, largest);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    dh_surface_record rec;
    rec.status = few ? DH_SURFACE_FEW_POINTS : DH_SURFACE_OK;
    rec.points = (uint32_t)points;
    rec.instances = (uint32_t)tally[DH_SURFACE_USED];
    rec.observed = s_count[0]; rec.clamped = s_count[1]; rec.rejected = s_count[2];
    rec.sum_r2_fixed = (int64_t)tally[DH_SURFACE_E];
    rec.max_abs = __longlong_as_double((long long)s_max);
    g.rec[sj] = rec;
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_subjects_update_surface(const SurfacePointsArgs &a, bool apply, hipStream_t s) {
    if (a.a.count == 0) return hipSuccess;
    if (apply) {
        const hipError_t e = dh_launch_subjects_apply(a.a, s);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((a.a.n + DH_SUBJECTS_THREADS - 1) / DH_SUBJECTS_THREADS, a.a.count);
    hipLaunchKernelGGL(k_subjects_points_surface, grid, dim3(DH_SUBJECTS_THREADS), 0, s, a);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : dh_launch_subjects_normals(a.a, s);
}
hipError_t dh_launch_surface_clear(const SurfaceArgs &a, hipStream_t s) {
    const uint32_t row_words = a.s.n_subjects * a.s.np * DH_SURFACE_ROW, tally_words = a.s.n_subjects * DH_SURFACE_TALLY;   // (at most 3 * 2^22 + 1024)
    if (row_words + tally_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_clear, dim3((row_words + tally_words + DH_SURFACE_THREADS - 1) / DH_SURFACE_THREADS), dim3(DH_SURFACE_THREADS), 0, s,
                       a.rows, row_words, a.tally, tally_words);
    return hipGetLastError();
}
hipError_t dh_launch_surface_accumulate(const SurfaceArgs &a, hipStream_t s) {
    if (a.s.n_inst == 0) return hipSuccess;
    hipLaunchKernelGGL(k_surface_accumulate, dim3(a.s.n_inst), dim3(DH_SURFACE_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_surface_solve(const SurfaceArgs &a, hipStream_t s) {
    if (a.s.n_subjects == 0) return hipSuccess;
    if (a.s.np > DH_SURFACE_LDS_POINTS) {
        hipLaunchKernelGGL(k_surface_solve<false>, dim3(a.s.n_subjects), dim3(DH_SURFACE_SOLVE_THREADS), 0, s, a);
        return hipGetLastError();
    }
    const size_t bytes = (size_t)a.s.np * 2 * sizeof(double);         // (dh_surface_solve_prepare allowed it when the set was made)
    hipLaunchKernelGGL(k_surface_solve<true>, dim3(a.s.n_subjects), dim3(DH_SURFACE_SOLVE_THREADS), bytes, s, a);
    return hipGetLastError();
}
hipError_t dh_surface_solve_prepare(uint32_t n) {
    if (n > DH_SURFACE_LDS_POINTS || (size_t)n * 2 * sizeof(double) <= 32768) return hipSuccess;
    // above the default limit of dynamic LDS the function must be told, on the current device
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_surface_solve<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(DH_SURFACE_LDS_POINTS * 2 * sizeof(double)));
}
