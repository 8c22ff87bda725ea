// k_train.hip -- HoughLearning on the GPU (src/hough/prediction.rs:103-234, houghforest.rs:185-310): the window pass of
// sample extraction, the per-sample rectangle-sum images, and the breadth-first split search of every tree at once.
//
// One of the kernel translation units of libdepthhead_hip.so (gfx950, wave64).  The host half (validation, subset draws,
// early_stop, partitions, comp_leaf_data, assembly) is dh_train.cpp; dh_api.hip sequences the launches.
#include "dh_device.h"

// ================================================================== window pass
// Summed-area table modulo 2^32, S[y][x] = sum of rows < y, columns < x.  Any patch sum taken from it is exact while it
// is below 2^32, which dh_train_validate_ guarantees (W * H * 65535 < 2^32).
__global__ void __launch_bounds__(256) k_train_sat_rows(TrainWinArgs a) {
    const int f = blockIdx.y, y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y > a.h) return;
    uint32_t *S = a.sat + (size_t)f * (a.h + 1) * (a.w + 1) + (size_t)y * (a.w + 1);
    S[0] = 0;
    if (y == 0) {
        for (int x = 0; x < a.w; ++x) S[x + 1] = 0;
        return;
    }
    const uint16_t *row = a.frames + (size_t)f * a.w * a.h + (size_t)(y - 1) * a.w;
    uint32_t acc = 0;
    for (int x = 0; x < a.w; ++x) S[x + 1] = acc += row[x];
}
__global__ void __launch_bounds__(256) k_train_sat_cols(TrainWinArgs a) {
    const int f = blockIdx.y, x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > a.w) return;
    uint32_t *S = a.sat + (size_t)f * (a.h + 1) * (a.w + 1) + x;
    uint32_t acc = 0;
    for (int y = 1; y <= a.h; ++y) S[(size_t)y * (a.w + 1)] = acc += S[(size_t)y * (a.w + 1)];
}

__device__ __forceinline__ uint32_t sat_rect(const uint32_t *S, int stride, uint32_t x0, uint32_t y0, uint32_t rw, uint32_t rh) {
    return S[(size_t)(y0 + rh) * stride + x0 + rw] - S[(size_t)y0 * stride + x0 + rw] - S[(size_t)(y0 + rh) * stride + x0] +
           S[(size_t)y0 * stride + x0];
}

// Class of window `i` of a frame: 0 = background (whole-patch mean not > 0, prediction.rs:175-176), 1 = negative,
// 2 = positive (mask at the centre != 0, :177-179).
__device__ __forceinline__ int window_class(const TrainWinArgs &a, const uint32_t *S, const uint8_t *mask, uint32_t i) {
    const uint32_t x = a.lw + (i % a.nx) * a.step, y = a.lh + (i / a.nx) * a.step;
    if (sat_rect(S, a.w + 1, x - a.lw, y - a.lh, a.W, a.H) == 0) return 0;
    return mask[(size_t)y * a.w + x] ? 2 : 1;
}

// One workgroup per frame.  The reference shuffles each class and keeps the first 20 (:205-215); here the kept windows
// are the 20 of each class with the smallest key(seed, WINDOW, frame, window index), ties by window index (PARITY
// UNPINNED), found in 20 rounds of a (key, index) minimum above the previous round's.
#define TW_THREADS 256
__global__ void __launch_bounds__(TW_THREADS) k_train_select(TrainWinArgs a) {
    __shared__ uint64_t s_key[TW_THREADS];
    __shared__ uint32_t s_idx[TW_THREADS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const uint32_t *S = a.sat + (size_t)f * (a.h + 1) * (a.w + 1);
    const uint8_t *mask = a.masks + (size_t)f * a.w * a.h;
    const uint32_t nwin = a.nx * a.ny;
    const uint64_t frame = a.frame0 + f;
    uint32_t *sel = a.sel + (size_t)f * 2 * DH_TRAIN_KEEP;
    uint32_t kept = 0;
    for (int cls = 1; cls <= 2; ++cls) {
        uint64_t last_key = 0;
        uint32_t last_idx = 0;
        bool have_last = false;
        uint32_t n_cls = 0;
        for (int round = 0; round < DH_TRAIN_KEEP; ++round) {
            uint64_t bk = ~0ull;
            uint32_t bi = ~0u;
            for (uint32_t i = tid; i < nwin; i += TW_THREADS) {
                if (window_class(a, S, mask, i) != cls) continue;
                const uint64_t k = dh_train_key_(a.seed, DH_TAG_WINDOW, frame, i);
                if (have_last && (k < last_key || (k == last_key && i <= last_idx))) continue;
                if (k < bk || (k == bk && i < bi)) { bk = k; bi = i; }
            }
            s_key[tid] = bk;
            s_idx[tid] = bi;
            __syncthreads();
            for (int o = TW_THREADS / 2; o > 0; o >>= 1) {
                if (tid < o) {
                    const uint64_t k2 = s_key[tid + o];
                    const uint32_t i2 = s_idx[tid + o];
                    if (k2 < s_key[tid] || (k2 == s_key[tid] && i2 < s_idx[tid])) { s_key[tid] = k2; s_idx[tid] = i2; }
                }
                __syncthreads();
            }
            const uint64_t wk = s_key[0];
            const uint32_t wi = s_idx[0];
            __syncthreads();
            if (wi == ~0u) break;                                  // (uniform: every thread read the same minimum)
            if (tid == 0) sel[kept] = wi;
            ++kept; ++n_cls;
            last_key = wk; last_idx = wi; have_last = true;
        }
        if (tid == 0) a.cnt[(size_t)f * 2 + (cls - 1)] = n_cls;
    }
}

hipError_t dh_launch_train_windows(const TrainWinArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_train_sat_rows, dim3((a.h + 1 + 255) / 256, a.n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_train_sat_cols, dim3((a.w + 1 + 255) / 256, a.n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_train_select, dim3(a.n), dim3(TW_THREADS), 0, s, a);
    return hipGetLastError();
}

// ================================================================== sample materialisation
// One workgroup per kept window: its (W - rw + 1) x (H - rh + 1) image of rw x rh rectangle sums (every feature of a
// HoughLearning forest has that one rectangle size, so a split test is two gathers from it), and its truth (:177-196):
// offset = img_to_space_coord([x, y], depth(x, y)) - pos3d in f32 (types.rs:432-445; depth 0 included), rotation = the
// frame's f32 degrees widened to f64.
__global__ void __launch_bounds__(256) k_train_extract(TrainExtractArgs a) {
    const uint4 e = a.list[blockIdx.x];
    const uint32_t f = e.x, i = e.y, slot = e.z;
    const uint32_t *S = a.sat + (size_t)f * (a.h + 1) * (a.w + 1);
    const uint32_t x = a.lw + (i % a.nx) * a.step, y = a.lh + (i / a.nx) * a.step;
    const uint32_t x0 = x - a.lw, y0 = y - a.lh;
    uint32_t *box = a.box + (size_t)slot * a.bw * a.bh;
    for (uint32_t j = threadIdx.x; j < a.bw * a.bh; j += blockDim.x)
        box[j] = sat_rect(S, a.w + 1, x0 + j % a.bw, y0 + j / a.bw, a.rw, a.rh);
    if (threadIdx.x == 0) {
        const uint8_t m = a.masks[(size_t)f * a.w * a.h + (size_t)y * a.w + x];
        a.lab[slot] = m ? 1 : 0;
        float p3[3];
        to3d(a.kinv + (size_t)f * 9, (float)x, (float)y, (float)a.frames[(size_t)f * a.w * a.h + (size_t)y * a.w + x], p3);
        for (int k = 0; k < 3; ++k) {
            a.off[(size_t)slot * 3 + k] = m ? __fsub_rn(p3[k], a.pos3d[f * 3 + k]) : 0.0f;
            a.rot[(size_t)slot * 3 + k] = m ? (double)a.rot_deg[f * 3 + k] : 0.0;
        }
    }
}

hipError_t dh_launch_train_extract(const TrainExtractArgs &a, hipStream_t s) {
    if (a.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(k_train_extract, dim3(a.n_list), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ================================================================== split search
struct Cand {
    uint32_t o1, o2;     // offsets of the two rectangles' sums in a sample's image
    uint16_t x1, y1, x2, y2;
    double th;
};
// param_set (houghforest.rs:227-246) / RandomSubRectThresholdIterator::next (types.rs:148-159), keyed by (tree, heap, c).
__device__ __forceinline__ Cand make_cand(const TrainLevelArgs &a, uint32_t tree, uint32_t heap, uint32_t c) {
    Cand k;
    k.x1 = (uint16_t)dh_subrect_corner_(a.W, a.scale, dh_cand_u01_(a.seed, tree, heap, c, 0));
    k.y1 = (uint16_t)dh_subrect_corner_(a.H, a.scale, dh_cand_u01_(a.seed, tree, heap, c, 1));
    k.x2 = (uint16_t)dh_subrect_corner_(a.W, a.scale, dh_cand_u01_(a.seed, tree, heap, c, 2));
    k.y2 = (uint16_t)dh_subrect_corner_(a.H, a.scale, dh_cand_u01_(a.seed, tree, heap, c, 3));
    k.th = dh_cand_threshold_(dh_cand_u01_(a.seed, tree, heap, c, 4));
    k.o1 = (uint32_t)k.y1 * a.bw + k.x1;
    k.o2 = (uint32_t)k.y2 * a.bw + k.x2;
    return k;
}
// binarize (houghforest.rs:185-193) with average_value_in_rect (types.rs:317-339): (u64 sum as f64) / (count as f64),
// count 0 -> 0.0; Binar::One when avg1 - avg2 > threshold, in f64.
__device__ __forceinline__ int binarize(const TrainLevelArgs &a, const Cand &k, uint32_t s) {
    double m1 = 0.0, m2 = 0.0;
    if (a.area > 0.0) {
        const uint32_t *b = a.box + (size_t)s * a.stride;
        m1 = __ddiv_rn((double)b[k.o1], a.area);
        m2 = __ddiv_rn((double)b[k.o2], a.area);
    }
    return __dsub_rn(m1, m2) > k.th ? 1 : 0;
}

// ln! (houghforest.rs:18-20)
__device__ __forceinline__ double ln0(double x) { return x == 0.0 ? 0.0 : log(x); }
// Mat3::det (meancov_estimation.rs:339-343) of a symmetric matrix c = {00, 01, 02, 11, 12, 22}.
__device__ __forceinline__ double det_sym(const double *c) {
    const double m00 = c[0], m01 = c[1], m02 = c[2], m11 = c[3], m12 = c[4], m22 = c[5];
    const double t0 = __dsub_rn(__dmul_rn(m11, m22), __dmul_rn(m12, m12));
    const double t1 = __dsub_rn(__dmul_rn(m01, m22), __dmul_rn(m02, m12));
    const double t2 = __dsub_rn(__dmul_rn(m01, m12), __dmul_rn(m02, m11));
    return __dadd_rn(__dsub_rn(__dmul_rn(m00, t0), __dmul_rn(m01, t1)), __dmul_rn(m02, t2));
}

// One lane per (node, candidate); a workgroup's 256 lanes are 256 candidates of one node, so the sample stream (index,
// label, offset, rotation) is uniform across the wave and only the two rectangle gathers diverge.  Each lane walks its
// node's samples in order twice -- side counts and the f64 sums of the means, then the centred outer products -- which
// is estimate_mean_cov's two-pass order (meancov_estimation.rs:359-378) bit for bit: sums start from -0.0, the additive
// identity, exactly as the reference starts from set[0].  impurity (houghforest.rs:250-295) follows; a candidate that
// leaves one side empty is invalid (+inf), where the reference's impurity would be NaN.
// Side statistics of one candidate: counts, then the sums / centred outer-product sums of the positives' offsets and
// rotations.  The two sides are separate objects selected by a branch, so every accumulator index is a compile-time
// constant and the accumulators stay in registers.
struct SideAcc {
    uint32_t n = 0, p = 0;
    double so[3] = {-0.0, -0.0, -0.0}, sr[3] = {-0.0, -0.0, -0.0};   // -0.0: the additive identity (x + -0.0 == x for every x)
    double co[6] = {-0.0, -0.0, -0.0, -0.0, -0.0, -0.0}, cr[6] = {-0.0, -0.0, -0.0, -0.0, -0.0, -0.0};
    double mo[3], mr[3];
};
__device__ __forceinline__ void acc_sum(SideAcc &S, const float *o, const double *r) {
    S.p++;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        S.so[j] = __dadd_rn(S.so[j], (double)o[j]);
        S.sr[j] = __dadd_rn(S.sr[j], r[j]);
    }
}
__device__ __forceinline__ void acc_cov(SideAcc &S, const float *o, const double *r) {
    double d[3], e[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d[j] = __dsub_rn((double)o[j], S.mo[j]);
        e[j] = __dsub_rn(r[j], S.mr[j]);
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j, ++t) {
            S.co[t] = __dadd_rn(S.co[t], __dmul_rn(d[i], d[j]));
            S.cr[t] = __dadd_rn(S.cr[t], __dmul_rn(e[i], e[j]));
        }
}
// entropy(set) and regression_log(set) of one side (houghforest.rs:262-287); *neg counts det sums below -0.001.
__device__ __forceinline__ void side_terms(const SideAcc &S, double *ent, double *reg, uint32_t *neg) {
    const double prob = __ddiv_rn((double)S.p, (double)S.n);
    const double q = __dsub_rn(1.0, prob);
    *ent = __dadd_rn(__dmul_rn(prob, ln0(prob)), __dmul_rn(q, ln0(q)));
    *reg = 0.0;
    if (S.p) {
        const double dn = (double)(S.p - 1);                                          // n = 1: 0 / 0 = NaN
        double c1[6], c2[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) { c1[j] = __ddiv_rn(S.co[j], dn); c2[j] = __ddiv_rn(S.cr[j], dn); }
        const double x = __dadd_rn(det_sym(c1), det_sym(c2));
        if (x > 0.0) *reg = log(x);
        else if (x < -0.001) ++*neg;                                                 // unreachable!() there: scored 0, counted
    }
}

// One lane per (node, candidate); a workgroup's 256 lanes are 256 candidates of one node, so the sample stream (index,
// label, offset, rotation) is uniform across the wave and only the two rectangle gathers diverge.  Each lane walks its
// node's samples in order twice -- side counts and the f64 sums of the means, then the centred outer products -- which
// is estimate_mean_cov's two-pass order (meancov_estimation.rs:359-378) bit for bit: sums start from -0.0, the additive
// identity, exactly as the reference starts from set[0].  impurity (houghforest.rs:250-295) follows; a candidate that
// leaves one side empty is invalid (+inf), where the reference's impurity would be NaN.
__global__ void __launch_bounds__(256) k_train_score(TrainLevelArgs a) {
    const uint32_t node = blockIdx.x / a.cblocks;
    const uint32_t c = (blockIdx.x % a.cblocks) * blockDim.x + threadIdx.x;
    if (c >= a.F) return;
    const TrainNode nd = a.nodes[node];
    const Cand k = make_cand(a, nd.tree, nd.heap, c);
    SideAcc zero, one;
    for (uint32_t q = nd.begin; q < nd.end; ++q) {
        const uint32_t smp = a.idx[q];
        const int sd = binarize(a, k, smp);
        if (sd) one.n++; else zero.n++;
        if (a.lab[smp]) {
            const float *o = a.off + (size_t)smp * 3;
            const double *r = a.rot + (size_t)smp * 3;
            if (sd) acc_sum(one, o, r); else acc_sum(zero, o, r);
        }
    }
    double *out = a.score + (size_t)node * a.F + c;
    if (zero.n == 0 || one.n == 0) { *out = INFINITY; return; }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        zero.mo[j] = __ddiv_rn(zero.so[j], (double)zero.p); zero.mr[j] = __ddiv_rn(zero.sr[j], (double)zero.p);
        one.mo[j] = __ddiv_rn(one.so[j], (double)one.p); one.mr[j] = __ddiv_rn(one.sr[j], (double)one.p);
    }
    for (uint32_t q = nd.begin; q < nd.end; ++q) {
        const uint32_t smp = a.idx[q];
        if (!a.lab[smp]) continue;
        const float *o = a.off + (size_t)smp * 3;
        const double *r = a.rot + (size_t)smp * 3;
        if (binarize(a, k, smp)) acc_cov(one, o, r); else acc_cov(zero, o, r);
    }
    const double count = (double)(zero.n + one.n);
    const double f0 = __ddiv_rn((double)zero.n, count), f1 = __ddiv_rn((double)one.n, count);   // rel!(set.len(), count)
    double e0, e1, r0, r1;
    uint32_t neg = 0;
    side_terms(zero, &e0, &r0, &neg);
    side_terms(one, &e1, &r1, &neg);
    const double ent = __dadd_rn(__dmul_rn(f0, e0), __dmul_rn(f1, e1));
    const double reg = __dadd_rn(__dmul_rn(f0, r0), __dmul_rn(f1, r1));
    *out = __dadd_rn(-ent, __dmul_rn(a.wdepth, reg));
    if (neg) atomicAdd(a.neg_det, (unsigned long long)neg);
}

// Per node: the minimum score over the valid candidates, the lowest candidate index on equal scores (PARITY UNPINNED:
// stamm's choice), then every sample's side under it.
__global__ void __launch_bounds__(256) k_train_best(TrainLevelArgs a) {
    __shared__ double s_sc[256];
    __shared__ uint32_t s_c[256];
    const uint32_t node = blockIdx.x, tid = threadIdx.x;
    const double *sc = a.score + (size_t)node * a.F;
    double bs = INFINITY;
    uint32_t bc = ~0u;
    for (uint32_t c = tid; c < a.F; c += blockDim.x) {
        const double v = sc[c];
        if (v < bs) { bs = v; bc = c; }                                 // (ascending c per thread: first of equals kept)
    }
    s_sc[tid] = bs;
    s_c[tid] = bc;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const double v = s_sc[tid + o];
            const uint32_t c2 = s_c[tid + o];
            if (v < s_sc[tid] || (v == s_sc[tid] && c2 < s_c[tid])) { s_sc[tid] = v; s_c[tid] = c2; }
        }
        __syncthreads();
    }
    const uint32_t win = s_c[0];
    const TrainNode nd = a.nodes[node];
    if (win == ~0u) {
        if (tid == 0) a.best[node].cand = -1;
        return;
    }
    const Cand k = make_cand(a, nd.tree, nd.heap, win);
    if (tid == 0) {
        TrainBest b{};
        b.cand = (int32_t)win;
        b.r1[0] = k.x1; b.r1[1] = k.y1; b.r1[2] = (uint16_t)(k.x1 + a.rw); b.r1[3] = (uint16_t)(k.y1 + a.rh);   // Rect::new (types.rs:40-45)
        b.r2[0] = k.x2; b.r2[1] = k.y2; b.r2[2] = (uint16_t)(k.x2 + a.rw); b.r2[3] = (uint16_t)(k.y2 + a.rh);
        b.threshold = k.th;
        b.score = s_sc[0];
        a.best[node] = b;
    }
    for (uint32_t q = nd.begin + tid; q < nd.end; q += blockDim.x) a.side[q] = (uint8_t)binarize(a, k, a.idx[q]);
}

hipError_t dh_launch_train_level(const TrainLevelArgs &a, hipStream_t s) {
    if (a.n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_train_score, dim3(a.n_nodes * a.cblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_train_best, dim3(a.n_nodes), dim3(256), 0, s, a);
    return hipGetLastError();
}
