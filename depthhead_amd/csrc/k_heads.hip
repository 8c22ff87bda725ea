// k_heads.hip -- several heads per frame: seed cells, their vote moments, the heads' support and rotation grids, merge and order
// (k_heads_seeds, k_heads_moments, k_heads_support, k_heads_finish)
//
// One of the kernel translation units of libdepthhead_hip.so (hand-written HIP for gfx950: wave64, 160 KB LDS/CU;
// no MFMA anywhere -- there is no dense contraction on this path).  The definition: include/depthhead_hip.h (dh_head) and
// DESIGN.md section 14.  A heads batch runs k_boxsum / k_traverse / k_emit (SUP instance) / k_vote as any batch, then
//   k_heads_seeds -> k_heads_moments -> k_cluster<HEADS> (positions) -> k_heads_support -> k_cluster<HEADS> (rotations) -> k_heads_finish.
// Every scratch array that is summed into (moments, support accumulators and bitmaps, rotation grids) is zero on entry and is
// returned to zero by the kernel that reads it, so nothing is filled between calls.
#include <algorithm>

#include "dh_device.h"

#define HD_THREADS 256
#define SEED_THREADS 512

// ================================================================== k_heads_seeds
// One workgroup per frame.  Round j picks the first cell in (count descending, index ascending) order that has a count above 0
// and lies more than DH_HEADS_SUPPRESS cells (Chebyshev) from the cells picked in rounds 0 .. j-1: that is the walk of the
// definition, since every cell it passes over before that one is empty or suppressed.  Key = count << 32 | ~index, maximum
// over the workgroup.
__global__ void __launch_bounds__(SEED_THREADS) k_heads_seeds(HeadsArgs a) {
    __shared__ unsigned long long red[SEED_THREADS / WAVE];
    __shared__ int32_t s_pick[DH_MAX_HEADS];
    const int frame = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const uint32_t c = tid < DH_POSGRID ? a.pos_grid[(size_t)frame * DH_POSGRID + tid] : 0u;
    const int gx = tid % DH_GRID, gy = tid / DH_GRID;
    int np = 0;
    for (int j = 0; j < a.max_heads; ++j) {
        bool ok = c > 0u;
        for (int q = 0; q < j; ++q) {
            const int pk = s_pick[q];
            if (abs(gx - pk % DH_GRID) <= DH_HEADS_SUPPRESS && abs(gy - pk / DH_GRID) <= DH_HEADS_SUPPRESS) ok = false;
        }
        unsigned long long key = ok ? ((unsigned long long)c << 32) | (uint32_t)~(uint32_t)tid : 0ull;
        for (int d = WAVE / 2; d; d >>= 1) { const unsigned long long o = __shfl_xor(key, d); key = o > key ? o : key; }
        if (lane == 0) red[wave] = key;
        __syncthreads();
        unsigned long long best = 0;
        for (int w2 = 0; w2 < SEED_THREADS / WAVE; ++w2) best = red[w2] > best ? red[w2] : best;
        if (!best) break;                                   // (uniform)
        if (tid == 0) s_pick[j] = (int32_t)~(uint32_t)best;
        np = j + 1;
        __syncthreads();                                    // s_pick[j] visible, red free for the next round
    }
    if (tid < DH_MAX_HEADS) a.pick[(size_t)frame * DH_MAX_HEADS + tid] = tid < np ? s_pick[tid] : -1;
    if (tid == 0) a.nseed[frame] = (uint32_t)np;
}

hipError_t dh_launch_heads_seeds(const HeadsArgs &a, hipStream_t s) {
    if (a.n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_heads_seeds, dim3(a.n_frames), dim3(SEED_THREADS), 0, s, a);
    return hipGetLastError();
}

// ================================================================== k_heads_moments
// Workgroup (x, frame) takes the frame's hit records x * HD_THREADS + lane, + gridDim.x * HD_THREADS, ... (one lane per record)
// and walks its position votes.  A vote's guess-grid cell is the reference's (prediction.rs:660-676): the projection with its two
// IEEE divisions, the clamps, the truncation and x * 20 / w -- the cell k_vote's approximate quotient also arrives at (it
// falls back to this expression wherever it could differ).  A vote in seed cell k adds (v, v c_x, v c_y, v c_z) to head k's
// moments in 128 bits: per lane in registers while consecutive votes stay in one seed cell, then into the workgroup's LDS
// copy, then into the frame's HdMom, each step an exact 128-bit add (a 64-bit atomic whose returned old value gives the carry).
__device__ __forceinline__ void mom_add(unsigned long long *lo, unsigned long long *hi, uint64_t vlo, uint64_t vhi) {
    if (!vlo && !vhi) return;
    const uint64_t old = atomicAdd(lo, (unsigned long long)vlo);
    const uint64_t carry = old + vlo < old ? 1ull : 0ull;
    if (vhi + carry) atomicAdd(hi, (unsigned long long)(vhi + carry));
}

template <bool CAM>
__global__ void __launch_bounds__(HD_THREADS) k_heads_moments(HeadsArgs a) {
    __shared__ unsigned long long s_lo[DH_MAX_HEADS * 4], s_hi[DH_MAX_HEADS * 4];
    const int frame = blockIdx.y, tid = threadIdx.x;
    const uint32_t ns = a.nseed[frame];
    if (ns == 0) return;                                                // (uniform)
    if (CAM) {
#pragma unroll
        for (int i = 0; i < 9; ++i) a.k[i] = a.cams[frame].k[i];
    }
    int32_t pk[DH_MAX_HEADS];
#pragma unroll
    for (int k = 0; k < DH_MAX_HEADS; ++k) pk[k] = a.pick[(size_t)frame * DH_MAX_HEADS + k];
    if (tid < DH_MAX_HEADS * 4) { s_lo[tid] = 0ull; s_hi[tid] = 0ull; }
    __syncthreads();
    uint32_t n = a.hit_count[frame];
    if (n > a.hits_cap) n = a.hits_cap;
    const HitRec *hits = a.hits + (size_t)frame * a.hits_cap;
    const HitBox *hbox = a.hit_box + (size_t)frame * a.hits_cap;
    const float wm1 = (float)(a.w - 1), hm1 = (float)(a.h - 1);
    for (uint32_t i = blockIdx.x * HD_THREADS + tid; i < n; i += gridDim.x * HD_THREADS) {
        const int4 b1 = ((const int4 *)(hbox + i))[1];
        const uint32_t v = (uint32_t)b1.z, fc = (uint32_t)b1.w;
        if (!(fc & LF_OFF)) continue;
        const float4 rec = *(const float4 *)(hits + i);
        const uint32_t ob = __float_as_uint(rec.w), oe = ob + (fc >> 8);
        int cur = -1;
        uint64_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
        auto flush = [&]() {
            if (cur < 0) return;
#pragma unroll
            for (int q = 0; q < 4; ++q) { mom_add(&s_lo[cur * 4 + q], &s_hi[cur * 4 + q], lo[q], hi[q]); lo[q] = 0; hi[q] = 0; }
        };
#pragma unroll 1
        for (uint32_t o = ob; o < oe; ++o) {
            const float4 of = a.off4[o];
            const float nx = __fsub_rn(rec.x, of.x), ny = __fsub_rn(rec.y, of.y), nz = __fsub_rn(rec.z, of.z);   // prediction.rs:647
            if (nz < 0.0f) continue;                                                                             // :650
            float r[3];
            matvec3(a.k, nx, ny, nz, r);                                                                         // types.rs:425
            const float qx = __fdiv_rn(r[0], r[2]), qy = __fdiv_rn(r[1], r[2]);
            float x2 = qx > 0.0f ? qx : 0.0f; x2 = x2 < wm1 ? x2 : wm1;                                          // :662
            float y2 = qy > 0.0f ? qy : 0.0f; y2 = y2 < hm1 ? y2 : hm1;                                          // :663
            const int32_t idx = (int32_t)(((uint32_t)y2 * DH_GRID / (uint32_t)a.h) * DH_GRID + (uint32_t)x2 * DH_GRID / (uint32_t)a.w);   // :671-675
            int kk = -1;
#pragma unroll
            for (int k = DH_MAX_HEADS - 1; k >= 0; --k) kk = idx == pk[k] ? k : kk;
            if (kk < 0) continue;
            if (kk != cur) { flush(); cur = kk; }
            const int64_t cx = f32_as_i32(nx), cy = f32_as_i32(ny), cz = f32_as_i32(__fdiv_rn(nz, (float)DH_ZSCALEFACTOR));   // :667
            add_i128(lo[0], hi[0], (int64_t)v);
            add_i128(lo[1], hi[1], (int64_t)v * cx);
            add_i128(lo[2], hi[2], (int64_t)v * cy);
            add_i128(lo[3], hi[3], (int64_t)v * cz);
        }
        flush();
    }
    __syncthreads();
    if (tid < (int)ns * 4) {
        HdMom *m = a.mom + (size_t)frame * DH_MAX_HEADS + tid / 4;
        mom_add(&m->lo[tid & 3], &m->hi[tid & 3], s_lo[tid], s_hi[tid]);
    }
}

// workgroups per frame of the record passes: about 2048 in the grid (8 per CU), none beyond one per HD_THREADS records
static dim3 hd_grid(const HeadsArgs &a) {
    const uint32_t per = (a.hits_cap + HD_THREADS - 1) / HD_THREADS;
    const uint32_t want = (2048u + (uint32_t)a.n_frames - 1) / (uint32_t)a.n_frames;
    return dim3(std::max(1u, std::min(per, want)), a.n_frames);
}

hipError_t dh_launch_heads_moments(const HeadsArgs &a, hipStream_t s) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.n_frames > 65535) return hipErrorInvalidConfiguration;
    if (a.cams) hipLaunchKernelGGL(k_heads_moments<true>, hd_grid(a), dim3(HD_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_heads_moments<false>, hd_grid(a), dim3(HD_THREADS), 0, s, a);
    return hipGetLastError();
}

// ================================================================== k_heads_support
// k_support for the cubes mid_k +- r of the frame's nseed heads at once: a hit's offsets are walked once
// and every vote is tested against every cube.  Per head the same record as k_support's, from per-head accumulators, window
// bitmaps and the last-workgroup write-and-zero; total_mass is the frame's and is kept once (head 0's accumulator, which also
// holds the workgroup ticket).  Besides the records:
//   * hmask[i]: bit k set when hit i supports head k (written for every record of the frame: no fill);
//   * the rotation votes of a supporting hit (prediction.rs:601-636: its distinct 20^3 guess-grid cells x valtoadd) go into the
//     20^3 grid of every head it supports -- the coarse grid of that head's restricted rotation accumulator.
__global__ void __launch_bounds__(HD_THREADS) k_heads_support(HeadsArgs a) {
    const int frame = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    const uint32_t nh = a.nseed[frame];
    if (nh == 0) return;                                                // (uniform)
    SupAcc *acc = a.acc + (size_t)frame * DH_MAX_HEADS;
    uint32_t n = a.hit_count[frame];
    if (n > a.hits_cap) n = a.hits_cap;
    const int64_t r = (int64_t)a.radius;
    int32_t m[DH_MAX_HEADS][3];
#pragma unroll
    for (int k = 0; k < DH_MAX_HEADS; ++k)
#pragma unroll
        for (int q = 0; q < 3; ++q) m[k][q] = (uint32_t)k < nh ? f32_as_i32(a.hpose[(size_t)frame * DH_MAX_HEADS + k].mid_point[q]) : 0;
    const HitRec *hits = a.hits + (size_t)frame * a.hits_cap;
    const HitBox *hbox = a.hit_box + (size_t)frame * a.hits_cap;
    const HitRot *hrot = a.hit_rot + (size_t)frame * a.hits_cap;
    const uint32_t *hwin = a.hit_win + (size_t)frame * a.hits_cap;
    uint8_t *hmask = a.hmask + (size_t)frame * a.hits_cap;
    uint64_t mass[DH_MAX_HEADS] = {}, total = 0;
    uint32_t n_hits[DH_MAX_HEADS] = {}, n_win[DH_MAX_HEADS] = {};
    uint32_t xmin[DH_MAX_HEADS], ymin[DH_MAX_HEADS], xmax[DH_MAX_HEADS] = {}, ymax[DH_MAX_HEADS] = {};
#pragma unroll
    for (int k = 0; k < DH_MAX_HEADS; ++k) { xmin[k] = 0xFFFFFFFFu; ymin[k] = 0xFFFFFFFFu; }
    const uint32_t stride = gridDim.x * HD_THREADS;
    for (uint32_t base = blockIdx.x * HD_THREADS; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const int4 b0 = ((const int4 *)(hbox + i))[0], b1 = ((const int4 *)(hbox + i))[1];
        const uint32_t v = (uint32_t)b1.z, fc = (uint32_t)b1.w, n_off = fc >> 8;
        uint32_t smask = 0;
        if (fc & LF_OFF) {
            bool meets[DH_MAX_HEADS], any = false;
#pragma unroll
            for (int k = 0; k < DH_MAX_HEADS; ++k) {
                meets[k] = (uint32_t)k < nh && (int64_t)b0.x <= m[k][0] + r && (int64_t)b0.w >= m[k][0] - r && (int64_t)b0.y <= m[k][1] + r &&
                           (int64_t)b1.x >= m[k][1] - r && (int64_t)b0.z <= m[k][2] + r && (int64_t)b1.y >= m[k][2] - r;
                any = any || meets[k];
            }
            if (!any && b0.z >= 1) {
                total += (uint64_t)v * n_off;                    // every vote has z >= 1: none is dropped, none supports
            } else {
                const float4 rec = *(const float4 *)(hits + i);
                const uint32_t ob = __float_as_uint(rec.w);
                uint32_t cnt = 0, in[DH_MAX_HEADS] = {};
#pragma unroll 1
                for (uint32_t o = ob; o < ob + n_off; ++o) {
                    const float4 of = a.off4[o];
                    const float nx = __fsub_rn(rec.x, of.x), ny = __fsub_rn(rec.y, of.y), nz = __fsub_rn(rec.z, of.z);  // prediction.rs:647
                    if (nz < 0.0f) continue;                                                                             // :650
                    ++cnt;
                    if (!any) continue;
                    const int64_t cx = f32_as_i32(nx), cy = f32_as_i32(ny), cz = f32_as_i32(__fdiv_rn(nz, (float)DH_ZSCALEFACTOR));
#pragma unroll
                    for (int k = 0; k < DH_MAX_HEADS; ++k)
                        if (meets[k] && cx >= m[k][0] - r && cx <= m[k][0] + r && cy >= m[k][1] - r && cy <= m[k][1] + r &&
                            cz >= m[k][2] - r && cz <= m[k][2] + r)
                            ++in[k];
                }
                total += (uint64_t)v * cnt;
#pragma unroll
                for (int k = 0; k < DH_MAX_HEADS; ++k) {
                    mass[k] += (uint64_t)v * in[k];
                    smask |= in[k] ? 1u << k : 0u;
                }
            }
        }
        hmask[i] = (uint8_t)smask;
        if (!smask) continue;
        const uint32_t gp = hwin[i];
        const uint32_t gy = gp / (uint32_t)a.nx, gx = gp - gy * (uint32_t)a.nx;
        const uint32_t cx = gx * (uint32_t)a.step + (uint32_t)a.lw, cy = gy * (uint32_t)a.step + (uint32_t)a.lh;
        const uint4 rr = (fc & LF_ROT) ? *(const uint4 *)(hrot + i) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int k = 0; k < DH_MAX_HEADS; ++k) {
            if (!(smask & (1u << k))) continue;
            ++n_hits[k];
            xmin[k] = min(xmin[k], cx); xmax[k] = max(xmax[k], cx); ymin[k] = min(ymin[k], cy); ymax[k] = max(ymax[k], cy);
            uint32_t *bits = a.bits + ((size_t)frame * DH_MAX_HEADS + k) * a.bit_words;
            const uint32_t bit = 1u << (gp & 31u);
            if (!(atomicOr(&bits[gp >> 5], bit) & bit)) ++n_win[k];     // first supporting hit of this window for head k
            uint32_t *g = a.rgrid + ((size_t)frame * DH_MAX_HEADS + k) * DH_GRID3;
            for (uint32_t q = rr.z; q < rr.z + (rr.w >> 16); ++q) {      // :636 (no rotation votes: rr = 0, an empty range)
                const uint32_t c = a.rough_cell[q];
                atomicAdd(&g[c & 0xffffu], v * (c >> 16));
            }
        }
    }
    // one atomic per wave and quantity
    total = wave_sum_u64(total);
    if (lane == 0 && total) atomicAdd((unsigned long long *)&acc[0].total, (unsigned long long)total);
#pragma unroll
    for (int k = 0; k < DH_MAX_HEADS; ++k) {
        if ((uint32_t)k >= nh) break;                                   // (uniform)
        const uint64_t ms = wave_sum_u64(mass[k]);
        const uint32_t hc = (uint32_t)wave_sum_u64(n_hits[k]), wc = (uint32_t)wave_sum_u64(n_win[k]);
        const uint32_t x0 = wave_min_u32(xmin[k]), y0 = wave_min_u32(ymin[k]), x1 = wave_max_u32(xmax[k]), y1 = wave_max_u32(ymax[k]);
        if (lane == 0 && hc) {
            atomicAdd((unsigned long long *)&acc[k].mass, (unsigned long long)ms);
            atomicAdd(&acc[k].hits, hc);
            if (wc) atomicAdd(&acc[k].windows, wc);
            atomicMax(&acc[k].nxmin, ~x0); atomicMax(&acc[k].nymin, ~y0);
            atomicMax(&acc[k].xmax, x1); atomicMax(&acc[k].ymax, y1);
        }
    }
    // the frame's last workgroup writes the records and clears the scratch for the next call
    __shared__ uint32_t s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(&acc[0].done, 1u) == gridDim.x - 1 ? 1u : 0u;
        if (s_last) __threadfence();
    }
    __syncthreads();
    if (!s_last) return;
    uint32_t *bits = a.bits + (size_t)frame * DH_MAX_HEADS * a.bit_words;
    for (uint32_t wd = threadIdx.x; wd < nh * a.bit_words; wd += HD_THREADS) bits[wd] = 0u;
    dh_support sr{};
    if (threadIdx.x < nh) {
        const int k = threadIdx.x;
        const uint32_t hc = load_agent(&acc[k].hits);
        if (hc) {
            const uint32_t x0 = ~load_agent(&acc[k].nxmin), y0 = ~load_agent(&acc[k].nymin);
            sr.x = x0; sr.y = y0;
            sr.width = load_agent(&acc[k].xmax) - x0 + 1u;
            sr.height = load_agent(&acc[k].ymax) - y0 + 1u;
            sr.windows = load_agent(&acc[k].windows);
            sr.hits = hc;
            sr.mass = load_agent(&acc[k].mass);
        }
        sr.total_mass = load_agent(&acc[0].total);
    }
    __syncthreads();                                                    // (every record has read head 0's total)
    if (threadIdx.x < nh) {
        a.hsup[(size_t)frame * DH_MAX_HEADS + threadIdx.x] = sr;
        acc[threadIdx.x] = SupAcc{};
    }
}

hipError_t dh_launch_heads_support(const HeadsArgs &a, hipStream_t s) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.n_frames > 65535) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_heads_support, hd_grid(a), dim3(HD_THREADS), 0, s, a);
    return hipGetLastError();
}

// ================================================================== k_heads_finish
// One thread per frame: drop heads without mass, merge (a head within DH_MEANSHIFT_KERNEL_SIZE cells, Chebyshev, of a head kept
// before it in seed order is dropped), order by mass descending with ties in seed order, zero-fill the remaining slots.
__global__ void __launch_bounds__(WAVE) k_heads_finish(HeadsArgs a) {
    const int frame = blockIdx.x * WAVE + threadIdx.x;
    if (frame >= a.n_frames) return;
    const uint32_t ns = a.nseed[frame];
    int keep[DH_MAX_HEADS];
    int nk = 0;
    for (uint32_t k = 0; k < ns; ++k) {
        const size_t e = (size_t)frame * DH_MAX_HEADS + k;
        if (a.hsup[e].mass == 0) continue;
        const float *mk = a.hpose[e].mid_point;
        bool merged = false;
        for (int j = 0; j < nk; ++j) {
            const float *mj = a.hpose[(size_t)frame * DH_MAX_HEADS + keep[j]].mid_point;
            int64_t d = 0;
            for (int q = 0; q < 3; ++q) {
                const int64_t dq = (int64_t)f32_as_i32(mk[q]) - (int64_t)f32_as_i32(mj[q]);
                d = std::max(d, dq < 0 ? -dq : dq);
            }
            merged = merged || d <= DH_MEANSHIFT_KERNEL_SIZE;
        }
        if (!merged) keep[nk++] = (int)k;
    }
    for (int j = 1; j < nk; ++j) {                                      // stable insertion sort, mass descending
        const int x = keep[j];
        const uint64_t mx = a.hsup[(size_t)frame * DH_MAX_HEADS + x].mass;
        int q = j - 1;
        while (q >= 0 && a.hsup[(size_t)frame * DH_MAX_HEADS + keep[q]].mass < mx) { keep[q + 1] = keep[q]; --q; }
        keep[q + 1] = x;
    }
    dh_head *out = a.heads + (size_t)frame * a.max_heads;
    for (int j = 0; j < a.max_heads; ++j) {
        dh_head hd{};
        if (j < nk) {
            const size_t e = (size_t)frame * DH_MAX_HEADS + keep[j];
            hd.pose = a.hpose[e];
            hd.pose.reserved = 0;
            hd.support = a.hsup[e];
        }
        out[j] = hd;
    }
    a.n_heads[frame] = (uint32_t)nk;
}

hipError_t dh_launch_heads_finish(const HeadsArgs &a, hipStream_t s) {
    if (a.n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_heads_finish, dim3((a.n_frames + WAVE - 1) / WAVE), dim3(WAVE), 0, s, a);
    return hipGetLastError();
}
