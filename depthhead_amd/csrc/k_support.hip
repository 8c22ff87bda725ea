// k_support.hip -- vote support of each frame's pose: head bounding box, supporting windows / hits, mass (k_support)
//
// One of the kernel translation units of libdepthhead_hip.so (hand-written HIP for gfx950: wave64, 160 KB LDS/CU;
// no MFMA anywhere -- there is no dense contraction on this path).  Overview of the pipeline: dh_api.hip; the
// definition of the record: include/depthhead_hip.h (dh_support) and DESIGN.md section 13.
#include <algorithm>

#include "dh_device.h"

// ================================================================== k_support
// Runs after k_cluster on the same stream.  Workgroup (x, frame) takes the frame's hit records x, x + gridDim.x, ... in
// runs of SUP_THREADS (one lane per record).  For a hit record with position votes (LF_OFF) the lane first tests its
// HitBox -- the cell box every vote of the leaf lands in -- against the cube m +- r around the frame's final midpoint cell m:
//   * box misses the cube: no vote can support.  Its votes still count into total_mass: when lo[2] >= 1 every vote's z is
//     at least 1 (z cell = trunc(p3.z - o.z) and lo[2] = trunc(p3.z - max o.z)), so the hit adds v * n_offsets without a
//     read; otherwise the offsets are walked under the reference's z < 0 rule (non-finite offsets included);
//   * box meets the cube: the offsets are walked, every vote with !(z < 0) adds v to total_mass and, when its cell lies in
//     the cube, to mass, and marks the hit as supporting.
// A supporting hit sets its window's bit in the frame's window bitmap (SupAcc::bits): the lanes that find the bit clear
// count a new window.  Sums and counts are reduced over the wave and added with one atomic per wave; the box of the
// supporting windows' centres is a wave min / max, then one atomicMin / atomicMax per wave.  Everything is integer, so the
// record does not depend on the order of the atomics.
//
// The last workgroup of a frame (ticket on SupAcc::done) writes the frame's dh_support and returns the frame's
// accumulator and bitmap to zero, so the scratch needs no fill between calls.
#define SUP_THREADS 256

__device__ __forceinline__ bool in_cube(int32_t c, int64_t lo, int64_t hi) { return (int64_t)c >= lo && (int64_t)c <= hi; }

// (wave_sum_u64, wave_min_u32, wave_max_u32, load_agent: dh_device.h)

__global__ void __launch_bounds__(SUP_THREADS) k_support(SupportArgs a) {
    const int frame = blockIdx.y, lane = threadIdx.x & (WAVE - 1);
    SupAcc *acc = a.acc + frame;
    uint32_t *bits = a.bits + (size_t)frame * a.bit_words;
    uint32_t n = a.hit_count[frame];
    if (n > a.hits_cap) n = a.hits_cap;
    // the frame's midpoint cell (k_cluster: integer-valued, DH_ZSCALEFACTOR = 1) and the cube around it, in 64 bits
    const float *mp = a.poses[frame].mid_point;
    const int64_t r = (int64_t)a.radius;
    int64_t clo[3], chi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t m = (int64_t)f32_as_i32(mp[k]);
        clo[k] = m - r; chi[k] = m + r;
    }
    const HitRec *hits = a.hits + (size_t)frame * a.hits_cap;
    const HitBox *hbox = a.hit_box + (size_t)frame * a.hits_cap;
    const uint32_t *hwin = a.hit_win + (size_t)frame * a.hits_cap;
    uint64_t mass = 0, total = 0;           // this lane's share, over all its records
    uint32_t n_hits = 0, n_win = 0;
    uint32_t xmin = 0xFFFFFFFFu, ymin = 0xFFFFFFFFu, xmax = 0, ymax = 0;
    const uint32_t stride = gridDim.x * SUP_THREADS;
    for (uint32_t base = blockIdx.x * SUP_THREADS; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool sup = false;
        if (i < n) {
            const int4 b0 = ((const int4 *)(hbox + i))[0], b1 = ((const int4 *)(hbox + i))[1];
            const uint32_t v = (uint32_t)b1.z, fc = (uint32_t)b1.w, n_off = fc >> 8;
            if (fc & LF_OFF) {
                const bool meets = (int64_t)b0.x <= chi[0] && (int64_t)b0.w >= clo[0] && (int64_t)b0.y <= chi[1] && (int64_t)b1.x >= clo[1] &&
                                   (int64_t)b0.z <= chi[2] && (int64_t)b1.y >= clo[2];
                if (!meets && b0.z >= 1) {
                    total += (uint64_t)v * n_off;                    // every vote has z >= 1: none is dropped, none supports
                } else {
                    const float4 rec = *(const float4 *)(hits + i);
                    const uint32_t ob = __float_as_uint(rec.w);
                    uint32_t cnt = 0, in = 0;
#pragma unroll 1
                    for (uint32_t o = ob; o < ob + n_off; ++o) {
                        const float4 of = a.off4[o];
                        const float nx = __fsub_rn(rec.x, of.x), ny = __fsub_rn(rec.y, of.y), nz = __fsub_rn(rec.z, of.z);  // prediction.rs:647
                        if (nz < 0.0f) continue;                                                                             // :650
                        ++cnt;
                        if (meets && in_cube(f32_as_i32(nx), clo[0], chi[0]) && in_cube(f32_as_i32(ny), clo[1], chi[1]) &&
                            in_cube(f32_as_i32(__fdiv_rn(nz, (float)DH_ZSCALEFACTOR)), clo[2], chi[2]))
                            ++in;
                    }
                    total += (uint64_t)v * cnt;
                    mass += (uint64_t)v * in;
                    sup = in > 0;
                }
            }
        }
        if (sup) {
            ++n_hits;
            const uint32_t gp = hwin[i];
            const uint32_t gy = gp / (uint32_t)a.nx, gx = gp - gy * (uint32_t)a.nx;
            const uint32_t cx = gx * (uint32_t)a.step + (uint32_t)a.lw, cy = gy * (uint32_t)a.step + (uint32_t)a.lh;
            xmin = min(xmin, cx); xmax = max(xmax, cx); ymin = min(ymin, cy); ymax = max(ymax, cy);
            const uint32_t bit = 1u << (gp & 31u);
            if (!(atomicOr(&bits[gp >> 5], bit) & bit)) ++n_win;     // first supporting hit of this window
        }
    }
    // one atomic per wave and quantity (the accumulator's neutral value is 0: minima are kept as their complement)
    mass = wave_sum_u64(mass); total = wave_sum_u64(total);
    n_hits = (uint32_t)wave_sum_u64(n_hits); n_win = (uint32_t)wave_sum_u64(n_win);
    xmin = wave_min_u32(xmin); ymin = wave_min_u32(ymin); xmax = wave_max_u32(xmax); ymax = wave_max_u32(ymax);
    if (lane == 0) {
        if (total) atomicAdd((unsigned long long *)&acc->total, (unsigned long long)total);
        if (n_hits) {
            atomicAdd((unsigned long long *)&acc->mass, (unsigned long long)mass);
            atomicAdd(&acc->hits, n_hits);
            if (n_win) atomicAdd(&acc->windows, n_win);
            atomicMax(&acc->nxmin, ~xmin); atomicMax(&acc->nymin, ~ymin);
            atomicMax(&acc->xmax, xmax); atomicMax(&acc->ymax, ymax);
        }
    }
    // the frame's last workgroup writes the record and clears the scratch for the next call
    __shared__ uint32_t s_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(&acc->done, 1u) == gridDim.x - 1 ? 1u : 0u;
        if (s_last) __threadfence();
    }
    __syncthreads();
    if (!s_last) return;
    for (uint32_t wd = threadIdx.x; wd < a.bit_words; wd += SUP_THREADS) bits[wd] = 0u;
    if (threadIdx.x == 0) {
        dh_support s{};
        const uint32_t hc = load_agent(&acc->hits);
        if (hc) {
            const uint32_t x0 = ~load_agent(&acc->nxmin), y0 = ~load_agent(&acc->nymin);
            s.x = x0; s.y = y0;
            s.width = load_agent(&acc->xmax) - x0 + 1u;
            s.height = load_agent(&acc->ymax) - y0 + 1u;
            s.windows = load_agent(&acc->windows);
            s.hits = hc;
            s.mass = load_agent(&acc->mass);
        }
        s.total_mass = load_agent(&acc->total);
        a.out[frame] = s;
        *acc = SupAcc{};
    }
}

hipError_t dh_launch_support(const SupportArgs &a, hipStream_t s) {
    if (a.n_frames == 0) return hipSuccess;
    if (a.n_frames > 65535) return hipErrorInvalidConfiguration;
    // workgroups per frame: about 2048 in the grid (8 per CU), none beyond one per SUP_THREADS records a frame can hold
    const uint32_t per = (a.hits_cap + SUP_THREADS - 1) / SUP_THREADS;
    const uint32_t want = (2048u + (uint32_t)a.n_frames - 1) / (uint32_t)a.n_frames;
    const dim3 grid(std::max(1u, std::min(per, want)), a.n_frames), block(SUP_THREADS);
    hipLaunchKernelGGL(k_support, grid, block, 0, s, a);
    return hipGetLastError();
}
