// k_render.hip -- posed triangle meshes to depth frames and head masks (the rule is stated in
// include/depthhead_hip.h, section "rendering posed meshes").  Four kernels:
//   k_render_setup    one lane per (instance, triangle): transform, projection, snapping, rejection; the triangle record; one
//                     count per screen tile its bounding box touches;
//   k_render_offsets  one lane per (frame, tile): the tile's run of list slots (a wave scan and one atomic per wave: the runs
//                     are disjoint, their order is free, as the minimum that reads them is);
//   k_render_fill     one lane per triangle again: its record index into the list of every tile it touches;
//   k_render_resolve  one workgroup per (frame, tile): the tile's triangles rasterised into 64 x 16 keys in LDS with LDS atomic
//                     minima -- small triangles one per lane, larger ones by the 64 lanes of a wave together -- then the
//                     sensor model and 16-byte depth / 8-byte mask stores.  An empty tile stores zeros and does nothing else.
// Integer coverage (int64 edge functions), f64 depth in a fixed order, an order-free minimum: bit-identical run to run.
#include "dh_device.h"
#include "dh_render.h"

#define RS_THREADS 256

// ------------------------------------------------------------------ the pieces of the rule
// Pixel columns (rows alike) whose centre 16 x + 8 lies in [lo, hi] of snapped coordinates: ceil((lo - 8) / 16) .. floor((hi - 8) / 16)
__device__ __forceinline__ int px_first(int lo) { return (lo + 7) >> 4; }
__device__ __forceinline__ int px_last(int hi) { return (hi - 8) >> 4; }

__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(a, max(b, c)); }

// The pixel rectangle of a record inside the frame: false when it holds no pixel centre.
__device__ __forceinline__ bool tri_pixels(const RenderTri &t, int w, int h, int &xa, int &xb, int &ya, int &yb) {
    xa = max(px_first(min3(t.x0, t.x1, t.x2)), 0);
    xb = min(px_last(max3(t.x0, t.x1, t.x2)), w - 1);
    ya = max(px_first(min3(t.y0, t.y1, t.y2)), 0);
    yb = min(px_last(max3(t.y0, t.y1, t.y2)), h - 1);
    return xa <= xb && ya <= yb;
}

// edge function of a -> b at P: (bx - ax) (Py - ay) - (by - ay) (Px - ax); every factor fits 22 bits, the value 43
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}
// an edge a -> b of a triangle of positive area owns the pixel centres on it when it is a left edge (dy < 0: the inside lies
// toward +x) or a top edge (dy == 0, dx > 0: the inside lies toward +y)
__device__ __forceinline__ bool edge_owns(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return dy < 0 || (dy == 0 && dx > 0);
}

// What a lane needs to rasterise one triangle.
struct TriEval {
    int x0, y0, x1, y1, x2, y2;
    double iz0, iz1, iz2;
    long long b0, b1, b2;      // 0 where the edge owns its pixels, else -1: inside <=> e_i + b_i >= 0
    uint32_t low;
};
__device__ __forceinline__ TriEval tri_eval(const RenderTri &t) {
    TriEval e;
    e.x0 = t.x0; e.y0 = t.y0; e.x1 = t.x1; e.y1 = t.y1; e.x2 = t.x2; e.y2 = t.y2;
    e.iz0 = 1.0 / (double)t.z0; e.iz1 = 1.0 / (double)t.z1; e.iz2 = 1.0 / (double)t.z2;
    e.b0 = edge_owns(t.x1, t.y1, t.x2, t.y2) ? 0 : -1;      // edge i lies opposite vertex i
    e.b1 = edge_owns(t.x2, t.y2, t.x0, t.y0) ? 0 : -1;
    e.b2 = edge_owns(t.x0, t.y0, t.x1, t.y1) ? 0 : -1;
    e.low = t.low;
    return e;
}
// The key of pixel (x, y) under a triangle, or 0xFFFFFFFF when its centre is not covered.
__device__ __forceinline__ uint32_t tri_key(const TriEval &t, int x, int y) {
    const int px = 16 * x + 8, py = 16 * y + 8;
    const long long e0 = edge_fn(t.x1, t.y1, t.x2, t.y2, px, py);
    const long long e1 = edge_fn(t.x2, t.y2, t.x0, t.y0, px, py);
    const long long e2 = edge_fn(t.x0, t.y0, t.x1, t.y1, px, py);
    if (((e0 + t.b0) | (e1 + t.b1) | (e2 + t.b2)) < 0) return 0xFFFFFFFFu;
    const double num = (double)(e0 + e1 + e2);
    const double den = __dadd_rn(__dadd_rn(__dmul_rn((double)e0, t.iz0), __dmul_rn((double)e1, t.iz1)), __dmul_rn((double)e2, t.iz2));
    const double zz = __dadd_rn(__ddiv_rn(num, den), 0.5);
    uint32_t d;
    if (!(zz >= 1.0)) d = 1u;                  // (NaN included)
    else if (zz >= 65535.0) d = 65535u;
    else d = (uint32_t)zz;
    return (d << 1) | t.low;
}

// ------------------------------------------------------------------ setup
__global__ __launch_bounds__(RS_THREADS) void k_render_setup(const RenderArgs a) {
    const uint32_t inst_i = blockIdx.x;
    const dh_render_instance *in = a.inst + inst_i;
    const RenderMesh m = a.meshes[in->mesh];
    const uint32_t tri_i = blockIdx.y * RS_THREADS + threadIdx.x;
    unsigned long long refs = 0;
    if (tri_i < m.nt) {
        const uint32_t frame = in->frame;
        float K[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) K[q] = a.cams ? a.cams[frame].k[q] : a.k[q];
        const float sc = in->scale;
        RenderTri t;
        t.frame = frame;
        t.low = (in->flags & DH_RENDER_HEAD) ? 0u : 1u;
        bool ok = true;
        int sx[3], sy[3];
        float pz[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t vi = m.tris[(size_t)tri_i * 3 + c];
            const float sv0 = __fmul_rn(m.verts[(size_t)vi * 3 + 0], sc), sv1 = __fmul_rn(m.verts[(size_t)vi * 3 + 1], sc),
                        sv2 = __fmul_rn(m.verts[(size_t)vi * 3 + 2], sc);
            float p[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                p[j] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(in->R[3 * j], sv0), __fmul_rn(in->R[3 * j + 1], sv1)),
                                           __fmul_rn(in->R[3 * j + 2], sv2)), in->t[j]);
            float r[3];
            matvec3(K, p[0], p[1], p[2], r);
            const float fx = floorf(__fadd_rn(__fmul_rn(__fdiv_rn(r[0], r[2]), 16.0f), 0.5f));
            const float fy = floorf(__fadd_rn(__fmul_rn(__fdiv_rn(r[1], r[2]), 16.0f), 0.5f));
            // (a NaN or infinity fails the comparisons)
            ok = ok && !(p[2] < 1.0f) && fabsf(fx) <= (float)DH_RENDER_GUARD && fabsf(fy) <= (float)DH_RENDER_GUARD;
            sx[c] = ok ? (int)fx : 0; sy[c] = ok ? (int)fy : 0;
            pz[c] = p[2];
        }
        const long long area = edge_fn(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
        ok = ok && area != 0;
        const bool swap = area < 0;            // both windings are drawn: vertices 1 and 2 change places
        t.x0 = sx[0]; t.y0 = sy[0]; t.z0 = pz[0];
        t.x1 = swap ? sx[2] : sx[1]; t.y1 = swap ? sy[2] : sy[1]; t.z1 = swap ? pz[2] : pz[1];
        t.x2 = swap ? sx[1] : sx[2]; t.y2 = swap ? sy[1] : sy[2]; t.z2 = swap ? pz[1] : pz[2];
        int xa, xb, ya, yb;
        ok = ok && tri_pixels(t, a.w, a.h, xa, xb, ya, yb);
        t.valid = ok ? 1u : 0u;
        a.tri[(size_t)a.tri_begin[inst_i] + tri_i] = t;
        if (ok) {
            uint32_t *cnt = a.tile_cnt + (size_t)frame * a.tiles_x * a.tiles_y;
            for (int ty = ya / DH_RT_H; ty <= yb / DH_RT_H; ++ty)
                for (int tx = xa / DH_RT_W; tx <= xb / DH_RT_W; ++tx) atomicAdd(cnt + ty * a.tiles_x + tx, 1u);
            refs = (unsigned long long)(yb / DH_RT_H - ya / DH_RT_H + 1) * (unsigned long long)(xb / DH_RT_W - xa / DH_RT_W + 1);
        }
    }
    refs = wave_sum_u64(refs);
    if (lane_id() == 0 && refs) atomicAdd(a.total, refs);
}

// ------------------------------------------------------------------ offsets
__global__ __launch_bounds__(RS_THREADS) void k_render_offsets(const RenderArgs a, uint32_t n_tiles) {
    const uint32_t i = blockIdx.x * RS_THREADS + threadIdx.x;
    const uint32_t c = i < n_tiles ? a.tile_cnt[i] : 0u;
    const uint32_t incl = wave_incl_scan(c);
    const uint32_t sum = (uint32_t)__shfl((int)incl, WAVE - 1);
    unsigned long long base = 0;
    if (lane_id() == 0 && sum) base = atomicAdd(a.total + 1, (unsigned long long)sum);
    base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
    if (i < n_tiles) a.tile_cur[i] = (uint32_t)(base + incl - c);      // (the host has checked: the whole list is below 2^32 slots)
}

// ------------------------------------------------------------------ fill
__global__ __launch_bounds__(RS_THREADS) void k_render_fill(const RenderArgs a, uint32_t n_tri) {
    const uint32_t i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n_tri) return;
    const RenderTri t = a.tri[i];
    if (!t.valid) return;
    int xa, xb, ya, yb;
    if (!tri_pixels(t, a.w, a.h, xa, xb, ya, yb)) return;
    uint32_t *cur = a.tile_cur + (size_t)t.frame * a.tiles_x * a.tiles_y;
    for (int ty = ya / DH_RT_H; ty <= yb / DH_RT_H; ++ty)
        for (int tx = xa / DH_RT_W; tx <= xb / DH_RT_W; ++tx) {
            const unsigned long long slot = atomicAdd(cur + ty * a.tiles_x + tx, 1u);
            if (slot < a.list_cap) a.list[slot] = i;       // (always: the host sized the list from the counts of this very call)
        }
}

// ------------------------------------------------------------------ resolve
// splitmix64 output number c of the stream seeded with `seed` (synth.SplitMix: state seed + (c + 1) * golden, then the finaliser)
__device__ __forceinline__ unsigned long long splitmix_at(unsigned long long seed, unsigned long long c) {
    unsigned long long z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// depth of a key after the sensor model; k = the pixel's index in the batch
template <bool SENSOR>
__device__ __forceinline__ uint32_t key_depth(const RenderArgs &a, uint32_t key, unsigned long long k) {
    if (key == 0xFFFFFFFFu) return 0u;
    uint32_t d = key >> 1;
    if (SENSOR) {
        const long long noisy = (long long)d + (long long)(splitmix_at(a.seed, 2ull * k) % (2ull * a.noise + 1ull)) - (long long)a.noise;
        d = (uint32_t)min(max(noisy, 1ll), 65535ll);
        if ((splitmix_at(a.seed, 2ull * k + 1ull) >> 11) < a.hole_thr) d = 0u;
    }
    return d;
}

#define SMALL_PIXELS 8      // a triangle with at most this many candidate pixels in the tile is rasterised by the lane that loaded it

template <bool SENSOR>
__global__ __launch_bounds__(RS_THREADS) void k_render_resolve(const RenderArgs a) {
    __shared__ uint32_t keys[DH_RT_W * DH_RT_H];
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, frame = blockIdx.y;
    const size_t tile = ((size_t)frame * a.tiles_y + ty) * a.tiles_x + tx;
    const uint32_t cnt = a.tile_cnt[tile];
    const int ox = tx * DH_RT_W, oy = ty * DH_RT_H;
    if (cnt) {
        for (int i = threadIdx.x; i < DH_RT_W * DH_RT_H; i += RS_THREADS) keys[i] = 0xFFFFFFFFu;
        __syncthreads();
        const uint32_t end = a.tile_cur[tile], begin = end - cnt;
        const int lane = lane_id(), wave = threadIdx.x / WAVE;
        const int tx1 = min(ox + DH_RT_W, a.w) - 1, ty1 = min(oy + DH_RT_H, a.h) - 1;
        for (uint32_t base = begin + wave * WAVE; base < end; base += RS_THREADS) {
            const bool have = base + lane < end;
            RenderTri t;
            t.x0 = t.y0 = t.x1 = t.y1 = t.x2 = t.y2 = 0; t.z0 = t.z1 = t.z2 = 1.0f; t.frame = 0; t.low = 1; t.valid = 0;
            if (have) t = a.tri[a.list[base + lane]];
            int xa, xb, ya, yb;
            bool any = have && tri_pixels(t, a.w, a.h, xa, xb, ya, yb);
            if (any) { xa = max(xa, ox); xb = min(xb, tx1); ya = max(ya, oy); yb = min(yb, ty1); any = xa <= xb && ya <= yb; }
            const int bw = any ? xb - xa + 1 : 0, bh = any ? yb - ya + 1 : 0;
            const bool small = any && bw * bh <= SMALL_PIXELS;
            if (small) {
                const TriEval e = tri_eval(t);
                for (int y = ya; y <= yb; ++y)
                    for (int x = xa; x <= xb; ++x) {
                        const uint32_t key = tri_key(e, x, y);
                        if (key != 0xFFFFFFFFu) atomicMin(&keys[(y - oy) * DH_RT_W + (x - ox)], key);
                    }
            }
            // the larger ones, one after the other, by the whole wave: lane p takes candidate pixels p, p + 64, ...
            unsigned long long big = __ballot(any && !small);
            while (big) {
                const int src = __ffsll((long long)big) - 1;
                big &= big - 1;
                RenderTri u;
                u.x0 = __shfl(t.x0, src); u.y0 = __shfl(t.y0, src); u.x1 = __shfl(t.x1, src); u.y1 = __shfl(t.y1, src);
                u.x2 = __shfl(t.x2, src); u.y2 = __shfl(t.y2, src);
                u.z0 = __shfl(t.z0, src); u.z1 = __shfl(t.z1, src); u.z2 = __shfl(t.z2, src);
                u.low = (uint32_t)__shfl((int)t.low, src);
                const int uxa = __shfl(xa, src), uya = __shfl(ya, src), ubw = __shfl(bw, src), ubh = __shfl(bh, src);
                const TriEval e = tri_eval(u);
                const float rbw = 1.0f / (float)ubw;
                for (int p = lane; p < ubw * ubh; p += WAVE) {
                    const int row = div_small(p, ubw, rbw), col = p - row * ubw;
                    const uint32_t key = tri_key(e, uxa + col, uya + row);
                    if (key != 0xFFFFFFFFu) atomicMin(&keys[(uya + row - oy) * DH_RT_W + (uxa + col - ox)], key);
                }
            }
        }
        __syncthreads();
    }
    // store: 8 pixels per lane, the first 128 lanes cover the tile's 16 rows of 64
    if (threadIdx.x < DH_RT_W * DH_RT_H / 8) {
        const int row = threadIdx.x / (DH_RT_W / 8), x = ox + (threadIdx.x % (DH_RT_W / 8)) * 8, y = oy + row;
        if (y < a.h && x < a.w) {
            const size_t k0 = ((size_t)frame * a.h + y) * a.w + x;
            uint32_t d[8], m[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t key = cnt ? keys[row * DH_RT_W + (x - ox) + q] : 0xFFFFFFFFu;
                d[q] = key_depth<SENSOR>(a, key, k0 + q);
                m[q] = (key & 1u) ? 0u : 1u;            // (the empty key is odd)
            }
            if (a.vec) {
                uint4 dv;
                dv.x = d[0] | (d[1] << 16); dv.y = d[2] | (d[3] << 16); dv.z = d[4] | (d[5] << 16); dv.w = d[6] | (d[7] << 16);
                *(uint4 *)(a.frames + k0) = dv;
                if (a.masks) {
                    uint2 mv;
                    mv.x = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24); mv.y = m[4] | (m[5] << 8) | (m[6] << 16) | (m[7] << 24);
                    *(uint2 *)(a.masks + k0) = mv;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (x + q < a.w) {
                        a.frames[k0 + q] = (uint16_t)d[q];
                        if (a.masks) a.masks[k0 + q] = (uint8_t)m[q];
                    }
            }
        }
    }
}

// ------------------------------------------------------------------ launchers
hipError_t dh_launch_render_setup(const RenderArgs &a, hipStream_t s) {
    if (a.n_inst == 0 || a.max_nt == 0) return hipSuccess;
    const uint32_t chunks = (a.max_nt + RS_THREADS - 1) / RS_THREADS;
    if (chunks > 65535) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_render_setup, dim3(a.n_inst, chunks), dim3(RS_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t dh_launch_render_offsets(const RenderArgs &a, hipStream_t s) {
    const uint32_t n_tiles = (uint32_t)a.n * a.tiles_x * a.tiles_y;
    hipLaunchKernelGGL(k_render_offsets, dim3((n_tiles + RS_THREADS - 1) / RS_THREADS), dim3(RS_THREADS), 0, s, a, n_tiles);
    return hipGetLastError();
}
hipError_t dh_launch_render_fill(const RenderArgs &a, hipStream_t s) {
    if (a.n_tri == 0) return hipSuccess;
    hipLaunchKernelGGL(k_render_fill, dim3((a.n_tri + RS_THREADS - 1) / RS_THREADS), dim3(RS_THREADS), 0, s, a, a.n_tri);
    return hipGetLastError();
}
hipError_t dh_launch_render_resolve(const RenderArgs &a, hipStream_t s) {
    if (a.n > 65535) return hipErrorInvalidConfiguration;
    const dim3 grid((uint32_t)(a.tiles_x * a.tiles_y), (uint32_t)a.n);
    if (a.noise != 0 || a.hole_thr != 0) hipLaunchKernelGGL(k_render_resolve<true>, grid, dim3(RS_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_render_resolve<false>, grid, dim3(RS_THREADS), 0, s, a);
    return hipGetLastError();
}
