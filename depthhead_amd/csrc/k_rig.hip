// k_rig.hip -- the heads of a rig's cameras fused into persons with rig-wide identities (k_rig_fuse)
//
// One of the kernel translation units of libdepthhead_hip.so (hand-written HIP for gfx950).  Overview of the pipeline: dh_api.hip.
#include "dh_device.h"
#include "dh_rig.h"

// ================================================================== k_rig_fuse
// After a rig tracker step's k_heads_finish, on the same stream: ONE WORKGROUP PER RIG runs the rule of dh_rig.h (dh_rig_step is
// its sequential statement; this is a parallel implementation of it and must produce its bytes).  A rig has up to 64 x 4 = 256
// heads, one per lane: lane = (camera - rig_begin) * DH_MAX_HEADS + j, so ascending lanes are ascending (camera, j).
//   load    every lane loads its head's midpoint and mass and its camera's R, t with all loads in flight, and writes world
//           midpoint, cell and mass to LDS; the rig's 16 track records come into LDS as 288 dwords, coalesced.
//   order   a head's rank is the number of heads that precede it (dh_rig_before_): one broadcast read per lane and head of the
//           rig, no sort network; the head's cell and mass are stored again at its rank.
//   fuse    wave 0 walks the ranked heads; lane p < 16 IS person p and keeps its anchor cell, views, sums and mass in registers.
//           Every person tests the head at once; __ballot and its first set bit pick "the first person in creation order"; a
//           head nobody takes founds person n_persons.  Only the joined lane's registers change: no atomics.
//   match   wave 0 again: lane = (person, 4 slots); <= 16 rounds, each a wave-wide minimum (six __shfl_xor steps) of the packed
//           key (d, person, slot) over the pairs still free; the taken masks are wave-uniform registers.  Then lane t coasts or
//           frees track t, and the births walk the free-slot mask.  Matched and born tracks are written by their person's lane.
//   store   ids per lane, persons and tracks as dwords from LDS, plain coalesced stores.
// The phases are separated by workgroup barriers that all four waves reach; waves 1 .. 3 idle through fuse and match (the
// sequential part: at most 256 + 16 dependent steps of a few instructions each).
// A rig with no present camera keeps its state: ids 0, n_persons 0, persons zero, the snapshot its unchanged records.
#define RIG_THREADS 256
#define RIG_TRACK_WORDS (DH_RIG_MAX_TRACKS * sizeof(dh_rig_track) / 4)      // 288
#define RIG_PERSON_WORDS (DH_RIG_MAX_PERSONS * sizeof(dh_rig_person) / 4)   // 224
static_assert(RIG_THREADS == DH_RIG_MAX_RIG_HEADS, "one lane per head of the largest rig");
static_assert(DH_MAX_HEADS == 4, "lane = camera * 4 + head");

__device__ __forceinline__ uint64_t rig_wave_min(uint64_t v) {
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ void __launch_bounds__(RIG_THREADS) k_rig_fuse(RigFuseArgs a) {
    __shared__ int32_t s_cell[RIG_THREADS][3];        // (stride 3 dwords: the lanes of a wave fall on different banks)
    __shared__ float s_world[RIG_THREADS][3];
    __shared__ uint64_t s_mass[RIG_THREADS];
    __shared__ int32_t s_rcell[RIG_THREADS][3];       // the heads in the order of step 1: cell, mass and lane of rank r, so that
    __shared__ uint64_t s_rmass[RIG_THREADS];         // the fuse walk's loads do not depend on one another
    __shared__ uint16_t s_order[RIG_THREADS];
    __shared__ uint8_t s_valid[RIG_THREADS];
    __shared__ int8_t s_pof[RIG_THREADS];             // the person of a head, -1: none
    __shared__ dh_rig_track s_tr[DH_RIG_MAX_TRACKS];
    __shared__ dh_rig_person s_ps[DH_RIG_MAX_PERSONS];
    __shared__ int32_t s_pslot[DH_RIG_MAX_PERSONS];   // the slot a person matched (0 .. 15) or was born into (256 + slot), -1: none
    __shared__ uint32_t s_np;

    const int g = blockIdx.x, l = threadIdx.x, k = l >> 2, j = l & 3;
    const int c0 = a.rig_begin[g], nc = a.rig_begin[g + 1] - c0;      // 1 .. 64 (dh_rig_create)
    const int c = c0 + k;
    const bool cam = k < nc, pres = cam && (!a.present || a.present[c] != 0);
    uint32_t nh = pres ? a.n_heads[c] : 0u;
    nh = nh > (uint32_t)a.max_heads ? (uint32_t)a.max_heads : nh;
    const bool valid = (uint32_t)j < nh;

    // ---- load
    uint32_t *trw = reinterpret_cast<uint32_t *>(s_tr);
    const uint32_t *gtr = reinterpret_cast<const uint32_t *>(a.state + (size_t)g * DH_RIG_MAX_TRACKS);
    for (int i = l; i < (int)RIG_TRACK_WORDS; i += RIG_THREADS) trw[i] = gtr[i];
    uint64_t mass = 0;
    if (valid) {
        const dh_head *h = a.heads + (size_t)c * a.max_heads + j;
        const RigCam rc = a.cams[c];
        const float m[3] = {h->pose.mid_point[0], h->pose.mid_point[1], h->pose.mid_point[2]};
        mass = h->support.mass;
        for (int q = 0; q < 3; ++q) {
            const float w = dh_rig_world_(rc.R, rc.t, m, q);
            s_world[l][q] = w;
            s_cell[l][q] = (int32_t)dh_th_cell_(w);
        }
    }
    s_mass[l] = mass;
    s_valid[l] = valid ? 1 : 0;
    s_pof[l] = -1;
    if (l < DH_RIG_MAX_PERSONS) s_pslot[l] = -1;
    const int any = __syncthreads_or(pres ? 1 : 0);
    const int n = __syncthreads_count(valid ? 1 : 0);

    // ---- order
    if (valid) {
        int rank = 0;
#pragma unroll 8
        for (int m = 0; m < nc * DH_MAX_HEADS; ++m) rank += s_valid[m] && dh_rig_before_(s_mass[m], (uint32_t)m, mass, (uint32_t)l) ? 1 : 0;
        s_order[rank] = (uint16_t)l;
        s_rmass[rank] = mass;
        for (int q = 0; q < 3; ++q) s_rcell[rank][q] = s_cell[l][q];
    }
    __syncthreads();

    // ---- fuse (wave 0; lane p is person p)
    if (l < 64) {
        int np = 0, anchor = 0;
        int32_t ac[3] = {0, 0, 0};
        int64_t sum[3] = {0, 0, 0};
        uint64_t views = 0, msum = 0;
        uint32_t nv = 0;
        for (int r = 0; r < n; ++r) {
            const int h = s_order[r], hk = h >> 2;
            const int32_t hc[3] = {s_rcell[r][0], s_rcell[r][1], s_rcell[r][2]};
            const bool ok = l < np && dh_rig_cheb_(ac, hc) <= (int64_t)a.fuse_gate && !(views >> hk & 1u);
            const uint64_t b = __ballot(ok);
            int p;
            if (b) p = __ffsll((unsigned long long)b) - 1;
            else if (np < DH_RIG_MAX_PERSONS) {
                p = np++;
                if (l == p) { anchor = h; ac[0] = hc[0]; ac[1] = hc[1]; ac[2] = hc[2]; }
            } else continue;                                   // unassigned: s_pof stays -1
            if (l == p) {
                views |= (uint64_t)1 << hk;
                nv += 1u;
                msum = dh_rig_sat_add_(msum, s_rmass[r]);
                for (int q = 0; q < 3; ++q) sum[q] += hc[q];
                s_pof[h] = (int8_t)p;
            }
        }
        if (l < DH_RIG_MAX_PERSONS) {
            dh_rig_person rec;
            memset(&rec, 0, sizeof rec);
            if (l < np) {
                rec.views = views; rec.mass = msum; rec.n_views = nv;
                for (int q = 0; q < 3; ++q) { rec.cell[q] = (int32_t)dh_rig_floor_div_(sum[q], (int64_t)nv); rec.world[q] = s_world[anchor][q]; }
                rec.best_cam = (uint32_t)(c0 + (anchor >> 2)); rec.best_head = (uint32_t)(anchor & 3);
            }
            s_ps[l] = rec;
        }
        if (l == 0) s_np = (uint32_t)np;
    }
    __syncthreads();

    // ---- match (wave 0; lane = person * 4 + a group of four slots).  A rig without a present camera skips it: state kept.
    if (any && l < 64) {
        const int np = (int)s_np, p = l >> 2, sg = (l & 3) * 4;
        uint32_t live = 0;
        for (int s = 0; s < DH_RIG_MAX_TRACKS; ++s) live |= s_tr[s].id != 0 ? 1u << s : 0u;
        uint64_t key[4];
        for (int i = 0; i < 4; ++i) {
            const int s = sg + i;
            const int64_t d = dh_rig_cheb_(s_tr[s].person.cell, s_ps[p].cell);
            key[i] = p < np && (live >> s & 1u) && d <= (int64_t)a.gate ? dh_rig_key_(d, p, s) : UINT64_MAX;
        }
        uint32_t t_used = 0, p_used = 0;
        for (int round = 0; round < np; ++round) {
            uint64_t best = UINT64_MAX;
            if (!(p_used >> p & 1u))
                for (int i = 0; i < 4; ++i) best = !(t_used >> (sg + i) & 1u) && key[i] < best ? key[i] : best;
            best = rig_wave_min(best);
            if (best == UINT64_MAX) break;
            const int bp = (int)(best >> 4 & 15u), bs = (int)(best & 15u);
            p_used |= 1u << bp;
            t_used |= 1u << bs;
            if (l == 0) { s_pslot[bp] = bs; s_ps[bp].id = s_tr[bs].id; }
        }
        // unmatched live tracks coast, and are freed after max_misses consecutive misses (lane t: track t)
        bool freed = false;
        if (l < DH_RIG_MAX_TRACKS && (live >> l & 1u) && !(t_used >> l & 1u)) {
            const uint32_t age = dh_th_inc_(s_tr[l].age), misses = dh_th_inc_(s_tr[l].misses);
            freed = misses > a.max_misses;
            if (freed) memset(&s_tr[l], 0, sizeof(dh_rig_track));
            else { s_tr[l].age = age; s_tr[l].misses = misses; }
        }
        uint32_t free_mask = (~live & 0xffffu) | (uint32_t)__ballot(freed);
        // unmatched persons are born in the lowest free slots
        uint32_t next = a.next_id[g];
        for (int q = 0; q < np; ++q) {
            if (p_used >> q & 1u) continue;
            if (!free_mask) break;
            const int slot = __ffs((int)free_mask) - 1;
            free_mask &= free_mask - 1u;
            if (l == 0) { s_pslot[q] = 256 + slot; s_ps[q].id = next; }
            next = next == UINT32_MAX ? 1u : next + 1u;
        }
        if (l == 0) a.next_id[g] = next;
    }
    __syncthreads();
    if (any && l < (int)s_np && s_pslot[l] >= 0) {
        const int slot = s_pslot[l] & 255;
        const bool born = s_pslot[l] >= 256;
        dh_rig_track &m = s_tr[slot];
        const dh_rig_person rec = s_ps[l];
        m.id = rec.id;
        m.age = born ? 1u : dh_th_inc_(m.age);
        m.hits = born ? 1u : dh_th_inc_(m.hits);
        m.misses = 0u;
        m.person = rec;
    }
    __syncthreads();

    // ---- store
    if (cam && j < a.max_heads) a.ids[(size_t)c * a.max_heads + j] = s_pof[l] >= 0 ? s_ps[s_pof[l]].id : 0u;
    if (l == 0) a.n_persons[g] = any ? s_np : 0u;
    const uint32_t *psw = reinterpret_cast<const uint32_t *>(s_ps);
    uint32_t *gps = reinterpret_cast<uint32_t *>(a.persons + (size_t)g * DH_RIG_MAX_PERSONS);
    if (l < (int)RIG_PERSON_WORDS) gps[l] = psw[l];
    uint32_t *gst = reinterpret_cast<uint32_t *>(a.state + (size_t)g * DH_RIG_MAX_TRACKS);
    uint32_t *gsn = a.snapshot ? reinterpret_cast<uint32_t *>(a.snapshot + (size_t)g * DH_RIG_MAX_TRACKS) : nullptr;
    for (int i = l; i < (int)RIG_TRACK_WORDS; i += RIG_THREADS) {
        const uint32_t v = trw[i];
        if (any) gst[i] = v;
        if (gsn) gsn[i] = v;
    }
}

hipError_t dh_launch_rig_fuse(const RigFuseArgs &a, hipStream_t s) {
    if (a.n_rigs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rig_fuse, dim3(a.n_rigs), dim3(RIG_THREADS), 0, s, a);
    return hipGetLastError();
}
