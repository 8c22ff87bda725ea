// k_track_heads.hip -- identities of several heads per camera across steps (k_track_heads)
//
// One of the kernel translation units of libdepthhead_hip.so (hand-written HIP for gfx950).  Overview of the pipeline: dh_api.hip.
#include "dh_device.h"
#include "dh_track_heads.h"

// ================================================================== k_track_heads
// After a multi-head tracker step's k_heads_finish, on the same stream: one lane per camera matches the step's heads against the
// camera's tracks (dh_track_heads.h: at most 8 x 4 distances and 4 rounds of picking the least), rewrites its track records and
// writes the heads' ids with plain per-lane stores.  Absent cameras (present[c] == 0) keep their tracks and get ids of zeros.
// With a snapshot output the camera's records after the step are copied there too.
// The rule reads back what it writes (a matched slot's counters after its head, the free slots after the frees), so a lane first
// copies its 8 records and its heads into its own rows of LDS -- all loads in flight at once -- runs the rule there, and writes
// the records back: a few global round trips per lane instead of one per dependent access.  Rows are padded by 8 bytes, so that
// the lanes of a wave fall on different banks.  No lane reads another's rows: no barrier.
#define TRACK_HEADS_THREADS 64
struct LaneTracks { dh_head_track t[DH_MAX_TRACKS]; uint32_t pad[2]; };   // 776 B
struct LaneHeads { dh_head h[DH_MAX_HEADS]; uint32_t pad[2]; };           // 328 B
__global__ void __launch_bounds__(TRACK_HEADS_THREADS) k_track_heads(TrackHeadsArgs a) {
    __shared__ LaneTracks s_tr[TRACK_HEADS_THREADS];
    __shared__ LaneHeads s_hd[TRACK_HEADS_THREADS];
    const int c = blockIdx.x * TRACK_HEADS_THREADS + threadIdx.x;
    if (c >= a.n) return;
    dh_head_track *tr = a.state + (size_t)c * DH_MAX_TRACKS;
    uint32_t *ids = a.ids + (size_t)c * a.max_heads;
    dh_head_track *ltr = s_tr[threadIdx.x].t;
    if (a.present && !a.present[c]) {
        for (int j = 0; j < a.max_heads; ++j) ids[j] = 0;
        if (!a.snapshot) return;
        for (int t = 0; t < DH_MAX_TRACKS; ++t) ltr[t] = tr[t];
    } else {
        const dh_head *hd = a.heads + (size_t)c * a.max_heads;
        dh_head *lhd = s_hd[threadIdx.x].h;
        for (int t = 0; t < DH_MAX_TRACKS; ++t) ltr[t] = tr[t];
        for (int j = 0; j < a.max_heads; ++j) lhd[j] = hd[j];
        uint32_t next_id = a.next_id[c];
        dh_track_heads_step(ltr, &next_id, lhd, a.n_heads[c], a.max_heads, a.gate, a.max_misses, ids);
        for (int t = 0; t < DH_MAX_TRACKS; ++t) tr[t] = ltr[t];
        a.next_id[c] = next_id;
    }
    if (a.snapshot) {
        dh_head_track *snap = a.snapshot + (size_t)c * DH_MAX_TRACKS;
        for (int t = 0; t < DH_MAX_TRACKS; ++t) snap[t] = ltr[t];
    }
}

hipError_t dh_launch_track_heads(const TrackHeadsArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_track_heads, dim3((a.n + TRACK_HEADS_THREADS - 1) / TRACK_HEADS_THREADS), dim3(TRACK_HEADS_THREADS), 0, s, a);
    return hipGetLastError();
}

static_assert(sizeof(LaneTracks) == 776 && sizeof(LaneHeads) == 328, "LDS rows: 194 and 82 dwords, 2 and 18 banks apart");
