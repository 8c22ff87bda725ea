// k_track.hip -- live tracking state update (k_track)
//
// One of the kernel translation units of libdepthhead_hip.so (hand-written HIP for gfx950).  Overview of the pipeline: dh_api.hip.
#include "dh_device.h"
#include "dh_track.h"

// ================================================================== k_track
// After a tracker step's k_cluster, on the same stream: one lane per camera applies the live loop's rule (dh_track.h) to the
// step's pose and rewrites the camera's guesses -- the arrays the next step's k_region / k_cluster read as midp_guess,
// rot_guess and guess_mask.  Cameras absent from the step (present[c] == 0) keep their state.
#define TRACK_THREADS 256
__global__ void __launch_bounds__(TRACK_THREADS) k_track(TrackArgs a) {
    const int c = blockIdx.x * TRACK_THREADS + threadIdx.x;
    if (c >= a.n) return;
    if (a.present && !a.present[c]) return;
    const dh_pose &p = a.poses[c];
    dh_track_update(a.flags, p.mid_point, p.rotation, a.midp + (size_t)c * 3, a.rot + (size_t)c * 3, a.mask + c, a.has_rot + c);
}

hipError_t dh_launch_track(const TrackArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_track, dim3((a.n + TRACK_THREADS - 1) / TRACK_THREADS), dim3(TRACK_THREADS), 0, s, a);
    return hipGetLastError();
}

static_assert(DH_TRACK_FLAG_PREV_GUESS == DH_TRACK_PREV_GUESS && DH_TRACK_FLAG_SLUGGISH == DH_TRACK_SLUGGISH, "dh_track.h flags = the ABI flags");
