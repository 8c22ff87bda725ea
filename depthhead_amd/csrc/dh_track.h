// dh_track.h -- the state update of a live head tracker (dh_tracker_step): the rule of the reference's live loop,
// examples/live_prediction.rs:79-101, written once for k_track (k_track.hip) and for the host checks (tests/host/track_check.cpp).
// Plain C++ outside hipcc: DH_HD drops the __host__ __device__ qualifiers, so g++ compiles this header as it stands.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define DH_HD __host__ __device__
#else
#define DH_HD
#endif

#define DH_TRACK_FLAG_PREV_GUESS 1u   // = DH_TRACK_PREV_GUESS of depthhead_hip.h
#define DH_TRACK_FLAG_SLUGGISH 2u     // = DH_TRACK_SLUGGISH

// f32 subtraction and addition with one IEEE rounding each, in the order written (the reference's `-`, `+` on f32)
DH_HD inline float dh_track_sub_(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
DH_HD inline float dh_track_add_(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

// The stored midpoint takes the new one (live_prediction.rs:92-99) unless --sluggish holds it: the sluggish test lets it move when
// |m0 - s0| + |m1 - s1| + |m2 - s2| < 100 (f32, summed left to right) or when the stored z is below 500.
DH_HD inline bool dh_track_takes_midp(uint32_t flags, const float mid[3], const float stored[3]) {
    if (!(flags & DH_TRACK_FLAG_SLUGGISH)) return true;
    const float d = dh_track_add_(dh_track_add_(fabsf(dh_track_sub_(mid[0], stored[0])), fabsf(dh_track_sub_(mid[1], stored[1]))),
                                  fabsf(dh_track_sub_(mid[2], stored[2])));
    return d < 100.0f || stored[2] < 500.0f;
}

// The next step's guess mask (bit0 midpoint, bit1 rotation; ClusterArgs::guess_mask): with --prevguess the stored midpoint is a
// guess when its z is above 500 (:79-86), the stored rotation whenever there is one (:101); without it neither.
DH_HD inline uint8_t dh_track_mask(uint32_t flags, const float stored[3], bool has_rot) {
    if (!(flags & DH_TRACK_FLAG_PREV_GUESS)) return 0;
    return (uint8_t)((stored[2] > 500.0f ? 1u : 0u) | (has_rot ? 2u : 0u));
}

// One camera's update after a step whose pose is (mid, rot): midpoint under the sluggish rule, rotation always (:100-101), mask.
DH_HD inline void dh_track_update(uint32_t flags, const float mid[3], const double rot[3], float midp[3], double stored_rot[3],
                                  uint8_t *mask, uint8_t *has_rot) {
    if (dh_track_takes_midp(flags, mid, midp)) { midp[0] = mid[0]; midp[1] = mid[1]; midp[2] = mid[2]; }
    stored_rot[0] = rot[0]; stored_rot[1] = rot[1]; stored_rot[2] = rot[2];
    *has_rot = 1;
    *mask = dh_track_mask(flags, midp, true);
}
