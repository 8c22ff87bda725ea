// dh_runtime_track.h -- what the trackers in dh_api.hip and the fit trackers' unit (dh_api_fit_track.hip) both use: the tracker
// core with its create, destroy, reset and state templates, the rig table and the rig tracker's handle, and the three functions
// of dh_api.hip that a fit tracker's step calls.  The structs and templates are static, as in dh_runtime.h.  Not part of the ABI;
// only those two units include it.
#pragma once
#include "dh_runtime.h"

// What both trackers share: the camera table they step, one frame per camera, and the device copy of a host step's present
// bytes.  Create, destroy, reset and the prelude of state are written once for either tracker type T (below); T supplies
// clear(c0, m, s), which puts the state of cameras [c0, c0 + m) back to its initial value on stream s.
struct TrackerCore {
    const dh_cameras *cams = nullptr;
    int n = 0;
    Buf<uint8_t> present;    // [n] host steps: the caller's present bytes on the device
};

// A tracker of type T over camera table c (the caller has checked its own arguments): init(t, n) sets t's parameters and allocates
// its state for n cameras, which clear() then sets for every camera before the call returns.  A tracker whose state is not per
// camera (a rig tracker's is per rig) passes the number of its state units as `states`.
template <typename T, typename F>
static int create_tracker(const dh_cameras *c, T **out, F init, size_t states = 0) {
    DeviceGuard guard(c->device);
    if (!guard.ok) return DH_EHIP;
    std::unique_ptr<T> t(new T);
    t->cams = c; t->n = c->n;
    const size_t n = (size_t)c->n;
    TRY(init(*t, n));
    TRY(t->present.alloc(n));
    TRY(t->clear(0, states ? states : n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    *out = t.release();
    return DH_OK;
}
template <typename T>
static int destroy_tracker(T *t) {
    if (!t) return DH_OK;
    DeviceGuard guard(t->cams->device);
    delete t;
    return DH_OK;
}
// One camera, or every camera for camera == -1, back to the initial state, ordered on `stream`; fn names the entry point.
// `units` (default: the cameras) and `unit` say what the index counts when the state is not per camera.
template <typename T>
static int reset_tracker(T *t, int camera, void *stream, const char *fn, int units = -1, const char *unit = "camera") {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", fn);
    if (units < 0) units = t->n;
    if (camera < -1 || camera >= units) return fail(DH_EINVAL, "%s: %s %d of %d", fn, unit, camera, units);
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    const size_t c0 = camera < 0 ? 0 : (size_t)camera, m = camera < 0 ? (size_t)units : 1;
    return t->clear(c0, m, (hipStream_t)stream);
}
// copy(n): the synchronous copies of a state call, once every step on the tracker's device is done; fn names the entry point.
template <typename F>
static int read_tracker(const TrackerCore *t, const char *fn, F copy) {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", fn);
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipDeviceSynchronize());          // the steps may run on any stream of the device
    return copy((size_t)t->n);
}

// A rig table: the extrinsics of every camera of a camera table and the camera ranges of the rigs, on the table's device.
struct dh_rig {
    const dh_cameras *cams = nullptr;
    int n_rigs = 0;
    Buf<RigCam> dev;            // [cams->n]
    Buf<int32_t> rig_begin;     // [n_rigs + 1]
    int largest = 0;            // cameras of the largest rig
};

// A rig tracker's state: DH_RIG_MAX_TRACKS track records and the next id per rig.  A step is a heads camera batch over the rig
// table's cameras followed by k_rig_fuse (dh_rig.h) once over all rigs.  The host steps keep every slice's heads on the device
// (heads, n_heads below) and fuse after the last slice, so that a resident limit smaller than a rig does not cut it in two.
struct dh_rig_tracker : TrackerCore {
    const dh_rig *rig = nullptr;
    dh_rig_track_params prm{};
    Buf<dh_rig_track> tracks;    // [n_rigs][DH_RIG_MAX_TRACKS]
    Buf<uint32_t> next_id;       // [n_rigs]
    // host steps: the whole table's heads for k_rig_fuse, and its outputs before their copy back
    Buf<dh_head> heads;          // [n][max_heads]
    Buf<uint32_t> n_heads;       // [n]
    Buf<uint32_t> ids;           // [n][max_heads]
    Buf<uint32_t> n_persons;     // [n_rigs]
    Buf<dh_rig_person> persons;  // [n_rigs][DH_RIG_MAX_PERSONS]
    // tracks zeroed, next ids 1, for rigs [g0, g0 + m)
    int clear(size_t g0, size_t m, hipStream_t s) {
        HIP_TRY(hipMemsetAsync(tracks.get() + g0 * DH_RIG_MAX_TRACKS, 0, m * DH_RIG_MAX_TRACKS * sizeof(dh_rig_track), s));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(next_id.get() + g0), 1, m, s));
        return DH_OK;
    }
};

// What a fit tracker's whole step runs of the predictor, defined in dh_api.hip (dh_host.h's names for internal symbols): the
// bodies of dh_predict_batch_cameras_support_device and dh_rig_tracker_step_device with their parameter lists, outside the
// entry points' guard, and the device a predictor lives on.
struct dh_predictor;
int dh_predict_batch_cameras_support_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                             const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                                             uint32_t radius, dh_pose *out, dh_support *support, void *stream);
int dh_rig_tracker_step_device_(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons,
                                dh_rig_track *tracks, void *stream);
int dh_predictor_device_(const dh_predictor *p);
