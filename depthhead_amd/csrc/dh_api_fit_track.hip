// dh_api_fit_track.hip -- the fit trackers' runtime, four trackers in two pairs.  What all four share: the angle table,
// FitTrackerCore, the creation check, the staging of a host step (fit_tracker_host).  The camera pair -- the camera fit tracker
//  and the subject fit tracker (section 29) -- stands on CamFitTrackerBase, the rig pair -- the rig fit
// tracker (section 22) and the rig subject fit tracker (section 30) -- on RigFitTrackerBase; each pair has one step check, one
// function that fills the argument blocks, one host form and its four step forms written once (section 31), with the tracker's
// core step (its launches) handed in.  The two subject trackers share SubjectParts and what goes with a binding.  Kernels:
// k_fit_track.hip, k_rig_fit_track.hip, k_subject_track.hip, k_rig_subject_track.hip, and the _sched launches of k_fit.hip and
// k_fit_views.hip.  Shares dh_runtime.h with every runtime unit, dh_runtime_fit.h with the fit family (dh_api_fit.hip), and
// dh_runtime_track.h with the trackers in dh_api.hip, which also defines the three functions of that header a whole step calls.
#include <math.h>
#include <string.h>

#include "dh_runtime.h"
#include "dh_fit.h"
#include "dh_runtime_fit.h"
#include "dh_runtime_track.h"

// ------------------------------------------------------------------ carrying fitted poses across steps
// The angle table of the header: computed once, by libm, and the only cosines and sines of the feature.
struct FitTrackAngles {
    double v[DH_FIT_TRACK_ANGLES][2];
    FitTrackAngles() {
        for (int i = 0; i < DH_FIT_TRACK_ANGLES; ++i) {
            const double a = (double)(i - 60) / 60.0 * 3.14159;
            v[i][0] = cos(a); v[i][1] = sin(a);
        }
    }
};
static const FitTrackAngles &fit_track_angles() {
    static const FitTrackAngles tab;
    return tab;
}
static int fit_tracker_angles_(double out[DH_FIT_TRACK_ANGLES][2]) {
    if (!out) return fail(DH_EINVAL, "dh_fit_tracker_angles: NULL argument");
    memcpy(out, fit_track_angles().v, sizeof fit_track_angles().v);
    return DH_OK;
}
static int fit_track_params_default_(dh_fit_track_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_fit_track_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->iterations_tracked = 6; p->keep_points = 30;
    p->rms_max = 5.0; p->max_jump = 150.0;
    p->conf_num = 1; p->conf_den = 50;
    p->min_windows = 1; p->max_coast = 3;
    return DH_OK;
}
// What a creation runs with: the defaults of P, or the caller's params where given.
template <typename P>
static P params_or_default(int (*defaults)(P *), const P *given) {
    P p;
    (void)defaults(&p);
    return given ? *given : p;
}

// What the camera's fit tracker (below) and the rig's (section 22) share: the model and what the acceptance rule reads, the
// tables every step reads, and for the host forms the tracker's own stream and the frames staged on it (they come with the first
// host step, for its frame size).  A tracker T adds its params (T::prm), its state, the buffers between its three launches and
// the staging buffers of its host forms (T::records among them); every device buffer of a step is allocated at creation.
struct FitTrackerCore : TrackerCore {
    const dh_fit_model *model = nullptr;
    float scale = 1.0f;
    uint32_t flags = 0;
    int64_t rms_lim = 0;
    double jump2 = 0.0;
    Buf<double> angles;                  // [120][2]
    Buf<FitModel> models;                // [1]
    Buf<uint32_t> sched, seed;           // [units][2], [units]: a unit is what one workgroup of the fit takes (a camera, a slot)
    hipStream_t s = nullptr;             // host forms
    Buf<uint16_t> frames;
    ~FitTrackerCore() { if (s) (void)hipStreamDestroy(s); }
    // The tail of a tracker's allocation: what the params come to, the shared tables for `units` units, and the stream.
    int init_fit(const dh_fit_model *m, float scale_, uint32_t flags_, double rms_max, double max_jump, size_t units) {
        model = m; scale = scale_; flags = flags_;
        rms_lim = (int64_t)(rms_max * rms_max * 1048576.0);
        jump2 = max_jump * max_jump;
        TRY(angles.alloc(DH_FIT_TRACK_ANGLES * 2));
        TRY(models.alloc(1));
        TRY(sched.alloc(units * 2)); TRY(seed.alloc(units));
        const FitModel fm{m->pts.get(), m->nrm.get(), m->n, 0};
        HIP_TRY(hipMemcpy(models.get(), &fm, sizeof fm, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(angles.get(), fit_track_angles().v, sizeof fit_track_angles().v, hipMemcpyHostToDevice));
        return hip_step(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate");
    }
};
// The refusals of the fields that only one params type has: the confidence fraction of a camera's, max_coast of a rig's.
static int fit_track_own_check(const dh_fit_track_params &prm, const char *who) {
    if (prm.conf_den == 0 || prm.conf_num > prm.conf_den)
        return fail(DH_EINVAL, "%s: confidence %u / %u, expected a fraction in [0, 1]", who, prm.conf_num, prm.conf_den);
    return DH_OK;
}
static int fit_track_own_check(const dh_rig_fit_track_params &prm, const char *who) {
    if (prm.max_coast > prm.max_misses)
        return fail(DH_EINVAL, "%s: max_coast %u above the max_misses %u the ids come from", who, prm.max_coast, prm.max_misses);
    return DH_OK;
}
// The refusals of a fit tracker's creation in the header's order.  P: dh_fit_track_params or dh_rig_fit_track_params (its own
// fields: fit_track_own_check); tables() gives the refusals of the tables and of the model beside them (NULL, device).
template <typename P, typename Tables>
static int fit_tracker_create_check(const P &prm, float scale, uint32_t flags, const dh_fit_model *m, Tables tables, const char *who) {
    if (flags & ~DH_FIT_TRACK_MOTION) return fail(DH_EINVAL, "%s: unknown flags 0x%x", who, flags);
    if (!std::isfinite(scale)) return fail(DH_EINVAL, "%s: scale is not finite", who);
    if (prm.iterations_tracked > 64) return fail(DH_EINVAL, "%s: iterations_tracked %u above 64", who, prm.iterations_tracked);
    if (!(prm.rms_max > 0.0 && prm.rms_max <= 4096.0)) return fail(DH_EINVAL, "%s: rms_max = %g outside (0, 4096]", who, prm.rms_max);
    if (!(prm.max_jump > 0.0 && prm.max_jump <= 4096.0)) return fail(DH_EINVAL, "%s: max_jump = %g outside (0, 4096]", who, prm.max_jump);
    TRY(fit_track_own_check(prm, who));
    if (prm.reserved[0] || prm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    TRY(tables());
    if (!m) return fail(DH_EINVAL, "%s: NULL model", who);     // (tables() refuses it in its place: m is never read unchecked)
    const double extent = fabs((double)scale) * m->radius;
    if (extent > DH_FIT_MAX_EXTENT) return fail(DH_EINVAL, "%s: the model spans %g mm from its origin (limit %g)", who, extent, DH_FIT_MAX_EXTENT);
    return DH_OK;
}
// (a step may still run on any stream of the device)
template <typename T>
static int destroy_fit_tracker(T *t) {
    if (t) {
        DeviceGuard guard(t->cams->device);
        (void)hipDeviceSynchronize();
    }
    return destroy_tracker(t);
}
// The host form of a step of fit tracker t (any of the four; the pairs' host forms, cam_fit_host and rig_fit_host, fill in the
// three functions), synchronous on its own stream: the frames and the present bytes are staged,
// upload(s) stages the caller's other inputs, step(frames, present, s) enqueues the step on the staged arrays (present: the
// staged bytes or NULL), download(s) copies back what the step reports beside its records, and the n_rec records follow.
template <typename T, typename Up, typename Step, typename Down, typename Rec>
static int fit_tracker_host(T *t, const uint16_t *frames, int w, int h, const uint8_t *present, Up upload, Step step, Down download, Rec *records,
                            size_t n_rec) {
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    const size_t n = (size_t)t->n, n_px = n * w * h;
    if (t->frames.cap() < n_px) TRY(t->frames.alloc(n_px));       // (host steps are synchronous: nothing reads the old buffer)
    hipStream_t s = t->s;
    HIP_TRY(hipMemcpyAsync(t->frames.get(), frames, n_px * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    if (present) HIP_TRY(hipMemcpyAsync(t->present.get(), present, n, hipMemcpyHostToDevice, s));
    TRY(upload(s));
    const int rc = step(t->frames.get(), present ? t->present.get() : nullptr, s);
    if (rc != DH_OK) { (void)hipStreamSynchronize(s); return rc; }
    TRY(download(s));
    HIP_TRY(hipMemcpyAsync(records, t->records.get(), n_rec * sizeof(Rec), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DH_OK;
}

// A FitTrackerCore whose units are the cameras.  What the camera fit tracker and the subject fit tracker (section 29) share:
// everything but the state, the records and what a binding needs.
struct CamFitTrackerBase : FitTrackerCore {
    dh_fit_track_params prm{};
    Buf<dh_render_instance> start, fit_out;  // [n]
    Buf<dh_fit_record> fit_rec;
    Buf<dh_pose> poses;                  // host forms
    Buf<dh_support> support;
    // the params and every buffer above for n cameras
    int alloc_cam(const dh_fit_track_params &prm_, size_t n) {
        prm = prm_;
        TRY(start.alloc(n)); TRY(fit_out.alloc(n)); TRY(fit_rec.alloc(n));
        TRY(poses.alloc(n)); TRY(support.alloc(n));
        return DH_OK;
    }
};
struct dh_fit_tracker : CamFitTrackerBase {
    Buf<dh_fit_track_state> state;       // [n]
    Buf<dh_fit_track_record> records;    // host forms
    int clear(size_t c0, size_t m, hipStream_t st) {
        HIP_TRY(hipMemsetAsync(state.get() + c0, 0, m * sizeof(dh_fit_track_state), st));
        return DH_OK;
    }
};
static int fit_tracker_create_(const dh_cameras *c, const dh_fit_model *m, float scale, uint32_t flags, const dh_fit_track_params *params,
                               dh_fit_tracker **out) {
    const char *who = "dh_fit_tracker_create";
    if (!out) return fail(DH_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    const dh_fit_track_params prm = params_or_default(fit_track_params_default_, params);
    TRY(fit_tracker_create_check(prm, scale, flags, m, [&]() -> int {
        if (!c) return fail(DH_EINVAL, "%s: NULL camera table", who);
        if (!m) return fail(DH_EINVAL, "%s: NULL model", who);
        if (m->device != c->device) return fail(DH_EINVAL, "%s: the model lives on device %d, the camera table on %d", who, m->device, c->device);
        return DH_OK;
    }, who));
    return create_tracker(c, out, [&](dh_fit_tracker &t, size_t n) -> int {
        TRY(t.alloc_cam(prm, n));
        TRY(t.state.alloc(n)); TRY(t.records.alloc(n));
        return t.init_fit(m, scale, flags, prm.rms_max, prm.max_jump, n);
    });
}
static int fit_tracker_destroy_(dh_fit_tracker *t) { return destroy_fit_tracker(t); }
static int fit_tracker_reset_(dh_fit_tracker *t, int camera, void *stream) { return reset_tracker(t, camera, stream, "dh_fit_tracker_reset"); }
// The synchronous copy of the state of tracker t of the camera pair, [n] entries of St; who names the entry point.
template <typename T, typename St>
static int cam_fit_state(T *t, St *states, const char *who) {
    if (t && !states) return fail(DH_EINVAL, "%s: NULL argument", who);
    return read_tracker(t, who, [&](size_t n) -> int {
        HIP_TRY(hipMemcpy(states, t->state.get(), n * sizeof(St), hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int fit_tracker_state_(dh_fit_tracker *t, dh_fit_track_state *states) { return cam_fit_state(t, states, "dh_fit_tracker_state"); }
// The refusals of a step that are the tracker's own, before anything is launched: one rule for both trackers of the pair.
static int cam_fit_check(const CamFitTrackerBase *t, const void *frames, int w, int h, const void *poses, const void *support,
                         const dh_fit_params *in, const void *records, dh_fit_params *prm, const char *who) {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (!frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!poses || !support) return fail(DH_EINVAL, "%s: NULL poses or support", who);
    if (!records) return fail(DH_EINVAL, "%s: NULL records", who);
    TRY(check_frame_size(w, h, who));
    return fit_params_check(in, prm, who);
}
// The argument blocks of a step's seed and update kernels (a; its state and records are the caller's to set) and of the fit
// between them (f).
static void cam_fit_args(CamFitTrackerBase *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses,
                         const dh_support *support, const dh_fit_params &prm, FitTrackArgs &a, FitSchedArgs &f) {
    memset(&a, 0, sizeof a);
    a.n = t->n; a.flags = t->flags; a.scale = t->scale; a.prm = t->prm; a.rms_lim = t->rms_lim; a.jump2 = t->jump2;
    a.coarse = prm.coarse_iterations; a.full = prm.iterations;
    a.angles = t->angles.get(); a.present = present; a.poses = poses; a.support = support;
    a.start = t->start.get(); a.sched = t->sched.get(); a.seed = t->seed.get();
    a.fit_out = t->fit_out.get(); a.fit_rec = t->fit_rec.get();
    memset(&f, 0, sizeof f);
    f.f.frames = frames; f.f.n = t->n; f.f.w = w; f.f.h = h;
    f.f.cams = t->cams->dev.get(); f.f.models = t->models.get(); f.f.inst = t->start.get(); f.f.n_inst = (uint32_t)t->n;
    fit_args_params(f.f, prm);                             // (k_fit_sched reads coarse and full per instance from sched)
    f.f.out = t->fit_out.get(); f.f.rec = t->fit_rec.get();
    f.sched = t->sched.get(); f.seed = t->seed.get();
}
// Steps 0 - 6 for every camera, on device arrays and stream s (arguments checked, device selected): three launches.
static int fit_track_enqueue(dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses,
                             const dh_support *support, const dh_fit_params &prm, dh_fit_track_record *records, hipStream_t s) {
    FitTrackArgs a;
    FitSchedArgs f;
    cam_fit_args(t, frames, w, h, present, poses, support, prm, a, f);
    a.state = t->state.get(); a.records = records;
    TRY(hip_step(dh_launch_fit_track_seed(a, s), "k_fit_track_seed"));
    TRY(hip_step(dh_launch_fit_sched(f, s), "k_fit_sched"));
    TRY(hip_step(dh_launch_fit_track_update(a, s), "k_fit_track_update"));
    return DH_OK;
}
// The four forms of a step, written once for the camera pair.  T: either tracker; Rec: its record; enqueue: its core step on
// device arrays (fit_track_enqueue's parameter list); who names the entry point.  The _device forms allocate nothing and never
// wait on the host.
template <typename T, typename Rec, typename Enqueue>
static int cam_fit_step_poses_device(const char *who, Enqueue enqueue, T *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                     const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, Rec *records,
                                     void *stream) {
    dh_fit_params prm;
    TRY(cam_fit_check(t, frames, w, h, poses, support, fit_params, records, &prm, who));
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return enqueue(t, frames, w, h, present, poses, support, prm, records, (hipStream_t)stream);
}
template <typename T, typename Rec, typename Enqueue>
static int cam_fit_step_device(const char *who, Enqueue enqueue, dh_predictor *p, T *t, const uint16_t *frames, int w, int h,
                               const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out,
                               dh_support *support_out, Rec *records, void *stream) {
    dh_fit_params prm;
    if (!p) return fail(DH_EINVAL, "%s: NULL predictor", who);
    TRY(cam_fit_check(t, frames, w, h, poses_out, support_out, fit_params, records, &prm, who));
    TRY(dh_predict_batch_cameras_support_device_(p, frames, t->n, w, h, t->cams, nullptr, nullptr, nullptr, radius, poses_out, support_out, stream));
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return enqueue(t, frames, w, h, present, poses_out, support_out, prm, records, (hipStream_t)stream);
}
// The host forms: everything staged through the tracker's buffers on its own stream; synchronous.  p NULL: the core step on
// the caller's poses and support; else the prediction first, its poses and support copied back too.
template <typename T, typename Rec, typename Enqueue>
static int cam_fit_host(dh_predictor *p, T *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius,
                        const dh_fit_params &prm, dh_pose *poses, dh_support *support, Rec *records, Enqueue enqueue) {
    const size_t n = (size_t)t->n;
    return fit_tracker_host(t, frames, w, h, present, [&](hipStream_t s) -> int {
        if (p) return DH_OK;
        HIP_TRY(hipMemcpyAsync(t->poses.get(), poses, n * sizeof(dh_pose), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->support.get(), support, n * sizeof(dh_support), hipMemcpyHostToDevice, s));
        return DH_OK;
    }, [&](const uint16_t *fr, const uint8_t *pr, hipStream_t s) -> int {
        if (p) TRY(dh_predict_batch_cameras_support_device_(p, fr, t->n, w, h, t->cams, nullptr, nullptr, nullptr, radius, t->poses.get(),
                                                         t->support.get(), s));
        return enqueue(t, fr, w, h, pr, t->poses.get(), t->support.get(), prm, t->records.get(), s);
    }, [&](hipStream_t s) -> int {
        if (!p) return DH_OK;
        HIP_TRY(hipMemcpyAsync(poses, t->poses.get(), n * sizeof(dh_pose), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(support, t->support.get(), n * sizeof(dh_support), hipMemcpyDeviceToHost, s));
        return DH_OK;
    }, records, n);
}
template <typename T, typename Rec, typename Enqueue>
static int cam_fit_step_poses(const char *who, Enqueue enqueue, T *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                              const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, Rec *records) {
    dh_fit_params prm;
    TRY(cam_fit_check(t, frames, w, h, poses, support, fit_params, records, &prm, who));
    return cam_fit_host(nullptr, t, frames, w, h, present, 0, prm, const_cast<dh_pose *>(poses), const_cast<dh_support *>(support), records, enqueue);
}
template <typename T, typename Rec, typename Enqueue>
static int cam_fit_step(const char *who, Enqueue enqueue, dh_predictor *p, T *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                        uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, Rec *records) {
    dh_fit_params prm;
    if (!p) return fail(DH_EINVAL, "%s: NULL predictor", who);
    TRY(cam_fit_check(t, frames, w, h, poses_out, support_out, fit_params, records, &prm, who));
    if (radius > 0x7fffffffu) return fail(DH_EINVAL, "%s: radius %u (a negative int?); expected 0 .. 2^31 - 1", who, radius);
    if (t->cams->device != dh_predictor_device_(p))
        return fail(DH_EINVAL, "%s: camera table on device %d, predictor on device %d", who, t->cams->device, dh_predictor_device_(p));
    return cam_fit_host(p, t, frames, w, h, present, radius, prm, poses_out, support_out, records, enqueue);
}
// The entry points' forwards (DH_API below gives each its parameter list, which the shared form checks against its own).
template <typename... A> static int fit_tracker_step_poses_device_(A... a) { return cam_fit_step_poses_device("dh_fit_tracker_step_poses_device", fit_track_enqueue, a...); }
template <typename... A> static int fit_tracker_step_device_(A... a) { return cam_fit_step_device("dh_fit_tracker_step_device", fit_track_enqueue, a...); }
template <typename... A> static int fit_tracker_step_poses_(A... a) { return cam_fit_step_poses("dh_fit_tracker_step_poses", fit_track_enqueue, a...); }
template <typename... A> static int fit_tracker_step_(A... a) { return cam_fit_step("dh_fit_tracker_step", fit_track_enqueue, a...); }

// ------------------------------------------------------------------ carrying each rig person's fitted world pose
static int rig_fit_track_params_default_(dh_rig_fit_track_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_rig_fit_track_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->iterations_tracked = 6; p->keep_points = 30;
    p->rms_max = 5.0; p->max_jump = 150.0;
    p->max_coast = 3; p->max_misses = DH_TRACK_MAX_MISSES;
    return DH_OK;
}

// A FitTrackerCore (section 19) whose state is per rig (DH_RIG_MAX_TRACKS entries each) and whose units are the slots; every
// device buffer of a step is sized by the rig table and allocated at creation.
// What the rig fit tracker and the rig subject fit tracker (section 30) share: everything but the records and what a binding needs.
struct RigFitTrackerBase : FitTrackerCore {
    const dh_rig *rig = nullptr;
    const dh_fit_views *views = nullptr;
    dh_rig_fit_track_params prm{};
    Buf<dh_rig_fit_state> state;         // [n_rigs][DH_RIG_MAX_TRACKS]
    Buf<dh_view_instance> start, fit_out;    // [slots]
    Buf<dh_view_fit_record> fit_rec;
    Buf<uint32_t> who;
    Buf<dh_head> heads;                  // host forms: [n][DH_MAX_HEADS]
    Buf<uint32_t> n_heads, ids, n_persons;
    Buf<dh_rig_person> persons;          // [n_rigs][DH_RIG_MAX_PERSONS]
    Buf<dh_rig_track> tracks;            // [n_rigs][DH_RIG_MAX_TRACKS]
    // the tables, the params and every buffer above for n cameras
    int alloc_rig(const dh_rig *rig_, const dh_fit_views *views_, const dh_rig_fit_track_params &prm_, size_t n) {
        rig = rig_; views = views_; prm = prm_;
        const size_t ng = (size_t)rig->n_rigs, slots = ng * DH_RIG_MAX_TRACKS;
        TRY(state.alloc(slots));
        TRY(start.alloc(slots)); TRY(fit_out.alloc(slots)); TRY(fit_rec.alloc(slots));
        TRY(who.alloc(slots));
        TRY(heads.alloc(n * DH_MAX_HEADS)); TRY(n_heads.alloc(n)); TRY(ids.alloc(n * DH_MAX_HEADS));
        TRY(n_persons.alloc(ng)); TRY(persons.alloc(ng * DH_RIG_MAX_PERSONS)); TRY(tracks.alloc(ng * DH_RIG_MAX_TRACKS));
        return DH_OK;
    }
    int clear(size_t g0, size_t m, hipStream_t st) {
        HIP_TRY(hipMemsetAsync(state.get() + g0 * DH_RIG_MAX_TRACKS, 0, m * DH_RIG_MAX_TRACKS * sizeof(dh_rig_fit_state), st));
        return DH_OK;
    }
};
struct dh_rig_fit_tracker : RigFitTrackerBase {
    Buf<dh_rig_fit_record> records;      // [slots]
};
// The refusal of a rig whose largest view sum is above what a multi-view fit takes: `points` per view (the model's, which the
// models of a set share).
static int rig_terms_check(const dh_rig *rig, uint32_t points, const char *who) {
    const int64_t largest = rig->largest;
    if ((uint64_t)largest * points > DH_FIT_MAX_POINTS)
        return fail(DH_EINVAL, "%s: a rig of %lld cameras sums %llu terms of a %u-point model, above %u", who, (long long)largest,
                    (unsigned long long)((uint64_t)largest * points), points, DH_FIT_MAX_POINTS);
    return DH_OK;
}
static int rig_fit_tracker_create_(const dh_rig *rig, const dh_fit_views *views, const dh_fit_model *m, float scale, uint32_t flags,
                                   const dh_rig_fit_track_params *params, dh_rig_fit_tracker **out) {
    const char *who = "dh_rig_fit_tracker_create";
    if (!out) return fail(DH_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    const dh_rig_fit_track_params prm = params_or_default(rig_fit_track_params_default_, params);
    TRY(fit_tracker_create_check(prm, scale, flags, m, [&]() -> int {
        if (!rig) return fail(DH_EINVAL, "%s: NULL rig table", who);
        if (!views) return fail(DH_EINVAL, "%s: NULL view table", who);
        if (!m) return fail(DH_EINVAL, "%s: NULL model", who);
        if (views->cams != rig->cams) return fail(DH_EINVAL, "%s: the rig table and the view table are bound to different camera tables", who);
        if (m->device != rig->cams->device)
            return fail(DH_EINVAL, "%s: the model lives on device %d, the tables on %d", who, m->device, rig->cams->device);
        return DH_OK;
    }, who));
    TRY(rig_terms_check(rig, m->n, who));
    const size_t ng = (size_t)rig->n_rigs, slots = ng * DH_RIG_MAX_TRACKS;
    return create_tracker(rig->cams, out, [&](dh_rig_fit_tracker &t, size_t n) -> int {
        TRY(t.alloc_rig(rig, views, prm, n));
        TRY(t.records.alloc(slots));
        return t.init_fit(m, scale, flags, prm.rms_max, prm.max_jump, slots);
    }, ng);
}
static int rig_fit_tracker_destroy_(dh_rig_fit_tracker *t) { return destroy_fit_tracker(t); }
static int rig_fit_tracker_reset_(dh_rig_fit_tracker *t, int rig, void *stream) {
    return reset_tracker(t, rig, stream, "dh_rig_fit_tracker_reset", t ? t->rig->n_rigs : 0, "rig");
}
static int rig_fit_tracker_state_(dh_rig_fit_tracker *t, dh_rig_fit_state *states) {
    if (t && !states) return fail(DH_EINVAL, "dh_rig_fit_tracker_state: NULL argument");
    return read_tracker(t, "dh_rig_fit_tracker_state", [&](size_t) -> int {
        HIP_TRY(hipMemcpy(states, t->state.get(), (size_t)t->rig->n_rigs * DH_RIG_MAX_TRACKS * sizeof(dh_rig_fit_state), hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
// The refusals of a step that are the tracker's own, before anything is launched.
static int rig_fit_check(const RigFitTrackerBase *t, const void *frames, int w, int h, int max_heads, const void *n_heads, const void *heads,
                         const void *n_persons, const void *persons, const dh_fit_params *in, const void *records, dh_fit_params *prm,
                         const char *who) {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (!frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!n_heads || !heads) return fail(DH_EINVAL, "%s: NULL heads", who);
    if (!n_persons || !persons) return fail(DH_EINVAL, "%s: NULL persons", who);
    if (!records) return fail(DH_EINVAL, "%s: NULL records", who);
    TRY(check_frame_size(w, h, who));
    if (max_heads < 1 || max_heads > DH_MAX_HEADS) return fail(DH_EINVAL, "%s: max_heads %d outside 1 .. %d", who, max_heads, DH_MAX_HEADS);
    return fit_params_check(in, prm, who);
}
// The argument blocks of a step's seed and update kernels (a; its records are the caller's to set) and of the fit between them (f).
static void rig_fit_args(RigFitTrackerBase *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                         const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons,
                         const dh_fit_params &prm, RigFitArgs &a, FitViewsSchedArgs &f) {
    memset(&a, 0, sizeof a);
    a.n_rigs = t->rig->n_rigs; a.n_cams = t->n; a.max_heads = max_heads;
    a.flags = t->flags; a.scale = t->scale; a.prm = t->prm; a.rms_lim = t->rms_lim; a.jump2 = t->jump2;
    a.coarse = prm.coarse_iterations; a.full = prm.iterations;
    a.angles = t->angles.get(); a.rig_begin = t->rig->rig_begin.get(); a.views = t->views->dev.get();
    a.present = present; a.n_heads = n_heads; a.heads = heads; a.n_persons = n_persons; a.persons = persons;
    a.state = t->state.get(); a.start = t->start.get(); a.sched = t->sched.get(); a.seed = t->seed.get(); a.who = t->who.get();
    a.fit_out = t->fit_out.get(); a.fit_rec = t->fit_rec.get();
    memset(&f, 0, sizeof f);
    f.f.frames = frames; f.f.n = t->n; f.f.w = w; f.f.h = h;
    f.f.cams = t->cams->dev.get(); f.f.views = t->views->dev.get(); f.f.models = t->models.get();
    f.f.inst = t->start.get(); f.f.n_inst = (uint32_t)(a.n_rigs * DH_RIG_MAX_TRACKS);
    fit_args_params(f.f, prm);                                   // (k_fit_views_sched reads coarse and full per slot from sched)
    f.f.out = t->fit_out.get(); f.f.rec = t->fit_rec.get();
    f.sched = t->sched.get(); f.seed = t->seed.get(); f.group = DH_RIG_MAX_TRACKS;
}
// Steps 0 - 6 for every rig, on device arrays and stream s (arguments checked, device selected): three launches, and nothing
// uploaded but their arguments.
static int rig_fit_enqueue(dh_rig_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                           const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons,
                           const dh_fit_params &prm, dh_rig_fit_record *records, hipStream_t s) {
    RigFitArgs a;
    FitViewsSchedArgs f;
    rig_fit_args(t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, prm, a, f);
    a.records = records;
    TRY(hip_step(dh_launch_rig_fit_seed(a, s), "k_rig_fit_seed"));
    TRY(hip_step(dh_launch_fit_views_sched(f, s), "k_fit_views_sched"));
    TRY(hip_step(dh_launch_rig_fit_update(a, s), "k_rig_fit_update"));
    return DH_OK;
}
// The four forms of a step, written once for the rig pair.  T: either rig tracker; Rec: its record; enqueue: its core step on
// device arrays (rig_fit_enqueue's parameter list); who names the entry point.  The _device forms allocate nothing and never
// wait on the host.
template <typename T, typename Rec, typename Enqueue>
static int rig_fit_step_persons_device(const char *who, Enqueue enqueue, T *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                       int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons,
                                       const dh_rig_person *persons, const dh_fit_params *fit_params, Rec *records, void *stream) {
    dh_fit_params prm;
    TRY(rig_fit_check(t, frames, w, h, max_heads, n_heads, heads, n_persons, persons, fit_params, records, &prm, who));
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return enqueue(t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, prm, records, (hipStream_t)stream);
}
// The refusals of the whole step beyond the core step's: the rig tracker must step the tracker's own rig table and must not
// drop an id sooner than the tracker stops coasting on it.
static int rig_fit_step_check(const dh_predictor *p, const RigFitTrackerBase *t, const dh_rig_tracker *rt, const void *frames, int w, int h,
                              const void *n_heads, const void *heads, const void *ids, const void *n_persons, const void *persons,
                              const dh_fit_params *in, const void *records, dh_fit_params *prm, const char *who) {
    if (!p) return fail(DH_EINVAL, "%s: NULL predictor", who);
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (!rt) return fail(DH_EINVAL, "%s: NULL rig tracker", who);
    TRY(rig_fit_check(t, frames, w, h, rt->prm.max_heads, n_heads, heads, n_persons, persons, in, records, prm, who));
    if (!ids) return fail(DH_EINVAL, "%s: NULL rig_ids", who);
    if (rt->rig != t->rig) return fail(DH_EINVAL, "%s: the rig tracker steps another rig table than the fit tracker's", who);
    if (rt->prm.max_misses < t->prm.max_coast)
        return fail(DH_EINVAL, "%s: the rig tracker's max_misses %u is below the fit tracker's max_coast %u", who, rt->prm.max_misses, t->prm.max_coast);
    return DH_OK;
}
template <typename T, typename Rec, typename Enqueue>
static int rig_fit_step_device(const char *who, Enqueue enqueue, dh_predictor *p, T *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h,
                               const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *ids,
                               uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, Rec *records, void *stream) {
    dh_fit_params prm;
    TRY(rig_fit_step_check(p, t, rt, frames, w, h, n_heads, heads, ids, n_persons, persons, fit_params, records, &prm, who));
    TRY(dh_rig_tracker_step_device_(p, rt, frames, w, h, present, n_heads, heads, ids, n_persons, persons, tracks, stream));
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return enqueue(t, frames, w, h, present, rt->prm.max_heads, n_heads, heads, n_persons, persons, prm, records, (hipStream_t)stream);
}
// The host forms: everything staged through the tracker's buffers on its own stream; synchronous.  p NULL: the core step on
// the caller's heads and persons; else the rig step first (its device form, on the staged frames), its outputs copied back too.
// T: either rig tracker; enqueue: its core step on device arrays (rig_fit_enqueue's parameter list).
template <typename T, typename Rec, typename Enqueue>
static int rig_fit_host(dh_predictor *p, T *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h, const uint8_t *present,
                        int max_heads, const dh_fit_params &prm, uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons,
                        dh_rig_person *persons, dh_rig_track *tracks, Rec *records, Enqueue enqueue) {
    const size_t n = (size_t)t->n, ng = (size_t)t->rig->n_rigs, mh = (size_t)max_heads;
    return fit_tracker_host(t, frames, w, h, present, [&](hipStream_t s) -> int {
        if (p) return DH_OK;
        HIP_TRY(hipMemcpyAsync(t->n_heads.get(), n_heads, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->heads.get(), heads, n * mh * sizeof(dh_head), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->n_persons.get(), n_persons, ng * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->persons.get(), persons, ng * DH_RIG_MAX_PERSONS * sizeof(dh_rig_person), hipMemcpyHostToDevice, s));
        return DH_OK;
    }, [&](const uint16_t *fr, const uint8_t *pr, hipStream_t s) -> int {
        if (p) TRY(dh_rig_tracker_step_device_(p, rt, fr, w, h, pr, t->n_heads.get(), t->heads.get(), t->ids.get(), t->n_persons.get(),
                                            t->persons.get(), tracks ? t->tracks.get() : nullptr, s));
        return enqueue(t, fr, w, h, pr, max_heads, t->n_heads.get(), t->heads.get(), t->n_persons.get(), t->persons.get(), prm,
                       t->records.get(), s);
    }, [&](hipStream_t s) -> int {
        if (!p) return DH_OK;
        HIP_TRY(hipMemcpyAsync(n_heads, t->n_heads.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(heads, t->heads.get(), n * mh * sizeof(dh_head), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(ids, t->ids.get(), n * mh * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(n_persons, t->n_persons.get(), ng * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(persons, t->persons.get(), ng * DH_RIG_MAX_PERSONS * sizeof(dh_rig_person), hipMemcpyDeviceToHost, s));
        if (tracks) HIP_TRY(hipMemcpyAsync(tracks, t->tracks.get(), ng * DH_RIG_MAX_TRACKS * sizeof(dh_rig_track), hipMemcpyDeviceToHost, s));
        return DH_OK;
    }, records, ng * DH_RIG_MAX_TRACKS);
}
template <typename T, typename Rec, typename Enqueue>
static int rig_fit_step_persons(const char *who, Enqueue enqueue, T *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                                const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons,
                                const dh_fit_params *fit_params, Rec *records) {
    dh_fit_params prm;
    TRY(rig_fit_check(t, frames, w, h, max_heads, n_heads, heads, n_persons, persons, fit_params, records, &prm, who));
    return rig_fit_host(nullptr, t, nullptr, frames, w, h, present, max_heads, prm, const_cast<uint32_t *>(n_heads), const_cast<dh_head *>(heads),
                        nullptr, const_cast<uint32_t *>(n_persons), const_cast<dh_rig_person *>(persons), nullptr, records, enqueue);
}
template <typename T, typename Rec, typename Enqueue>
static int rig_fit_step(const char *who, Enqueue enqueue, dh_predictor *p, T *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h,
                        const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *ids,
                        uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, Rec *records) {
    dh_fit_params prm;
    TRY(rig_fit_step_check(p, t, rt, frames, w, h, n_heads, heads, ids, n_persons, persons, fit_params, records, &prm, who));
    if (t->cams->device != dh_predictor_device_(p))
        return fail(DH_EINVAL, "%s: rig table on device %d, predictor on device %d", who, t->cams->device, dh_predictor_device_(p));
    return rig_fit_host(p, t, rt, frames, w, h, present, rt->prm.max_heads, prm, n_heads, heads, ids, n_persons, persons, tracks, records, enqueue);
}
// The entry points' forwards, as the camera fit tracker's.
template <typename... A> static int rig_fit_tracker_step_persons_device_(A... a) { return rig_fit_step_persons_device("dh_rig_fit_tracker_step_persons_device", rig_fit_enqueue, a...); }
template <typename... A> static int rig_fit_tracker_step_device_(A... a) { return rig_fit_step_device("dh_rig_fit_tracker_step_device", rig_fit_enqueue, a...); }
template <typename... A> static int rig_fit_tracker_step_persons_(A... a) { return rig_fit_step_persons("dh_rig_fit_tracker_step_persons", rig_fit_enqueue, a...); }
template <typename... A> static int rig_fit_tracker_step_(A... a) { return rig_fit_step("dh_rig_fit_tracker_step", rig_fit_enqueue, a...); }

// ------------------------------------------------------------------ following each tracked head with its own subject's model
static int subject_track_params_default_(dh_subject_track_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_subject_track_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->retry = 4; p->max_tries = 4;
    return DH_OK;
}

// What the subject fit tracker and the rig subject fit tracker (section 30) hold beside their fit tracker: the set and the params
// of a binding, and what an identification needs whatever its score record is -- the mask, the list and the poses of the pair
// scratch.  A unit is what may want identification: a camera, a slot of a rig.
struct SubjectParts {
    const dh_fit_subjects *set = nullptr;
    SubjectsView sv{};
    dh_ident_params iprm{};
    dh_subject_track_params sprm{};
    uint32_t grid = 0;                   // workgroups of the score kernel
    Buf<uint8_t> enrolled;               // [S]: ones for "all"
    Buf<uint32_t> want, n_want, wants;   // [units], [1], [units]
    Buf<float> pose;                     // [units][S][12]
    // the mask on the device, ordered on st; the caller's memory is free when this returns
    int put_enrolled(const uint8_t *mask, hipStream_t st) {
        if (!mask) { HIP_TRY(hipMemsetAsync(enrolled.get(), 1, sv.n_subjects, st)); return DH_OK; }
        HIP_TRY(hipMemcpyAsync(enrolled.get(), mask, sv.n_subjects, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return DH_OK;
    }
    // Everything above for `units` units on `device` (the grid: min(units * S, 2 * the compute units)), and in `models` the table
    // of S + 1 models -- the set's, then the generic one -- in place of a FitTrackerCore's one.
    int init_subjects(const dh_fit_subjects *set_, const dh_fit_model *m, const dh_ident_params &iprm_, const dh_subject_track_params &sprm_,
                      size_t units, int device, Buf<FitModel> &models, const uint8_t *mask) {
        set = set_; iprm = iprm_; sprm = sprm_;
        std::vector<FitModel> table;
        dh_fit_subjects_view_(set, &sv, nullptr);
        const uint32_t S = sv.n_subjects;
        table.resize((size_t)S + 1);
        dh_fit_subjects_view_(set, &sv, table.data());
        table[S] = FitModel{m->pts.get(), m->nrm.get(), m->n, 0};
        const uint64_t pairs = (uint64_t)units * S;
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        grid = (uint32_t)std::min<uint64_t>(pairs, 2ull * (uint64_t)std::max(prop.multiProcessorCount, 1));
        TRY(enrolled.alloc(S)); TRY(want.alloc(units)); TRY(n_want.alloc(1)); TRY(wants.alloc(units));
        TRY(pose.alloc((size_t)pairs * 12));
        TRY(models.alloc((size_t)S + 1));
        HIP_TRY(hipMemcpy(models.get(), table.data(), table.size() * sizeof(FitModel), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(n_want.get(), 0, sizeof(uint32_t)));
        HIP_TRY(hipMemset(wants.get(), 0, units * sizeof(uint32_t)));
        return put_enrolled(mask, nullptr);
    }
    // The half of an IdentArgs or IdentViewsArgs that the set and the tracker's params fill.
    template <typename G>
    void ident_args(G &q) const {
        q.f.coarse = 0; q.f.full = iprm.iterations; q.f.min_points = iprm.min_points;
        q.f.gate[0] = iprm.gate; q.f.gate[1] = iprm.gate;
        q.f.lam1 = 1.0 + iprm.lambda;
        q.models = sv.table; q.np = sv.n; q.n_subjects = sv.n_subjects;
        q.radius = sv.radius; q.largest = sv.largest;
        q.enrolled = enrolled.get(); q.pose = pose.get();
        q.max_ms = iprm.max_rms * iprm.max_rms; q.min_ratio = iprm.min_ratio;
    }
};

// What the creation of either subject tracker refuses after its NULL handles (set and m are not NULL), in the header's order: the
// ident params by ident_check (dh_ident_params_check_ or dh_ident_views_params_check_; *iprm is what the tracker runs with), the
// reserved words of sprm, and the set (*sv) and the generic model against `device`, where `tables` live, and against each other.
static int subject_create_check(const dh_fit_subjects *set, const dh_fit_model *m, float scale, const dh_ident_params *ident_params,
                                int (*ident_check)(const dh_ident_params *, dh_ident_params *, const char *),
                                const dh_subject_track_params &sprm, int device, const char *tables, dh_ident_params *iprm, SubjectsView *sv,
                                const char *who) {
    TRY(ident_check(ident_params, iprm, who));
    if (sprm.reserved[0] || sprm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the dh_subject_track_params is not 0", who);
    dh_fit_subjects_view_(set, sv, nullptr);
    if (sv->device != device) return fail(DH_EINVAL, "%s: the subject set lives on device %d, the %s on %d", who, sv->device, tables, device);
    if (m->device != device) return fail(DH_EINVAL, "%s: the model lives on device %d, the %s on %d", who, m->device, tables, device);
    if (m->n != sv->n) return fail(DH_EINVAL, "%s: the generic model has %u points, a model of the set %u", who, m->n, sv->n);
    const double extent = fabs((double)scale) * sv->radius;
    if (extent > DH_FIT_MAX_EXTENT)
        return fail(DH_EINVAL, "%s: a model of the set may span %g mm from its origin (limit %g)", who, extent, DH_FIT_MAX_EXTENT);
    return DH_OK;
}
// What either subject tracker T reports of itself (`units`: its cameras or its rigs) and the change of its mask.
template <typename T>
static int subject_tracker_info(const T *t, int units, int *n_units, uint32_t *n_subjects, uint32_t *score_workgroups, const char *who) {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (n_units) *n_units = units;
    if (n_subjects) *n_subjects = t->sv.n_subjects;
    if (score_workgroups) *score_workgroups = t->grid;
    return DH_OK;
}
template <typename T>
static int subject_tracker_set_enrolled(T *t, const uint8_t *enrolled, void *stream, const char *who) {
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return t->put_enrolled(enrolled, (hipStream_t)stream);
}

// A CamFitTrackerBase whose model table holds the set's S models and the generic one at index S (core.model: the generic one), whose
// state carries each camera's binding, and which owns what an identification needs: the mask, the list and the pair scratch.
struct dh_subject_fit_tracker : CamFitTrackerBase, SubjectParts {
    Buf<dh_subject_track_state> state;   // [n]
    Buf<dh_fit_record> score;            // [n][S]
    Buf<dh_subject_track_record> records;    // host forms
    // zeros, and DH_IDENT_UNKNOWN (every byte 0xFF) in the subject word of each state
    int clear(size_t c0, size_t m, hipStream_t st) {
        HIP_TRY(hipMemsetAsync(state.get() + c0, 0, m * sizeof(dh_subject_track_state), st));
        HIP_TRY(hipMemset2DAsync(&state.get()[c0].subject, sizeof(dh_subject_track_state), 0xFF, sizeof(uint32_t), m, st));
        return DH_OK;
    }
};
static int subject_fit_tracker_create_(const dh_cameras *c, const dh_fit_subjects *set, const dh_fit_model *m, float scale, uint32_t flags,
                                       const dh_fit_track_params *track_params, const dh_ident_params *ident_params,
                                       const dh_subject_track_params *params, const uint8_t *enrolled, dh_subject_fit_tracker **out) {
    const char *who = "dh_subject_fit_tracker_create";
    if (!out) return fail(DH_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    const dh_fit_track_params prm = params_or_default(fit_track_params_default_, track_params);
    const dh_subject_track_params sprm = params_or_default(subject_track_params_default_, params);
    dh_ident_params iprm;
    SubjectsView sv{};
    TRY(fit_tracker_create_check(prm, scale, flags, m, [&]() -> int {
        if (!c) return fail(DH_EINVAL, "%s: NULL camera table", who);
        if (!set) return fail(DH_EINVAL, "%s: NULL subject set", who);
        if (!m) return fail(DH_EINVAL, "%s: NULL model", who);
        return subject_create_check(set, m, scale, ident_params, dh_ident_params_check_, sprm, c->device, "camera table", &iprm, &sv, who);
    }, who));
    const uint64_t pairs = (uint64_t)c->n * sv.n_subjects;
    if (pairs > DH_IDENT_MAX_PAIRS)
        return fail(DH_EINVAL, "%s: %d cameras times %u subjects exceed %u pairs", who, c->n, sv.n_subjects, DH_IDENT_MAX_PAIRS);
    return create_tracker(c, out, [&](dh_subject_fit_tracker &t, size_t n) -> int {
        TRY(t.alloc_cam(prm, n));
        TRY(t.state.alloc(n)); TRY(t.score.alloc((size_t)pairs)); TRY(t.records.alloc(n));
        TRY(t.init_fit(m, scale, flags, prm.rms_max, prm.max_jump, n));
        return t.init_subjects(set, m, iprm, sprm, n, c->device, t.models, enrolled);
    });
}
static int subject_fit_tracker_destroy_(dh_subject_fit_tracker *t) { return destroy_fit_tracker(t); }
static int subject_fit_tracker_reset_(dh_subject_fit_tracker *t, int camera, void *stream) {
    return reset_tracker(t, camera, stream, "dh_subject_fit_tracker_reset");
}
static int subject_fit_tracker_state_(dh_subject_fit_tracker *t, dh_subject_track_state *states) {
    return cam_fit_state(t, states, "dh_subject_fit_tracker_state");
}
static int subject_fit_tracker_info_(const dh_subject_fit_tracker *t, int *n_cams, uint32_t *n_subjects, uint32_t *score_workgroups) {
    return subject_tracker_info(t, t ? t->n : 0, n_cams, n_subjects, score_workgroups, "dh_subject_fit_tracker_info");
}
static int subject_fit_tracker_set_enrolled_(dh_subject_fit_tracker *t, const uint8_t *enrolled, void *stream) {
    return subject_tracker_set_enrolled(t, enrolled, stream, "dh_subject_fit_tracker_set_enrolled");
}
static int subject_fit_tracker_bind_(dh_subject_fit_tracker *t, int camera, uint32_t subject, void *stream) {
    const char *who = "dh_subject_fit_tracker_bind";
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (camera < 0 || camera >= t->n) return fail(DH_EINVAL, "%s: camera %d of %d", who, camera, t->n);
    if (subject >= t->sv.n_subjects && subject != DH_IDENT_UNKNOWN)
        return fail(DH_EINVAL, "%s: subject %u of %u (DH_IDENT_UNKNOWN unbinds)", who, subject, t->sv.n_subjects);
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    dh_subject_track_state *st = t->state.get() + camera;
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&st->subject, (int)subject, 1, (hipStream_t)stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&st->wait, 0, 3, (hipStream_t)stream));      // wait, tries, bound_age
    return DH_OK;
}
// One step of every camera on device arrays and stream s (arguments checked, device selected): five launches, a linear chain.
// (g.a.state and g.a.records stay 0: the state and the records of this tracker travel in g itself.)
static int subject_track_enqueue(dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses,
                                 const dh_support *support, const dh_fit_params &prm, dh_subject_track_record *records, hipStream_t s) {
    SubjectTrackArgs g;
    memset(&g, 0, sizeof g);
    FitSchedArgs f;
    cam_fit_args(t, frames, w, h, present, poses, support, prm, g.a, f);
    IdentArgs &q = g.q;
    q.f.frames = frames; q.f.n = t->n; q.f.w = w; q.f.h = h;
    q.f.cams = t->cams->dev.get(); q.f.inst = t->fit_out.get(); q.f.n_inst = (uint32_t)t->n;
    t->ident_args(q);
    q.fit_rec = t->fit_rec.get(); q.score = t->score.get();
    g.state = t->state.get(); g.records = records;
    g.retry = t->sprm.retry; g.max_tries = t->sprm.max_tries;
    g.want = t->want.get(); g.n_want = t->n_want.get(); g.wants = t->wants.get();
    g.grid = t->grid;
    TRY(hip_step(dh_launch_subject_track_seed(g, s), "k_subject_track_seed"));
    TRY(hip_step(dh_launch_fit_sched(f, s), "k_fit_sched"));
    TRY(hip_step(dh_launch_subject_track_update(g, s), "k_subject_track_update"));
    TRY(hip_step(dh_launch_subject_track_score(g, s), "k_subject_track_score"));
    TRY(hip_step(dh_launch_subject_track_bind(g, s), "k_subject_track_bind"));
    return DH_OK;
}
// The entry points' forwards to the camera pair's forms (section 19's step check, host form and refusals) with this core step.
template <typename... A> static int subject_fit_tracker_step_poses_device_(A... a) { return cam_fit_step_poses_device("dh_subject_fit_tracker_step_poses_device", subject_track_enqueue, a...); }
template <typename... A> static int subject_fit_tracker_step_device_(A... a) { return cam_fit_step_device("dh_subject_fit_tracker_step_device", subject_track_enqueue, a...); }
template <typename... A> static int subject_fit_tracker_step_poses_(A... a) { return cam_fit_step_poses("dh_subject_fit_tracker_step_poses", subject_track_enqueue, a...); }
template <typename... A> static int subject_fit_tracker_step_(A... a) { return cam_fit_step("dh_subject_fit_tracker_step", subject_track_enqueue, a...); }

// ------------------------------------------------------------------ following each rig person with its own subject's model
// The rig fit tracker's core with the subject trackers' parts: the entries' dh_rig_fit_state in `state`, the four words of their
// bindings beside it in `bound`, and the pair scratch of slots * S multi-view scores.
struct dh_rig_subject_fit_tracker : RigFitTrackerBase, SubjectParts {
    Buf<SubjectBinding> bound;           // [slots]
    Buf<dh_view_fit_record> score;       // [slots][S]
    Buf<dh_rig_subject_record> records;  // host forms: [slots]
    // zeros, and DH_IDENT_UNKNOWN (every byte 0xFF) in the subject word of each binding
    int clear(size_t g0, size_t m, hipStream_t st) {
        TRY(RigFitTrackerBase::clear(g0, m, st));
        SubjectBinding *b = bound.get() + g0 * DH_RIG_MAX_TRACKS;
        HIP_TRY(hipMemsetAsync(b, 0, m * DH_RIG_MAX_TRACKS * sizeof(SubjectBinding), st));
        HIP_TRY(hipMemset2DAsync(&b->subject, sizeof(SubjectBinding), 0xFF, sizeof(uint32_t), m * DH_RIG_MAX_TRACKS, st));
        return DH_OK;
    }
};
static int rig_subject_fit_tracker_create_(const dh_rig *rig, const dh_fit_views *views, const dh_fit_subjects *set, const dh_fit_model *m,
                                           float scale, uint32_t flags, const dh_rig_fit_track_params *track_params,
                                           const dh_ident_params *ident_params, const dh_subject_track_params *params,
                                           const uint8_t *enrolled, dh_rig_subject_fit_tracker **out) {
    const char *who = "dh_rig_subject_fit_tracker_create";
    if (!out) return fail(DH_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    const dh_rig_fit_track_params prm = params_or_default(rig_fit_track_params_default_, track_params);
    const dh_subject_track_params sprm = params_or_default(subject_track_params_default_, params);
    dh_ident_params iprm;
    SubjectsView sv{};
    TRY(fit_tracker_create_check(prm, scale, flags, m, [&]() -> int {
        if (!rig) return fail(DH_EINVAL, "%s: NULL rig table", who);
        if (!views) return fail(DH_EINVAL, "%s: NULL view table", who);
        if (!set) return fail(DH_EINVAL, "%s: NULL subject set", who);
        if (!m) return fail(DH_EINVAL, "%s: NULL model", who);
        if (views->cams != rig->cams) return fail(DH_EINVAL, "%s: the rig table and the view table are bound to different camera tables", who);
        return subject_create_check(set, m, scale, ident_params, dh_ident_views_params_check_, sprm, rig->cams->device, "tables", &iprm, &sv, who);
    }, who));
    TRY(rig_terms_check(rig, sv.n, who));
    const size_t ng = (size_t)rig->n_rigs, slots = ng * DH_RIG_MAX_TRACKS;
    const uint64_t pairs = (uint64_t)slots * sv.n_subjects;
    if (pairs > DH_IDENT_MAX_PAIRS)
        return fail(DH_EINVAL, "%s: %d rigs of %d slots times %u subjects exceed %u pairs", who, rig->n_rigs, DH_RIG_MAX_TRACKS, sv.n_subjects,
                    DH_IDENT_MAX_PAIRS);
    return create_tracker(rig->cams, out, [&](dh_rig_subject_fit_tracker &t, size_t n) -> int {
        TRY(t.alloc_rig(rig, views, prm, n));
        TRY(t.bound.alloc(slots)); TRY(t.score.alloc((size_t)pairs)); TRY(t.records.alloc(slots));
        TRY(t.init_fit(m, scale, flags, prm.rms_max, prm.max_jump, slots));
        return t.init_subjects(set, m, iprm, sprm, slots, rig->cams->device, t.models, enrolled);
    }, ng);
}
static int rig_subject_fit_tracker_destroy_(dh_rig_subject_fit_tracker *t) { return destroy_fit_tracker(t); }
static int rig_subject_fit_tracker_reset_(dh_rig_subject_fit_tracker *t, int rig, void *stream) {
    return reset_tracker(t, rig, stream, "dh_rig_subject_fit_tracker_reset", t ? t->rig->n_rigs : 0, "rig");
}
// (the two device arrays of an entry, interleaved)
static int rig_subject_fit_tracker_state_(dh_rig_subject_fit_tracker *t, dh_rig_subject_state *states) {
    if (t && !states) return fail(DH_EINVAL, "dh_rig_subject_fit_tracker_state: NULL argument");
    return read_tracker(t, "dh_rig_subject_fit_tracker_state", [&](size_t) -> int {
        const size_t slots = (size_t)t->rig->n_rigs * DH_RIG_MAX_TRACKS;
        HIP_TRY(hipMemcpy2D(&states->fit, sizeof *states, t->state.get(), sizeof(dh_rig_fit_state), sizeof(dh_rig_fit_state), slots,
                            hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(&states->subject, sizeof *states, t->bound.get(), sizeof(SubjectBinding), sizeof(SubjectBinding), slots,
                            hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int rig_subject_fit_tracker_info_(const dh_rig_subject_fit_tracker *t, int *n_rigs, uint32_t *n_subjects, uint32_t *score_workgroups) {
    return subject_tracker_info(t, t ? t->rig->n_rigs : 0, n_rigs, n_subjects, score_workgroups, "dh_rig_subject_fit_tracker_info");
}
static int rig_subject_fit_tracker_set_enrolled_(dh_rig_subject_fit_tracker *t, const uint8_t *enrolled, void *stream) {
    return subject_tracker_set_enrolled(t, enrolled, stream, "dh_rig_subject_fit_tracker_set_enrolled");
}
static int rig_subject_fit_tracker_bind_(dh_rig_subject_fit_tracker *t, int rig, uint32_t id, uint32_t subject, void *stream) {
    const char *who = "dh_rig_subject_fit_tracker_bind";
    if (!t) return fail(DH_EINVAL, "%s: NULL tracker", who);
    if (rig < 0 || rig >= t->rig->n_rigs) return fail(DH_EINVAL, "%s: rig %d of %d", who, rig, t->rig->n_rigs);
    if (id == 0) return fail(DH_EINVAL, "%s: id 0 names no entry", who);
    if (subject >= t->sv.n_subjects && subject != DH_IDENT_UNKNOWN)
        return fail(DH_EINVAL, "%s: subject %u of %u (DH_IDENT_UNKNOWN unbinds)", who, subject, t->sv.n_subjects);
    DeviceGuard guard(t->cams->device);
    if (!guard.ok) return DH_EHIP;
    return hip_step(dh_launch_rig_subject_set(t->state.get(), t->bound.get(), rig, id, subject, (hipStream_t)stream), "k_rig_subject_set");
}
// One step of every rig on device arrays and stream s (arguments checked, device selected): five launches, a linear chain.
static int rig_subject_enqueue(dh_rig_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                               const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons,
                               const dh_fit_params &prm, dh_rig_subject_record *records, hipStream_t s) {
    RigSubjectArgs g;
    memset(&g, 0, sizeof g);
    FitViewsSchedArgs f;
    rig_fit_args(t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, prm, g.a, f);
    IdentViewsArgs &q = g.q;
    q.f.frames = frames; q.f.n = t->n; q.f.w = w; q.f.h = h;
    q.f.cams = t->cams->dev.get(); q.f.views = t->views->dev.get();
    q.f.inst = t->fit_out.get(); q.f.n_inst = f.f.n_inst;
    t->ident_args(q);
    q.n_sets = 1;
    q.fit_rec = t->fit_rec.get(); q.score = t->score.get();
    g.bound = t->bound.get(); g.records = records;
    g.retry = t->sprm.retry; g.max_tries = t->sprm.max_tries;
    g.want = t->want.get(); g.n_want = t->n_want.get(); g.wants = t->wants.get();
    g.grid = t->grid;
    TRY(hip_step(dh_launch_rig_subject_seed(g, s), "k_rig_subject_seed"));
    TRY(hip_step(dh_launch_fit_views_sched(f, s), "k_fit_views_sched"));
    TRY(hip_step(dh_launch_rig_subject_update(g, s), "k_rig_subject_update"));
    TRY(hip_step(dh_launch_rig_subject_score(g, s), "k_rig_subject_score"));
    TRY(hip_step(dh_launch_rig_subject_bind(g, s), "k_rig_subject_bind"));
    return DH_OK;
}
// The entry points' forwards to the rig pair's forms (section 22's checks, host form and refusals) with this core step.
template <typename... A> static int rig_subject_fit_tracker_step_persons_device_(A... a) { return rig_fit_step_persons_device("dh_rig_subject_fit_tracker_step_persons_device", rig_subject_enqueue, a...); }
template <typename... A> static int rig_subject_fit_tracker_step_device_(A... a) { return rig_fit_step_device("dh_rig_subject_fit_tracker_step_device", rig_subject_enqueue, a...); }
template <typename... A> static int rig_subject_fit_tracker_step_persons_(A... a) { return rig_fit_step_persons("dh_rig_subject_fit_tracker_step_persons", rig_subject_enqueue, a...); }
template <typename... A> static int rig_subject_fit_tracker_step_(A... a) { return rig_fit_step("dh_rig_subject_fit_tracker_step", rig_subject_enqueue, a...); }

// ------------------------------------------------------------------ the C ABI (DH_API: dh_runtime.h)
DH_API(fit_track_params_default, (dh_fit_track_params *p), (p))
DH_API(fit_tracker_angles, (double out[DH_FIT_TRACK_ANGLES][2]), (out))
DH_API(fit_tracker_create, (const dh_cameras *c, const dh_fit_model *m, float scale, uint32_t flags, const dh_fit_track_params *params, dh_fit_tracker **out), (c, m, scale, flags, params, out))
DH_API(fit_tracker_destroy, (dh_fit_tracker *t), (t))
DH_API(fit_tracker_reset, (dh_fit_tracker *t, int camera, void *stream), (t, camera, stream))
DH_API(fit_tracker_state, (dh_fit_tracker *t, dh_fit_track_state *states), (t, states))
DH_API(fit_tracker_step_poses, (dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, dh_fit_track_record *records), (t, frames, w, h, present, poses, support, fit_params, records))
DH_API(fit_tracker_step_poses_device, (dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, dh_fit_track_record *records, void *stream), (t, frames, w, h, present, poses, support, fit_params, records, stream))
DH_API(fit_tracker_step, (dh_predictor *p, dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, dh_fit_track_record *records), (p, t, frames, w, h, present, radius, fit_params, poses_out, support_out, records))
DH_API(fit_tracker_step_device, (dh_predictor *p, dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, dh_fit_track_record *records, void *stream), (p, t, frames, w, h, present, radius, fit_params, poses_out, support_out, records, stream))
DH_API(rig_fit_track_params_default, (dh_rig_fit_track_params *p), (p))
DH_API(rig_fit_tracker_create, (const dh_rig *rig, const dh_fit_views *views, const dh_fit_model *model, float scale, uint32_t flags, const dh_rig_fit_track_params *params, dh_rig_fit_tracker **out), (rig, views, model, scale, flags, params, out))
DH_API(rig_fit_tracker_destroy, (dh_rig_fit_tracker *t), (t))
DH_API(rig_fit_tracker_reset, (dh_rig_fit_tracker *t, int rig, void *stream), (t, rig, stream))
DH_API(rig_fit_tracker_state, (dh_rig_fit_tracker *t, dh_rig_fit_state *states), (t, states))
DH_API(rig_fit_tracker_step_persons, (dh_rig_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_fit_record *records), (t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, fit_params, records))
DH_API(rig_fit_tracker_step_persons_device, (dh_rig_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_fit_record *records, void *stream), (t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, fit_params, records, stream))
DH_API(rig_fit_tracker_step, (dh_predictor *p, dh_rig_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, dh_rig_fit_record *records), (p, t, rt, frames, w, h, present, fit_params, n_heads, heads, rig_ids, n_persons, persons, tracks, records))
DH_API(rig_fit_tracker_step_device, (dh_predictor *p, dh_rig_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, dh_rig_fit_record *records, void *stream), (p, t, rt, frames, w, h, present, fit_params, n_heads, heads, rig_ids, n_persons, persons, tracks, records, stream))
DH_API(subject_track_params_default, (dh_subject_track_params *p), (p))
DH_API(subject_fit_tracker_create, (const dh_cameras *c, const dh_fit_subjects *set, const dh_fit_model *generic, float scale, uint32_t flags, const dh_fit_track_params *track_params, const dh_ident_params *ident_params, const dh_subject_track_params *params, const uint8_t *enrolled, dh_subject_fit_tracker **out), (c, set, generic, scale, flags, track_params, ident_params, params, enrolled, out))
DH_API(subject_fit_tracker_destroy, (dh_subject_fit_tracker *t), (t))
DH_API(subject_fit_tracker_reset, (dh_subject_fit_tracker *t, int camera, void *stream), (t, camera, stream))
DH_API(subject_fit_tracker_state, (dh_subject_fit_tracker *t, dh_subject_track_state *states), (t, states))
DH_API(subject_fit_tracker_info, (const dh_subject_fit_tracker *t, int *n_cams, uint32_t *n_subjects, uint32_t *score_workgroups), (t, n_cams, n_subjects, score_workgroups))
DH_API(subject_fit_tracker_set_enrolled, (dh_subject_fit_tracker *t, const uint8_t *enrolled, void *stream), (t, enrolled, stream))
DH_API(subject_fit_tracker_bind, (dh_subject_fit_tracker *t, int camera, uint32_t subject, void *stream), (t, camera, subject, stream))
DH_API(subject_fit_tracker_step_poses, (dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, dh_subject_track_record *records), (t, frames, w, h, present, poses, support, fit_params, records))
DH_API(subject_fit_tracker_step_poses_device, (dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params, dh_subject_track_record *records, void *stream), (t, frames, w, h, present, poses, support, fit_params, records, stream))
DH_API(subject_fit_tracker_step, (dh_predictor *p, dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, dh_subject_track_record *records), (p, t, frames, w, h, present, radius, fit_params, poses_out, support_out, records))
DH_API(subject_fit_tracker_step_device, (dh_predictor *p, dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, dh_subject_track_record *records, void *stream), (p, t, frames, w, h, present, radius, fit_params, poses_out, support_out, records, stream))
DH_API(rig_subject_fit_tracker_create, (const dh_rig *rig, const dh_fit_views *views, const dh_fit_subjects *set, const dh_fit_model *generic, float scale, uint32_t flags, const dh_rig_fit_track_params *track_params, const dh_ident_params *ident_params, const dh_subject_track_params *params, const uint8_t *enrolled, dh_rig_subject_fit_tracker **out), (rig, views, set, generic, scale, flags, track_params, ident_params, params, enrolled, out))
DH_API(rig_subject_fit_tracker_destroy, (dh_rig_subject_fit_tracker *t), (t))
DH_API(rig_subject_fit_tracker_reset, (dh_rig_subject_fit_tracker *t, int rig, void *stream), (t, rig, stream))
DH_API(rig_subject_fit_tracker_state, (dh_rig_subject_fit_tracker *t, dh_rig_subject_state *states), (t, states))
DH_API(rig_subject_fit_tracker_info, (const dh_rig_subject_fit_tracker *t, int *n_rigs, uint32_t *n_subjects, uint32_t *score_workgroups), (t, n_rigs, n_subjects, score_workgroups))
DH_API(rig_subject_fit_tracker_set_enrolled, (dh_rig_subject_fit_tracker *t, const uint8_t *enrolled, void *stream), (t, enrolled, stream))
DH_API(rig_subject_fit_tracker_bind, (dh_rig_subject_fit_tracker *t, int rig, uint32_t id, uint32_t subject, void *stream), (t, rig, id, subject, stream))
DH_API(rig_subject_fit_tracker_step_persons, (dh_rig_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_subject_record *records), (t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, fit_params, records))
DH_API(rig_subject_fit_tracker_step_persons_device, (dh_rig_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_subject_record *records, void *stream), (t, frames, w, h, present, max_heads, n_heads, heads, n_persons, persons, fit_params, records, stream))
DH_API(rig_subject_fit_tracker_step, (dh_predictor *p, dh_rig_subject_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, dh_rig_subject_record *records), (p, t, rt, frames, w, h, present, fit_params, n_heads, heads, rig_ids, n_persons, persons, tracks, records))
DH_API(rig_subject_fit_tracker_step_device, (dh_predictor *p, dh_rig_subject_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, dh_rig_subject_record *records, void *stream), (p, t, rt, frames, w, h, present, fit_params, n_heads, heads, rig_ids, n_persons, persons, tracks, records, stream))
