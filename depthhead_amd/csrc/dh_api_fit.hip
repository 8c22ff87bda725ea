// dh_api_fit.hip -- the fit family's runtime: models, view tables, bases and subject sets, the fitter and every call it runs (fit,
// multi-view fit, shape, surface, identify, calibration) in its host and _device forms.  Kernels: k_fit.hip, k_fit_views.hip,
// k_fit_shape.hip, k_fit_shape_views.hip, k_calib_views.hip, k_subjects.hip, k_surface.hip, k_ident.hip, k_ident_views.hip.  Shares
// dh_runtime.h with every runtime unit and dh_runtime_fit.h with the fit trackers in dh_api_fit_track.hip.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

#include "dh_runtime.h"
#include "dh_fit.h"
#include "dh_runtime_fit.h"

// ------------------------------------------------------------------ fitting posed models to depth frames
static int fit_model_create_(const float *points, const float *normals, uint32_t n, int device, dh_fit_model **out) {
    if (!out) return fail(DH_EINVAL, "dh_fit_model_create: NULL argument");
    *out = nullptr;
    if (!points || !normals) return fail(DH_EINVAL, "dh_fit_model_create: NULL argument");
    if (n == 0 || n > DH_FIT_MAX_POINTS) return fail(DH_EINVAL, "dh_fit_model_create: %u points, expected 1 .. %u", n, DH_FIT_MAX_POINTS);
    std::unique_ptr<dh_fit_model> m(new dh_fit_model);
    m->device = device; m->n = n;
    double r2 = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        double v2 = 0.0, m2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            const float v = points[(size_t)i * 3 + c], nm = normals[(size_t)i * 3 + c];
            if (!std::isfinite(v)) return fail(DH_EINVAL, "dh_fit_model_create: point %u is not finite", i);
            if (!std::isfinite(nm)) return fail(DH_EINVAL, "dh_fit_model_create: normal %u is not finite", i);
            v2 += (double)v * (double)v; m2 += (double)nm * (double)nm;
        }
        if (!(m2 >= 0.98 && m2 <= 1.02)) return fail(DH_EINVAL, "dh_fit_model_create: normal %u has squared length %g, expected 0.98 .. 1.02", i, m2);
        r2 = std::max(r2, v2);
    }
    m->radius = sqrt(r2);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    TRY(m->pts.alloc((size_t)n * 3));
    TRY(m->nrm.alloc((size_t)n * 3));
    HIP_TRY(hipMemcpy(m->pts.get(), points, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->nrm.get(), normals, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    *out = m.release();
    return DH_OK;
}
static int fit_model_destroy_(dh_fit_model *m) {
    if (!m) return DH_OK;
    DeviceGuard guard(m->device);
    delete m;
    return DH_OK;
}
static int fit_model_info_(const dh_fit_model *m, uint32_t *n, double *radius) {
    if (!m) return fail(DH_EINVAL, "dh_fit_model_info: NULL model");
    if (n) *n = m->n;
    if (radius) *radius = m->radius;
    return DH_OK;
}

// A fitter: the call's tables, the kernels' scratch (both forms of a call use it) and one arena that holds the device copy of a
// host call's arguments, which CallArgs slices anew for every call.  Everything grows on demand and is
// kept between calls.
struct dh_fitter {
    int device = 0;
    Buf<unsigned char> arena;                // host calls: every array the call passes or returns, one 256-byte aligned slice each
    Buf<unsigned long long> shape_sums;      // shape calls: [DH_SHAPE_MAX_SUBJECTS][DH_SHAPE_STRIDE], taken at the first one
    Buf<unsigned long long> calib_sums;      // calibration calls: [cameras][DH_CALIB_STRIDE], taken at the first one of a table size
    Buf<dh_fit_record> ident_score;          // identify calls: one score and one pose (R, t: 12 floats) per (instance, subject) pair
    Buf<float> ident_pose;
    Buf<dh_view_fit_record> ident_vscore;    // multi-view identify calls: one 32-byte score per pair (the poses: ident_pose)
    std::vector<unsigned char> view_cmp;     // a captured multi-view call's tables, to be compared with the staged ones
    CallTables tab;                          // models | instances (last: its stream and events go before any buffer)
};
static int fitter_create_(int device, dh_fitter **out) { return create_owner(device, out, "dh_fitter_create"); }
static int fitter_destroy_(dh_fitter *f) { return destroy_owner(f); }

// The array arguments of one call of the fit family, bound the same way by every *_run and in both forms.  The call declares each
// array once -- in(): one the kernels read, out(): one they write -- naming the field of the kernels' arguments that is to point
// at it; a declaration allocates nothing.  commit() then fills every field: in the _device form with the caller's own pointers,
// and nothing is asked of the runtime (a stream that is being captured stays untouched); in the host form with slices of the
// fitter's arena, each aligned to 256 bytes as an allocation of its own would be; the arena grows at most once, before any slice
// exists, and the inputs follow on the stream in the order they were declared.  A NULL array binds NULL.  finish() ends a host call: the outputs the caller asked for come back in the order they
// were declared and the stream is waited for.
class CallArgs {
    struct Arg {
        void *field;              // the pointer to fill
        const void *src;          // in(): the caller's array
        void *dst, *at;           // out(): the caller's array, and where the output lives on the device when that is not it
        size_t bytes;
    };
    dh_fitter *f_;
    bool dev_;
    hipStream_t s_;
    Arg arg_[12];                 // (the longest call, the multi-view identify, declares nine)
    int n_ = 0;
    static size_t slice(size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; }
  public:
    CallArgs(dh_fitter *f, bool dev, hipStream_t s) : f_(f), dev_(dev), s_(s) {}
    template <typename T>
    void in(const T **field, const T *src, size_t count) { arg_[n_++] = Arg{field, src, nullptr, nullptr, count * sizeof(T)}; }
    // `at`: scratch of the fitter's or the set's that a host call's output is read back from, and a _device call's output goes to
    // when the caller passes NULL
    template <typename T>
    void out(T **field, T *dst, size_t count, T *at = nullptr) { arg_[n_++] = Arg{field, nullptr, dst, at, count * sizeof(T)}; }
    int commit() {
        size_t total = 0;
        for (int i = 0; i < n_ && !dev_; ++i)
            if (!arg_[i].at && (arg_[i].src || arg_[i].dst)) total += slice(arg_[i].bytes);
        if (f_->arena.cap() < total) {
            HIP_TRY(hipDeviceSynchronize());         // (an earlier call may still use the old arena)
            TRY(f_->arena.grow(total));
        }
        unsigned char *next = f_->arena.get();
        for (int i = 0; i < n_; ++i) {
            Arg &a = arg_[i];
            void *p = a.at;
            if (dev_) p = a.src ? const_cast<void *>(a.src) : a.dst ? a.dst : a.at;
            else if (!a.at && (a.src || a.dst)) { p = next; next += slice(a.bytes); }
            memcpy(a.field, &p, sizeof p);           // (every field is a pointer to an object type)
            a.at = p;
            if (!dev_ && a.src && a.bytes) HIP_TRY(hipMemcpyAsync(p, a.src, a.bytes, hipMemcpyHostToDevice, s_));
        }
        return DH_OK;
    }
    int finish() {
        if (dev_) return DH_OK;
        for (int i = 0; i < n_; ++i)
            if (arg_[i].dst && arg_[i].bytes) HIP_TRY(hipMemcpyAsync(arg_[i].dst, arg_[i].at, arg_[i].bytes, hipMemcpyDeviceToHost, s_));
        HIP_TRY(hipStreamSynchronize(s_));
        return DH_OK;
    }
};

// The half of a FitArgs or ShapeArgs that the (checked) frames fill: their count and size, and K or the camera table.
template <typename A>
static void args_frames(A &a, int n, int w, int h, const float *K, const dh_cameras *cams, bool use_cams) {
    a.n = n; a.w = w; a.h = h;
    if (use_cams) a.cams = cams->dev.get();
    else memcpy(a.k, K, sizeof a.k);
}
// What dh_fit_instance_fault found in instance i, as the refusal of a fit or shape call; DH_OK where it found nothing.
static int instance_refusal(const FitInstanceFault &fault, float scale, uint32_t i, double radius, double largest, const char *who) {
    switch (fault.why) {
    case DH_FIT_INST_OK: return DH_OK;
    case DH_FIT_INST_NOT_FINITE: return fail(DH_EINVAL, "%s: instance %u has a non-finite R, t or scale", who, i);
    case DH_FIT_INST_NOT_ORTHONORMAL:
        return fail(DH_EINVAL, "%s: instance %u has an R that is not orthonormal: (R R^T)[%d][%d] = %g", who, i, fault.a, fault.b, fault.g);
    case DH_FIT_INST_EXTENT:
        return fail(DH_EINVAL, "%s: instance %u spans %g mm from its origin (limit %g)", who, i, fabs((double)scale) * radius, DH_FIT_MAX_EXTENT);
    default:
        return fail(DH_EINVAL, "%s: instance %u scales the basis to %g mm (limit %g)", who, i, fabs((double)scale) * largest, DH_SHAPE_MAX_FIELD);
    }
}
// The refusals of instance i (a dh_render_instance, or a dh_view_instance with its world pose) of a fit call that rest on its
// model m, the call's models[model], in the header's order: what dh_fit_instance_fault finds before the extent, then the model's
// own refusals (NULL, another device than the fitter's), then the rest of the fault.
template <typename Instance>
static int instance_model_refusal(const Instance &in, uint32_t i, const dh_fit_model *m, uint32_t model, int device, const char *who) {
    const double radius = m ? m->radius : 0.0;
    const FitInstanceFault fault = dh_fit_instance_fault(in, radius, 0.0);
    if (fault.why != DH_FIT_INST_OK && fault.why < DH_FIT_INST_EXTENT) return instance_refusal(fault, in.scale, i, radius, 0.0, who);
    if (!m) return fail(DH_EINVAL, "%s: model %u is NULL", who, model);
    if (m->device != device) return fail(DH_EINVAL, "%s: model %u lives on device %d, the fitter on %d", who, model, m->device, device);
    return instance_refusal(fault, in.scale, i, radius, 0.0, who);
}
// A fit call's tables, models | instances, as one run of bytes: where the instances begin, and the fill of all
// fit_tables_offset(n_models) + n_inst * sizeof(Instance) bytes at dst -- every byte is written, so two fills of the same call
// compare equal (the capture path of the multi-view fit).
static size_t fit_tables_offset(uint32_t n_models) { return ((size_t)n_models * sizeof(FitModel) + 15) & ~(size_t)15; }
template <typename Instance>
static void fit_tables_fill(unsigned char *dst, const dh_fit_model *const *models, uint32_t n_models, const Instance *inst, uint32_t n_inst,
                            int device) {
    const size_t o_inst = fit_tables_offset(n_models);
    FitModel *mm = (FitModel *)dst;
    for (uint32_t i = 0; i < n_models; ++i)          // (a model no instance names may be NULL: its row is never read)
        mm[i] = models[i] && models[i]->device == device ? FitModel{models[i]->pts.get(), models[i]->nrm.get(), models[i]->n, 0}
                                                         : FitModel{nullptr, nullptr, 0, 0};
    memset(dst + (size_t)n_models * sizeof(FitModel), 0, o_inst - (size_t)n_models * sizeof(FitModel));
    memcpy(dst + o_inst, inst, (size_t)n_inst * sizeof(Instance));
}

// One fit call.  dev: frames / out / records are device pointers and `stream` the caller's; else host pointers.
struct FitReq {
    const uint16_t *frames; int n, w, h;
    const float *K; const dh_cameras *cams; bool use_cams;
    const dh_fit_model *const *models; uint32_t n_models;
    const dh_render_instance *inst; uint32_t n_inst;
    const dh_fit_params *prm;
    dh_render_instance *out; dh_fit_record *rec;
    const dh_render_instance *carried = nullptr;     // (device forms) nullable [n_inst] on the device: the R and t to start from
};
static int fit_run(dh_fitter *f, const FitReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.out || !q.rec) return fail(DH_EINVAL, "%s: NULL output", who);
    TRY(check_frames(q.n, q.w, q.h, q.K, q.cams, q.use_cams, f->device, "fitter", who));
    dh_fit_params prm;
    TRY(fit_params_check(q.prm, &prm, who));
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (q.n_inst && !q.models) return fail(DH_EINVAL, "%s: NULL models", who);
    if (q.n_inst > 0x7fffffffu) return fail(DH_EINVAL, "%s: too many instances", who);
    for (uint32_t i = 0; i < q.n_inst; ++i) {
        const dh_render_instance &in = q.inst[i];
        if (in.frame >= (uint32_t)q.n) return fail(DH_EINVAL, "%s: instance %u names frame %u of %d", who, i, in.frame, q.n);
        if (in.mesh >= q.n_models) return fail(DH_EINVAL, "%s: instance %u names model %u of %u", who, i, in.mesh, q.n_models);
        TRY(instance_model_refusal(in, i, q.models[in.mesh], in.mesh, f->device, who));
    }
    if (q.n_inst == 0) return DH_OK;

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    FitArgs a;
    memset(&a, 0, sizeof a);
    args_frames(a, q.n, q.w, q.h, q.K, q.cams, q.use_cams);
    a.n_inst = q.n_inst;
    fit_args_params(a, prm);
    // ---- the call's tables: one staging buffer, one upload
    const size_t o_inst = fit_tables_offset(q.n_models);
    const size_t bytes = o_inst + (size_t)q.n_inst * sizeof(dh_render_instance);
    TRY(f->tab.reserve(bytes));
    fit_tables_fill(f->tab.stage.get(), q.models, q.n_models, q.inst, q.n_inst, f->device);
    a.models = (const FitModel *)f->tab.dev.get();
    a.inst = (const dh_render_instance *)(f->tab.dev.get() + o_inst);
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n * q.w * q.h);
    args.out(&a.out, q.out, q.n_inst);
    args.out(&a.rec, q.rec, q.n_inst);
    TRY(f->tab.upload(bytes, s));
    TRY(args.commit());
    if (q.carried) TRY(hip_step(dh_launch_fit_carry((dh_render_instance *)(f->tab.dev.get() + o_inst), q.carried, q.n_inst, s), "k_fit_carry"));
    TRY(hip_step(dh_launch_fit(a, s), "k_fit"));
    TRY(f->tab.done(s));
    return args.finish();
}
static int fit_depth_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models,
                      const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records) {
    return fit_run(f, FitReq{frames, n, w, h, K, nullptr, false, models, n_models, instances, n_instances, params, out, records}, false, nullptr, "dh_fit_depth");
}
static int fit_depth_cameras_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models, uint32_t n_models,
                              const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records) {
    return fit_run(f, FitReq{frames, n, w, h, nullptr, c, true, models, n_models, instances, n_instances, params, out, records}, false, nullptr, "dh_fit_depth_cameras");
}
static int fit_depth_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models,
                             const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream) {
    return fit_run(f, FitReq{frames, n, w, h, K, nullptr, false, models, n_models, instances, n_instances, params, out, records}, true, (hipStream_t)stream, "dh_fit_depth_device");
}
static int fit_depth_cameras_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models, uint32_t n_models,
                                     const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream) {
    return fit_run(f, FitReq{frames, n, w, h, nullptr, c, true, models, n_models, instances, n_instances, params, out, records}, true, (hipStream_t)stream, "dh_fit_depth_cameras_device");
}
// The device forms whose instances start from the device output of an earlier fit.
static int fit_depth_carried_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models,
                                     const dh_render_instance *instances, uint32_t n_instances, const dh_render_instance *carried, const dh_fit_params *params,
                                     dh_render_instance *out, dh_fit_record *records, void *stream) {
    const char *who = "dh_fit_depth_carried_device";
    if (n_instances && !carried) return fail(DH_EINVAL, "%s: NULL carried instances", who);
    return fit_run(f, FitReq{frames, n, w, h, K, nullptr, false, models, n_models, instances, n_instances, params, out, records, carried}, true, (hipStream_t)stream, who);
}
static int fit_depth_cameras_carried_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models,
                                             uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_render_instance *carried,
                                             const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream) {
    const char *who = "dh_fit_depth_cameras_carried_device";
    if (n_instances && !carried) return fail(DH_EINVAL, "%s: NULL carried instances", who);
    return fit_run(f, FitReq{frames, n, w, h, nullptr, c, true, models, n_models, instances, n_instances, params, out, records, carried}, true, (hipStream_t)stream, who);
}

// ------------------------------------------------------------------ fitting one model to several views
static int fit_views_create_(const dh_cameras *c, const float *V, const float *u, dh_fit_views **out) {
    if (!out) return fail(DH_EINVAL, "dh_fit_views_create: NULL argument");
    *out = nullptr;
    if (!c || !V || !u) return fail(DH_EINVAL, "dh_fit_views_create: NULL argument");
    std::vector<FitView> host((size_t)c->n);
    for (int i = 0; i < c->n; ++i) {
        FitView &v = host[(size_t)i];
        memcpy(v.V, V + (size_t)i * 9, sizeof v.V);
        memcpy(v.u, u + (size_t)i * 3, sizeof v.u);
        for (int q = 0; q < 9; ++q) if (!std::isfinite(v.V[q])) return fail(DH_EINVAL, "dh_fit_views_create: view %d has a non-finite V or u", i);
        for (int q = 0; q < 3; ++q) if (!std::isfinite(v.u[q])) return fail(DH_EINVAL, "dh_fit_views_create: view %d has a non-finite V or u", i);
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                const double g = ((double)v.V[3 * a] * (double)v.V[3 * b] + (double)v.V[3 * a + 1] * (double)v.V[3 * b + 1]) +
                                 (double)v.V[3 * a + 2] * (double)v.V[3 * b + 2];
                if (!(fabs(g - (a == b ? 1.0 : 0.0)) <= DH_FIT_VIEW_TOLERANCE))
                    return fail(DH_EINVAL, "dh_fit_views_create: view %d has a V that is not orthonormal: (V V^T)[%d][%d] = %g", i, a, b, g);
            }
    }
    std::unique_ptr<dh_fit_views> v(new dh_fit_views);
    v->device = c->device; v->n = c->n; v->cams = c;
    DeviceGuard guard(c->device);
    if (!guard.ok) return DH_EHIP;
    TRY(v->dev.alloc(host.size()));
    HIP_TRY(hipMemcpy(v->dev.get(), host.data(), host.size() * sizeof(FitView), hipMemcpyHostToDevice));
    *out = v.release();
    return DH_OK;
}
static int fit_views_destroy_(dh_fit_views *v) {
    if (!v) return DH_OK;
    DeviceGuard guard(v->device);
    delete v;
    return DH_OK;
}
static int fit_views_info_(const dh_fit_views *v, int *n, int *device) {
    if (!v) return fail(DH_EINVAL, "dh_fit_views_info: NULL view table");
    if (n) *n = v->n;
    if (device) *device = v->device;
    return DH_OK;
}

// The refusals of a multi-view call's view table and of what rests on it: the table, n_sets (NULL: the call takes one set of
// frames and has no such argument) and the frames of its cameras; *n: how many those are.
static int check_views(const dh_fitter *f, const dh_fit_views *views, const uint32_t *n_sets, int w, int h, int *n, const char *who) {
    if (!views) return fail(DH_EINVAL, "%s: NULL view table", who);
    if (views->device != f->device) return fail(DH_EINVAL, "%s: the view table lives on device %d, the fitter on %d", who, views->device, f->device);
    *n = views->n;
    if (n_sets && (*n_sets < 1 || (uint64_t)*n_sets * (uint64_t)*n > 65535))
        return fail(DH_EINVAL, "%s: n_sets = %u of %d cameras, expected 1 .. 65535 frames", who, *n_sets, *n);
    return check_frames(*n, w, h, nullptr, views->cams, true, f->device, "fitter", who);
}

// One multi-view fit call.  dev: frames / out / records are device pointers and `stream` the caller's; else host pointers.
struct FitViewsReq {
    const uint16_t *frames; int w, h;
    const dh_fit_views *views;
    const dh_fit_model *const *models; uint32_t n_models;
    const dh_view_instance *inst; uint32_t n_inst;
    const dh_fit_params *prm;
    dh_view_instance *out; dh_view_fit_record *rec;
};
static int fit_views_run(dh_fitter *f, const FitViewsReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.out || !q.rec) return fail(DH_EINVAL, "%s: NULL output", who);
    int n = 0;
    TRY(check_views(f, q.views, nullptr, q.w, q.h, &n, who));
    dh_fit_params prm;
    TRY(fit_params_check(q.prm, &prm, who));
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (q.n_inst && !q.models) return fail(DH_EINVAL, "%s: NULL models", who);
    if (q.n_inst > 0x7fffffffu) return fail(DH_EINVAL, "%s: too many instances", who);
    for (uint32_t i = 0; i < q.n_inst; ++i) {
        const dh_view_instance &in = q.inst[i];
        if (in.views == 0) return fail(DH_EINVAL, "%s: instance %u is seen by no view", who, i);
        const uint64_t last = (uint64_t)in.first_cam + (63u - (unsigned)__builtin_clzll(in.views));
        if (last >= (uint64_t)n) return fail(DH_EINVAL, "%s: instance %u names camera %llu of %d", who, i, (unsigned long long)last, n);
        if (in.model >= q.n_models) return fail(DH_EINVAL, "%s: instance %u names model %u of %u", who, i, in.model, q.n_models);
        const dh_fit_model *m = q.models[in.model];
        TRY(instance_model_refusal(in, i, m, in.model, f->device, who));
        const uint64_t terms = (uint64_t)__builtin_popcountll(in.views) * m->n;
        if (terms > DH_FIT_MAX_POINTS)
            return fail(DH_EINVAL, "%s: instance %u sums %llu terms (%d views of %u points), above %u", who, i, (unsigned long long)terms,
                        __builtin_popcountll(in.views), m->n, DH_FIT_MAX_POINTS);
    }
    if (q.n_inst == 0) return DH_OK;

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    // A stream that is being captured takes the kernel alone, and nothing else is asked of the runtime while it captures: the
    // tables must be the ones the fitter's last call uploaded (an eager call with the same models and instances), else DH_ESTATE.
    bool capturing = false;
    if (dev) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(s, &cs));
        capturing = cs != hipStreamCaptureStatusNone;
    }
    FitViewsArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.w = q.w; a.h = q.h;
    a.cams = q.views->cams->dev.get();
    a.views = q.views->dev.get();
    a.n_inst = q.n_inst;
    fit_args_params(a, prm);
    // ---- the call's tables: one staging buffer, one upload
    const size_t o_inst = fit_tables_offset(q.n_models);
    const size_t bytes = o_inst + (size_t)q.n_inst * sizeof(dh_view_instance);
    auto fill = [&](unsigned char *dst) { fit_tables_fill(dst, q.models, q.n_models, q.inst, q.n_inst, f->device); };
    if (capturing) {
        f->view_cmp.resize(bytes);                   // (the only path that builds the tables beside the staging buffer)
        fill(f->view_cmp.data());
        if (f->tab.stage.cap() < bytes || memcmp(f->tab.stage.get(), f->view_cmp.data(), bytes) != 0)
            return fail(DH_ESTATE, "%s: the stream is being captured and the fitter's tables are not those of this call (run the call once before the capture)", who);
    } else {
        TRY(f->tab.reserve(bytes));
        fill(f->tab.stage.get());
    }
    a.models = (const FitModel *)f->tab.dev.get();
    a.inst = (const dh_view_instance *)(f->tab.dev.get() + o_inst);
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)n * q.w * q.h);
    args.out(&a.out, q.out, q.n_inst);
    args.out(&a.rec, q.rec, q.n_inst);
    if (!capturing) TRY(f->tab.upload(bytes, s));
    TRY(args.commit());                              // (a capture is of a _device call: its pointers are the caller's)
    TRY(hip_step(dh_launch_fit_views(a, s), "k_fit_views"));
    if (capturing) return DH_OK;
    TRY(f->tab.done(s));
    return args.finish();
}
static int fit_depth_views_(dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views, const dh_fit_model *const *models, uint32_t n_models,
                            const dh_view_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out, dh_view_fit_record *records) {
    return fit_views_run(f, FitViewsReq{frames, w, h, views, models, n_models, instances, n_instances, params, out, records}, false, nullptr, "dh_fit_depth_views");
}
static int fit_depth_views_device_(dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views, const dh_fit_model *const *models, uint32_t n_models,
                                   const dh_view_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out, dh_view_fit_record *records,
                                   void *stream) {
    return fit_views_run(f, FitViewsReq{frames, w, h, views, models, n_models, instances, n_instances, params, out, records}, true, (hipStream_t)stream, "dh_fit_depth_views_device");
}

// ------------------------------------------------------------------ adapting a model's shape to a subject
// A basis: K displacement fields of a model of n points on one device, immutable, one plane per field and axis ([K][3][n]).
struct dh_fit_basis {
    int device = 0;
    uint32_t n = 0, k = 0;
    double largest = 0.0;         // the largest |B_k[i]|
    Buf<float> planes;
};
// (tests/test_abi_fit_shape.py and tests/test_abi_subjects.py hand a zeroed block of 256 bytes where a refusal only needs a basis
// that is not NULL: a basis of 0 points on device 0 whose memory is never touched)
static_assert(sizeof(dh_fit_basis) <= 256, "the ABI tests' stand-in for a basis is 256 zero bytes");
static int fit_basis_create_(const float *fields, uint32_t n, uint32_t n_fields, int device, dh_fit_basis **out) {
    if (!out) return fail(DH_EINVAL, "dh_fit_basis_create: NULL argument");
    *out = nullptr;
    if (!fields) return fail(DH_EINVAL, "dh_fit_basis_create: NULL argument");
    if (n == 0 || n > DH_FIT_MAX_POINTS) return fail(DH_EINVAL, "dh_fit_basis_create: %u points, expected 1 .. %u", n, DH_FIT_MAX_POINTS);
    if (n_fields == 0 || n_fields > DH_SHAPE_MAX_FIELDS)
        return fail(DH_EINVAL, "dh_fit_basis_create: %u fields, expected 1 .. %u", n_fields, DH_SHAPE_MAX_FIELDS);
    if (device < 0) return fail(DH_EINVAL, "dh_fit_basis_create: device %d", device);
    std::unique_ptr<dh_fit_basis> b(new dh_fit_basis);
    b->device = device; b->n = n; b->k = n_fields;
    std::vector<float> planes((size_t)n_fields * 3 * n);
    double l2 = 0.0;
    for (uint32_t k = 0; k < n_fields; ++k)
        for (uint32_t i = 0; i < n; ++i) {
            double v2 = 0.0;
            for (int c = 0; c < 3; ++c) {
                const float v = fields[((size_t)k * n + i) * 3 + c];
                if (!std::isfinite(v)) return fail(DH_EINVAL, "dh_fit_basis_create: field %u has a value at point %u that is not finite", k, i);
                planes[((size_t)k * 3 + c) * n + i] = v;
                v2 += (double)v * (double)v;
            }
            l2 = std::max(l2, v2);
        }
    b->largest = sqrt(l2);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    TRY(b->planes.alloc(planes.size()));
    HIP_TRY(hipMemcpy(b->planes.get(), planes.data(), planes.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = b.release();
    return DH_OK;
}
static int fit_basis_destroy_(dh_fit_basis *b) {
    if (!b) return DH_OK;
    DeviceGuard guard(b->device);
    delete b;
    return DH_OK;
}
static int fit_basis_info_(const dh_fit_basis *b, uint32_t *n, uint32_t *n_fields, double *largest) {
    if (!b) return fail(DH_EINVAL, "dh_fit_basis_info: NULL basis");
    if (n) *n = b->n;
    if (n_fields) *n_fields = b->k;
    if (largest) *largest = b->largest;
    return DH_OK;
}
static int shape_params_default_(dh_shape_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_shape_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->gate = 25.0;
    p->lambda = 1e-3;
    p->min_points = 64;
    return DH_OK;
}

// ---- a shape per subject
// A set: S deformable models of one base mesh on one device.  The models are ordinary dh_fit_models that the set owns; their
// radius is the set's bound.
struct dh_fit_subjects {
    int device = 0;
    uint32_t n = 0, n_tris = 0, n_subjects = 0;
    double max_coeff = 0.0, radius = 0.0;    // radius: the bound on |v'| (dh_subjects_radius_bound)
    const dh_fit_basis *basis = nullptr;     // borrowed: it outlives the set
    Buf<float> base;
    Buf<uint32_t> tris, corner_begin, corners;
    Buf<dh_subject_state> state;
    Buf<SubjectModel> table;                 // [S] the models' pointers
    Buf<dh_shape_record> rec;                // the host update's records
    std::vector<std::unique_ptr<dh_fit_model>> models;
    // a surface set: everything below is allocated at creation, nothing later
    bool surface = false;
    double max_offset = 0.0;
    Buf<float> nb;                           // [n][3] the base normals
    Buf<uint32_t> nbr_begin, nbr;            // each vertex's neighbour list
    Buf<double> offsets;                     // [S][n]
    Buf<unsigned long long> rows, tally;     // the step's sums: [S][n][DH_SURFACE_ROW] and [S][DH_SURFACE_TALLY]
    Buf<double> scratch;                     // [S][2][n]
    Buf<dh_surface_record> srec;             // [S] the host step's records
    hipStream_t s = nullptr;                 // the host calls' stream
    ~dh_fit_subjects() { if (s) (void)hipStreamDestroy(s); }
};
static SubjectsArgs subjects_args(const dh_fit_subjects *set, const dh_shape_record *rec, uint32_t first, uint32_t count) {
    SubjectsArgs a;
    memset(&a, 0, sizeof a);
    a.base = set->base.get(); a.basis = set->basis->planes.get();
    a.tris = set->tris.get(); a.corner_begin = set->corner_begin.get(); a.corners = set->corners.get();
    a.models = set->table.get(); a.state = set->state.get(); a.rec = rec;
    a.n = set->n; a.nk = set->basis->k;
    a.first = first; a.count = count;
    a.max_coeff = set->max_coeff;
    return a;
}
// One evaluation of subjects first .. first + count - 1 (apply where rec is given, points, normals): a surface set's points
// carry its offsets.
static hipError_t subjects_evaluate(const dh_fit_subjects *set, const dh_shape_record *rec, uint32_t first, uint32_t count, hipStream_t s) {
    const SubjectsArgs a = subjects_args(set, rec, first, count);
    if (!set->surface) return dh_launch_subjects_update(a, s);
    return dh_launch_subjects_update_surface(SurfacePointsArgs{a, set->nb.get(), set->offsets.get()}, true, s);
}
static int subjects_create(const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis, uint32_t n_subjects,
                           double max_coeff, bool surface, double max_offset, int device, dh_fit_subjects **out, const char *who) {
    if (!out) return fail(DH_EINVAL, "%s: NULL argument", who);
    *out = nullptr;
    if (!verts || !tris || !basis) return fail(DH_EINVAL, "%s: NULL argument", who);
    if (n == 0 || n > DH_FIT_MAX_POINTS) return fail(DH_EINVAL, "%s: %u points, expected 1 .. %u", who, n, DH_FIT_MAX_POINTS);
    if (n_tris == 0 || n_tris > DH_SUBJECTS_MAX_TRIS) return fail(DH_EINVAL, "%s: %u triangles, expected 1 .. %u", who, n_tris, DH_SUBJECTS_MAX_TRIS);
    if (n_subjects < 1 || n_subjects > DH_SHAPE_MAX_SUBJECTS)
        return fail(DH_EINVAL, "%s: n_subjects = %u, expected 1 .. %u", who, n_subjects, DH_SHAPE_MAX_SUBJECTS);
    if (!(max_coeff > 0.0) || !std::isfinite(max_coeff)) return fail(DH_EINVAL, "%s: max_coeff %g, expected a finite value > 0", who, max_coeff);
    if (device < 0) return fail(DH_EINVAL, "%s: device %d", who, device);
    double r2 = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
        double v2 = 0.0;
        for (int c = 0; c < 3; ++c) {
            const float v = verts[(size_t)i * 3 + c];
            if (!std::isfinite(v)) return fail(DH_EINVAL, "%s: vertex %u is not finite", who, i);
            v2 += (double)v * (double)v;
        }
        r2 = std::max(r2, v2);
    }
    std::vector<uint32_t> begin((size_t)n + 1), corners((size_t)n_tris * 3);
    uint32_t bad = 0;
    if (!dh_subjects_corner_lists(tris, n_tris, n, begin.data(), corners.data(), &bad))
        return fail(DH_EINVAL, "%s: triangle %u names a vertex that is not below %u", who, bad, n);
    const uint32_t flat = dh_subjects_first_zero_normal(verts, tris, begin.data(), corners.data(), n);
    if (flat < n) return fail(DH_EINVAL, "%s: vertex %u of the base mesh has a zero normal", who, flat);
    if (basis->n != n) return fail(DH_EINVAL, "%s: the basis is one of %u points, the mesh has %u", who, basis->n, n);
    if (basis->device != device) return fail(DH_EINVAL, "%s: the basis lives on device %d, the set on %d", who, basis->device, device);
    std::vector<uint32_t> nbr_begin, nbr;
    if (surface) {
        if (!(max_offset > 0.0 && max_offset <= DH_SURFACE_MAX_OFFSET))
            return fail(DH_EINVAL, "%s: max_offset %g outside (0, %g]", who, max_offset, DH_SURFACE_MAX_OFFSET);
        if ((uint64_t)n_subjects * n > DH_SURFACE_MAX_CELLS)
            return fail(DH_EINVAL, "%s: %u subjects of %u vertices exceed %u cells", who, n_subjects, n, DH_SURFACE_MAX_CELLS);
        std::vector<uint32_t> work((size_t)n_tris * 6);
        nbr_begin.resize((size_t)n + 1); nbr.resize((size_t)n_tris * 6);
        (void)dh_subjects_neighbour_lists(tris, n_tris, n, nbr_begin.data(), nbr.data(), work.data(), nullptr);   // (the indices were checked above)
        nbr.resize(std::max<size_t>(nbr_begin[n], 1));
    }

    std::unique_ptr<dh_fit_subjects> set(new dh_fit_subjects);
    set->device = device; set->n = n; set->n_tris = n_tris; set->n_subjects = n_subjects;
    set->max_coeff = max_coeff; set->basis = basis;
    set->surface = surface; set->max_offset = surface ? max_offset : 0.0;
    set->radius = surface ? dh_surface_radius_bound(sqrt(r2), basis->k, max_coeff, basis->largest, max_offset)
                          : dh_subjects_radius_bound(sqrt(r2), basis->k, max_coeff, basis->largest);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    TRY(set->base.alloc((size_t)n * 3));
    TRY(set->tris.alloc((size_t)n_tris * 3));
    TRY(set->corner_begin.alloc(begin.size()));
    TRY(set->corners.alloc(corners.size()));
    TRY(set->state.alloc(n_subjects));
    TRY(set->table.alloc(n_subjects));
    TRY(set->rec.alloc(n_subjects));
    std::vector<SubjectModel> table(n_subjects);
    for (uint32_t sj = 0; sj < n_subjects; ++sj) {
        std::unique_ptr<dh_fit_model> m(new dh_fit_model);
        m->device = device; m->n = n; m->radius = set->radius;
        TRY(m->pts.alloc((size_t)n * 3));
        TRY(m->nrm.alloc((size_t)n * 3));
        table[sj] = SubjectModel{m->pts.get(), m->nrm.get()};
        set->models.push_back(std::move(m));
    }
    TRY(hip_step(hipStreamCreateWithFlags(&set->s, hipStreamNonBlocking), "hipStreamCreate"));
    HIP_TRY(hipMemcpy(set->base.get(), verts, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->tris.get(), tris, (size_t)n_tris * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->corner_begin.get(), begin.data(), begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->corners.get(), corners.data(), corners.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->table.get(), table.data(), table.size() * sizeof(SubjectModel), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(set->state.get(), 0, (size_t)n_subjects * sizeof(dh_subject_state)));
    if (surface) {
        const size_t cells = (size_t)n_subjects * n;
        TRY(set->nb.alloc((size_t)n * 3));
        TRY(set->nbr_begin.alloc(nbr_begin.size()));
        TRY(set->nbr.alloc(nbr.size()));
        TRY(set->offsets.alloc(cells));
        TRY(set->rows.alloc(cells * DH_SURFACE_ROW));
        TRY(set->tally.alloc((size_t)n_subjects * DH_SURFACE_TALLY));
        TRY(set->scratch.alloc(cells * 2));
        TRY(set->srec.alloc(n_subjects));
        TRY(hip_step(dh_surface_solve_prepare(n), "k_surface_solve: dynamic LDS"));
        HIP_TRY(hipMemcpy(set->nbr_begin.get(), nbr_begin.data(), nbr_begin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(set->nbr.get(), nbr.data(), nbr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(set->offsets.get(), 0, cells * sizeof(double)));
        HIP_TRY(hipMemset(set->rows.get(), 0, cells * DH_SURFACE_ROW * sizeof(unsigned long long)));
        HIP_TRY(hipMemset(set->tally.get(), 0, (size_t)n_subjects * DH_SURFACE_TALLY * sizeof(unsigned long long)));
        HIP_TRY(hipDeviceSynchronize());
        // the base normals: section 25's normals of subject 0's model at its zero coefficients, which is the base mesh
        TRY(hip_step(dh_launch_subjects_update(subjects_args(set.get(), nullptr, 0, 1), set->s), "k_subjects"));
        HIP_TRY(hipMemcpyAsync(set->nb.get(), table[0].nrm, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, set->s));
    }
    // every model evaluated at its zero coefficients (and zero offsets)
    TRY(hip_step(subjects_evaluate(set.get(), nullptr, 0, n_subjects, set->s), "k_subjects"));
    HIP_TRY(hipStreamSynchronize(set->s));
    *out = set.release();
    return DH_OK;
}
static int fit_subjects_create_(const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis, uint32_t n_subjects,
                                double max_coeff, int device, dh_fit_subjects **out) {
    return subjects_create(verts, n, tris, n_tris, basis, n_subjects, max_coeff, false, 0.0, device, out, "dh_fit_subjects_create");
}
static int fit_subjects_create_surface_(const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis, uint32_t n_subjects,
                                        double max_coeff, double max_offset, int device, dh_fit_subjects **out) {
    return subjects_create(verts, n, tris, n_tris, basis, n_subjects, max_coeff, true, max_offset, device, out, "dh_fit_subjects_create_surface");
}
// The offsets of one subject of a surface set.
static int fit_subjects_set_offsets_(dh_fit_subjects *s, uint32_t subject, const double *offsets) {
    const char *who = "dh_fit_subjects_set_offsets";
    if (!s) return fail(DH_EINVAL, "%s: NULL subject set", who);
    if (!offsets) return fail(DH_EINVAL, "%s: NULL offsets", who);
    if (!s->surface) return fail(DH_EINVAL, "%s: the set holds no offsets (dh_fit_subjects_create_surface makes one that does)", who);
    if (subject >= s->n_subjects) return fail(DH_EINVAL, "%s: subject %u of %u", who, subject, s->n_subjects);
    for (uint32_t i = 0; i < s->n; ++i)
        if (!(fabs(offsets[i]) <= s->max_offset)) return fail(DH_EINVAL, "%s: offset %u is %g, outside +-%g", who, i, offsets[i], s->max_offset);
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipMemcpyAsync(s->offsets.get() + (size_t)subject * s->n, offsets, (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, s->s));
    TRY(hip_step(subjects_evaluate(s, nullptr, subject, 1, s->s), "k_subjects"));
    HIP_TRY(hipStreamSynchronize(s->s));
    return DH_OK;
}
static int fit_subjects_read_offsets_(dh_fit_subjects *s, uint32_t subject, double *offsets, uint32_t *counts) {
    const char *who = "dh_fit_subjects_read_offsets";
    if (!s) return fail(DH_EINVAL, "%s: NULL subject set", who);
    if (!s->surface) return fail(DH_EINVAL, "%s: the set holds no offsets (dh_fit_subjects_create_surface makes one that does)", who);
    if (subject >= s->n_subjects) return fail(DH_EINVAL, "%s: subject %u of %u", who, subject, s->n_subjects);
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    std::vector<unsigned long long> rows(counts ? (size_t)s->n * DH_SURFACE_ROW : 0);
    if (offsets) HIP_TRY(hipMemcpyAsync(offsets, s->offsets.get() + (size_t)subject * s->n, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost, s->s));
    if (counts) HIP_TRY(hipMemcpyAsync(rows.data(), s->rows.get() + (size_t)subject * s->n * DH_SURFACE_ROW, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->s));
    HIP_TRY(hipStreamSynchronize(s->s));
    if (counts)
        for (uint32_t i = 0; i < s->n; ++i) counts[i] = (uint32_t)std::min<unsigned long long>(rows[(size_t)i * DH_SURFACE_ROW + DH_SURFACE_CNT], 0xffffffffull);
    return DH_OK;
}
static int fit_subjects_destroy_(dh_fit_subjects *s) {
    if (!s) return DH_OK;
    DeviceGuard guard(s->device);
    delete s;
    return DH_OK;
}
static int fit_subjects_info_(const dh_fit_subjects *s, uint32_t *n, uint32_t *n_tris, uint32_t *n_fields, uint32_t *n_subjects, double *radius, int *device) {
    if (!s) return fail(DH_EINVAL, "dh_fit_subjects_info: NULL subject set");
    if (n) *n = s->n;
    if (n_tris) *n_tris = s->n_tris;
    if (n_fields) *n_fields = s->basis->k;
    if (n_subjects) *n_subjects = s->n_subjects;
    if (radius) *radius = s->radius;
    if (device) *device = s->device;
    return DH_OK;
}
static int fit_subjects_model_(const dh_fit_subjects *s, uint32_t subject, const dh_fit_model **model) {
    if (!s || !model) return fail(DH_EINVAL, "dh_fit_subjects_model: NULL argument");
    if (subject >= s->n_subjects) return fail(DH_EINVAL, "dh_fit_subjects_model: subject %u of %u", subject, s->n_subjects);
    *model = s->models[subject].get();
    return DH_OK;
}
static int fit_subjects_set_coeffs_(dh_fit_subjects *s, uint32_t first, uint32_t count, const double *coeffs) {
    const char *who = "dh_fit_subjects_set_coeffs";
    if (!s) return fail(DH_EINVAL, "%s: NULL subject set", who);
    if (!coeffs) return fail(DH_EINVAL, "%s: NULL coefficients", who);
    if ((uint64_t)first + count > s->n_subjects) return fail(DH_EINVAL, "%s: subjects %u .. %llu of %u", who, first, (unsigned long long)first + count, s->n_subjects);
    const uint32_t nk = s->basis->k;
    for (uint32_t i = 0; i < count; ++i)
        for (uint32_t k = 0; k < nk; ++k) {
            const double c = coeffs[(size_t)i * 8 + k];
            if (!(fabs(c) <= s->max_coeff)) return fail(DH_EINVAL, "%s: coefficient %u of subject %u is %g, outside +-%g", who, k, first + i, c, s->max_coeff);
        }
    if (count == 0) return DH_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    std::vector<dh_subject_state> st(count);
    HIP_TRY(hipMemcpyAsync(st.data(), s->state.get() + first, (size_t)count * sizeof(dh_subject_state), hipMemcpyDeviceToHost, s->s));
    HIP_TRY(hipStreamSynchronize(s->s));
    for (uint32_t i = 0; i < count; ++i) {
        for (uint32_t k = 0; k < 8; ++k) st[i].coeffs[k] = k < nk ? coeffs[(size_t)i * 8 + k] : 0.0;
        st[i].flags = 0;
    }
    HIP_TRY(hipMemcpyAsync(s->state.get() + first, st.data(), (size_t)count * sizeof(dh_subject_state), hipMemcpyHostToDevice, s->s));
    TRY(hip_step(subjects_evaluate(s, nullptr, first, count, s->s), "k_subjects"));
    HIP_TRY(hipStreamSynchronize(s->s));
    return DH_OK;
}
static int fit_subjects_state_(dh_fit_subjects *s, dh_subject_state *state) {
    if (!s) return fail(DH_EINVAL, "dh_fit_subjects_state: NULL subject set");
    if (!state) return fail(DH_EINVAL, "dh_fit_subjects_state: NULL state");
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipMemcpyAsync(state, s->state.get(), (size_t)s->n_subjects * sizeof(dh_subject_state), hipMemcpyDeviceToHost, s->s));
    HIP_TRY(hipStreamSynchronize(s->s));
    return DH_OK;
}
static int fit_subjects_read_(dh_fit_subjects *s, uint32_t subject, float *points, float *normals) {
    if (!s) return fail(DH_EINVAL, "dh_fit_subjects_read: NULL subject set");
    if (subject >= s->n_subjects) return fail(DH_EINVAL, "dh_fit_subjects_read: subject %u of %u", subject, s->n_subjects);
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    const dh_fit_model *m = s->models[subject].get();
    const size_t bytes = (size_t)s->n * 3 * sizeof(float);
    if (points) HIP_TRY(hipMemcpyAsync(points, m->pts.get(), bytes, hipMemcpyDeviceToHost, s->s));
    if (normals) HIP_TRY(hipMemcpyAsync(normals, m->nrm.get(), bytes, hipMemcpyDeviceToHost, s->s));
    HIP_TRY(hipStreamSynchronize(s->s));
    return DH_OK;
}
static int fit_subjects_update_(dh_fit_subjects *s, const dh_shape_record *records) {
    if (!s) return fail(DH_EINVAL, "dh_fit_subjects_update: NULL subject set");
    if (!records) return fail(DH_EINVAL, "dh_fit_subjects_update: NULL records");
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipMemcpyAsync(s->rec.get(), records, (size_t)s->n_subjects * sizeof(dh_shape_record), hipMemcpyHostToDevice, s->s));
    TRY(hip_step(subjects_evaluate(s, s->rec.get(), 0, s->n_subjects, s->s), "k_subjects"));
    HIP_TRY(hipStreamSynchronize(s->s));
    return DH_OK;
}
static int fit_subjects_update_device_(dh_fit_subjects *s, const dh_shape_record *records, void *stream) {
    if (!s) return fail(DH_EINVAL, "dh_fit_subjects_update_device: NULL subject set");
    if (!records) return fail(DH_EINVAL, "dh_fit_subjects_update_device: NULL records");
    DeviceGuard guard(s->device);
    if (!guard.ok) return DH_EHIP;
    return hip_step(subjects_evaluate(s, records, 0, s->n_subjects, (hipStream_t)stream), "k_subjects");
}

// The refusals every shape call (single-view or multi-view) begins with, around those of its frames: the pointers, then the
// subject count, the params (NULL: the defaults; *out is what the call runs with), the model and the basis, the instances.
static int shape_check_pointers(const dh_fitter *f, const void *frames, const void *rec, const dh_fit_model *m, const dh_fit_basis *b, const char *who) {
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!rec) return fail(DH_EINVAL, "%s: NULL records", who);
    if (!m) return fail(DH_EINVAL, "%s: NULL model", who);
    if (!b) return fail(DH_EINVAL, "%s: NULL basis", who);
    return DH_OK;
}
static int shape_check_call(const dh_fitter *f, const dh_fit_model *m, const dh_fit_basis *b, uint32_t n_subjects, const dh_shape_params *in,
                            dh_shape_params *out, const void *inst, uint32_t n_inst, const char *who) {
    if (n_subjects < 1 || n_subjects > DH_SHAPE_MAX_SUBJECTS)
        return fail(DH_EINVAL, "%s: n_subjects = %u, expected 1 .. %u", who, n_subjects, DH_SHAPE_MAX_SUBJECTS);
    dh_shape_params prm;
    (void)shape_params_default_(&prm);
    if (in) prm = *in;
    if (!(prm.gate > 0.0 && prm.gate <= DH_SHAPE_MAX_GATE)) return fail(DH_EINVAL, "%s: gate = %g outside (0, %g]", who, prm.gate, DH_SHAPE_MAX_GATE);
    if (!(prm.lambda >= 0.0) || !std::isfinite(prm.lambda)) return fail(DH_EINVAL, "%s: lambda %g, expected a finite value >= 0", who, prm.lambda);
    if (prm.min_points < 1) return fail(DH_EINVAL, "%s: min_points 0 below 1", who);
    if (prm.reserved0 || prm.reserved[0] || prm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    if (m->device != f->device) return fail(DH_EINVAL, "%s: the model lives on device %d, the fitter on %d", who, m->device, f->device);
    if (b->device != f->device) return fail(DH_EINVAL, "%s: the basis lives on device %d, the fitter on %d", who, b->device, f->device);
    if (b->n != m->n) return fail(DH_EINVAL, "%s: the basis is one of %u points, the model has %u", who, b->n, m->n);
    if (n_inst && !inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (n_inst > DH_SHAPE_MAX_TERMS) return fail(DH_EINVAL, "%s: too many instances", who);
    *out = prm;
    return DH_OK;
}
// The half of a ShapeArgs that the model, the basis, the subjects and the (checked) params fill.
static void shape_args_common(ShapeArgs &a, dh_fitter *f, const dh_fit_model *m, const dh_fit_basis *b, uint32_t n_inst, uint32_t n_subjects,
                              const dh_shape_params &prm) {
    a.pts = m->pts.get(); a.nrm = m->nrm.get(); a.basis = b->planes.get();
    a.np = m->n; a.nk = b->k;
    a.radius = m->radius; a.largest = b->largest;
    a.n_inst = n_inst; a.n_subjects = n_subjects;
    a.min_points = prm.min_points;
    a.gate = prm.gate;
    a.lam1 = 1.0 + prm.lambda;
    a.sums = f->shape_sums.get();
}
// The refusals of a single-view shape or surface step that rest on its instances.  The _device form knows their number alone; the
// host form goes through those that take part, in the header's order, and counts each subject's terms.  max_scale > 0: the
// surface step's bound on |scale|.
static int shape_check_terms(bool dev, const dh_render_instance *inst, uint32_t n_inst, const uint32_t *subjects, uint32_t n_subjects,
                             const dh_fit_record *fit_rec, int n, uint32_t np, double radius, double largest, double max_scale, const char *who) {
    if (dev) {
        if ((uint64_t)n_inst * np > DH_SHAPE_MAX_TERMS)
            return fail(DH_EINVAL, "%s: %u instances of %u points exceed %u terms", who, n_inst, np, DH_SHAPE_MAX_TERMS);
        return DH_OK;
    }
    std::vector<uint32_t> per(n_subjects, 0);
    for (uint32_t i = 0; i < n_inst; ++i) {
        const uint32_t sj = subjects ? subjects[i] : 0u;
        if (sj == DH_SHAPE_SKIP) continue;
        if (fit_rec && fit_rec[i].status != DH_FIT_OK) continue;
        if (sj >= n_subjects) return fail(DH_EINVAL, "%s: instance %u names subject %u of %u", who, i, sj, n_subjects);
        const dh_render_instance &in = inst[i];
        if (in.frame >= (uint32_t)n) return fail(DH_EINVAL, "%s: instance %u names frame %u of %d", who, i, in.frame, n);
        TRY(instance_refusal(dh_fit_instance_fault(in, radius, largest), in.scale, i, radius, largest, who));
        if (max_scale > 0.0 && !(fabs((double)in.scale) <= max_scale))
            return fail(DH_EINVAL, "%s: instance %u has |scale| = %g above %g", who, i, fabs((double)in.scale), max_scale);
        if ((uint64_t)(++per[sj]) * np > DH_SHAPE_MAX_TERMS)
            return fail(DH_EINVAL, "%s: subject %u has more than %u terms (instances times %u points)", who, sj, DH_SHAPE_MAX_TERMS, np);
    }
    return DH_OK;
}

// The refusals of the subject set of a surface or identify call (the shape step over a set has its own: it names n_subjects = 0
// with the plain step's words, after the params): the set's device, that it holds offsets where the call needs them, n_subjects.
static int check_subjects(const dh_fitter *f, const dh_fit_subjects *set, uint32_t n_subjects, bool surface, const char *who) {
    if (set->device != f->device) return fail(DH_EINVAL, "%s: the subject set lives on device %d, the fitter on %d", who, set->device, f->device);
    if (surface && !set->surface) return fail(DH_EINVAL, "%s: the set holds no offsets (dh_fit_subjects_create_surface makes one that does)", who);
    if (n_subjects < 1 || n_subjects > set->n_subjects)
        return fail(DH_EINVAL, "%s: n_subjects = %u, expected 1 .. %u, the set's", who, n_subjects, set->n_subjects);
    return DH_OK;
}

// One shape call.  dev: frames / instances / subjects / records are device pointers and `stream` the caller's; else host pointers.
struct ShapeReq {
    const uint16_t *frames; int n, w, h;
    const float *K; const dh_cameras *cams; bool use_cams;
    const dh_fit_model *model; const dh_fit_basis *basis;
    const dh_render_instance *inst; uint32_t n_inst;
    const uint32_t *subjects; uint32_t n_subjects;
    const dh_shape_params *prm;
    dh_shape_record *rec;
    // the step over a subject set: `set` in place of model and basis, and the instances' fit records
    bool use_set = false;
    const dh_fit_subjects *set = nullptr;
    const dh_fit_record *fit_rec = nullptr;
};
static int shape_run(dh_fitter *f, const ShapeReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (q.use_set && f && q.frames && q.rec && !q.set) return fail(DH_EINVAL, "%s: NULL subject set", who);
    // (a set's models all have the set's bound for their radius: the first stands for them in the checks)
    const dh_fit_model *m = q.use_set ? (q.set ? q.set->models[0].get() : nullptr) : q.model;
    const dh_fit_basis *b = q.use_set ? (q.set ? q.set->basis : nullptr) : q.basis;
    TRY(shape_check_pointers(f, q.frames, q.rec, m, b, who));
    TRY(check_frames(q.n, q.w, q.h, q.K, q.cams, q.use_cams, f->device, "fitter", who));
    if (q.use_set && q.set->device != f->device)
        return fail(DH_EINVAL, "%s: the subject set lives on device %d, the fitter on %d", who, q.set->device, f->device);
    if (q.use_set && q.n_subjects > q.set->n_subjects)
        return fail(DH_EINVAL, "%s: n_subjects = %u, expected 1 .. %u, the set's", who, q.n_subjects, q.set->n_subjects);
    dh_shape_params prm;
    TRY(shape_check_call(f, m, b, q.n_subjects, q.prm, &prm, q.inst, q.n_inst, who));
    TRY(shape_check_terms(dev, q.inst, q.n_inst, q.subjects, q.n_subjects, q.fit_rec, q.n, m->n, m->radius, b->largest, 0.0, who));

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    if (!f->shape_sums) TRY(f->shape_sums.alloc((size_t)DH_SHAPE_MAX_SUBJECTS * DH_SHAPE_STRIDE));
    ShapeArgs a;
    memset(&a, 0, sizeof a);
    args_frames(a, q.n, q.w, q.h, q.K, q.cams, q.use_cams);
    shape_args_common(a, f, m, b, q.n_inst, q.n_subjects, prm);
    const dh_fit_record *fit_rec = nullptr;
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n * q.w * q.h);
    args.in(&a.inst, q.inst, q.n_inst);
    args.in(&a.subjects, q.subjects, q.n_inst);
    args.in(&fit_rec, q.fit_rec, q.n_inst);
    args.out(&a.rec, q.rec, q.n_subjects);
    TRY(args.commit());
    // ---- the three stream-ordered operations
    TRY(hip_step(dh_launch_shape_clear(a, s), "k_shape_clear"));
    if (q.use_set) TRY(hip_step(dh_launch_shape_accumulate_subjects(ShapeSubjectsArgs{a, q.set->table.get(), fit_rec}, s), "k_shape_accumulate_subjects"));
    else TRY(hip_step(dh_launch_shape_accumulate(a, s), "k_shape_accumulate"));
    TRY(hip_step(dh_launch_shape_solve(a, s), "k_shape_solve"));
    return args.finish();
}
static int fit_shape_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model, const dh_fit_basis *basis,
                      const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params,
                      dh_shape_record *records) {
    return shape_run(f, ShapeReq{frames, n, w, h, K, nullptr, false, model, basis, instances, n_instances, subjects, n_subjects, params, records}, false, nullptr, "dh_fit_shape");
}
static int fit_shape_cameras_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *model, const dh_fit_basis *basis,
                              const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params,
                              dh_shape_record *records) {
    return shape_run(f, ShapeReq{frames, n, w, h, nullptr, c, true, model, basis, instances, n_instances, subjects, n_subjects, params, records}, false, nullptr, "dh_fit_shape_cameras");
}
static int fit_shape_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model, const dh_fit_basis *basis,
                             const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params,
                             dh_shape_record *records, void *stream) {
    return shape_run(f, ShapeReq{frames, n, w, h, K, nullptr, false, model, basis, instances, n_instances, subjects, n_subjects, params, records}, true, (hipStream_t)stream, "dh_fit_shape_device");
}
static int fit_shape_cameras_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *model, const dh_fit_basis *basis,
                                     const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params,
                                     dh_shape_record *records, void *stream) {
    return shape_run(f, ShapeReq{frames, n, w, h, nullptr, c, true, model, basis, instances, n_instances, subjects, n_subjects, params, records}, true, (hipStream_t)stream, "dh_fit_shape_cameras_device");
}

// The same step over a subject set.
static ShapeReq shape_subjects_req(const uint16_t *frames, int n, int w, int h, const float *K, const dh_cameras *c, bool use_cams, const dh_fit_subjects *set,
                                   const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                   const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records) {
    return ShapeReq{frames, n, w, h, K, c, use_cams, nullptr, nullptr, instances, n_instances, subjects, n_subjects, params, records, true, set, fit_records};
}
static int fit_shape_subjects_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                               const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                               const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records) {
    return shape_run(f, shape_subjects_req(frames, n, w, h, K, nullptr, false, set, instances, n_instances, subjects, n_subjects, fit_records, params, records),
                     false, nullptr, "dh_fit_shape_subjects");
}
static int fit_shape_subjects_cameras_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set,
                                       const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                       const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records) {
    return shape_run(f, shape_subjects_req(frames, n, w, h, nullptr, c, true, set, instances, n_instances, subjects, n_subjects, fit_records, params, records),
                     false, nullptr, "dh_fit_shape_subjects_cameras");
}
static int fit_shape_subjects_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                                      const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                      const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records, void *stream) {
    return shape_run(f, shape_subjects_req(frames, n, w, h, K, nullptr, false, set, instances, n_instances, subjects, n_subjects, fit_records, params, records),
                     true, (hipStream_t)stream, "dh_fit_shape_subjects_device");
}
static int fit_shape_subjects_cameras_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set,
                                              const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                              const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records, void *stream) {
    return shape_run(f, shape_subjects_req(frames, n, w, h, nullptr, c, true, set, instances, n_instances, subjects, n_subjects, fit_records, params, records),
                     true, (hipStream_t)stream, "dh_fit_shape_subjects_cameras_device");
}

// ---- the surface step over a surface set
static int fit_surface_params_default_(dh_surface_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_fit_surface_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->gate = 25.0; p->min_cos2 = 0.25; p->mu = 0.5; p->eps = 0.05;
    p->min_count = 2; p->min_points = 64; p->iterations = 32;
    return DH_OK;
}
// One surface call.  dev: frames / instances / subjects / fit records / records are device pointers and `stream` the caller's.
struct SurfaceReq {
    const uint16_t *frames; int n, w, h;
    const float *K; const dh_cameras *cams; bool use_cams;
    dh_fit_subjects *set;
    const dh_render_instance *inst; uint32_t n_inst;
    const uint32_t *subjects; uint32_t n_subjects;
    const dh_fit_record *fit_rec;
    const dh_surface_params *prm;
    dh_surface_record *rec;
};
static int surface_run(dh_fitter *f, const SurfaceReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.rec) return fail(DH_EINVAL, "%s: NULL records", who);
    if (!q.set) return fail(DH_EINVAL, "%s: NULL subject set", who);
    TRY(check_frames(q.n, q.w, q.h, q.K, q.cams, q.use_cams, f->device, "fitter", who));
    dh_fit_subjects *set = q.set;
    TRY(check_subjects(f, set, q.n_subjects, true, who));
    dh_surface_params prm;
    (void)fit_surface_params_default_(&prm);
    if (q.prm) prm = *q.prm;
    if (!std::isfinite(prm.gate) || !std::isfinite(prm.min_cos2) || !std::isfinite(prm.mu) || !std::isfinite(prm.eps))
        return fail(DH_EINVAL, "%s: gate %g, min_cos2 %g, mu %g, eps %g: a value is not finite", who, prm.gate, prm.min_cos2, prm.mu, prm.eps);
    if (!(prm.gate > 0.0 && prm.gate <= DH_SHAPE_MAX_GATE)) return fail(DH_EINVAL, "%s: gate = %g outside (0, %g]", who, prm.gate, DH_SHAPE_MAX_GATE);
    if (!(prm.min_cos2 >= 0.0 && prm.min_cos2 <= 1.0)) return fail(DH_EINVAL, "%s: min_cos2 = %g outside [0, 1]", who, prm.min_cos2);
    if (!(prm.mu >= 0.0)) return fail(DH_EINVAL, "%s: mu = %g below 0", who, prm.mu);
    if (!(prm.eps > 0.0)) return fail(DH_EINVAL, "%s: eps = %g, expected a value > 0", who, prm.eps);
    if (prm.min_count < 1) return fail(DH_EINVAL, "%s: min_count 0 below 1", who);
    if (prm.min_points < 1) return fail(DH_EINVAL, "%s: min_points 0 below 1", who);
    if (prm.iterations > DH_SURFACE_MAX_ITERATIONS) return fail(DH_EINVAL, "%s: iterations = %u above %u", who, prm.iterations, DH_SURFACE_MAX_ITERATIONS);
    if (prm.reserved0 || prm.reserved[0] || prm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (q.n_inst > DH_SHAPE_MAX_TERMS) return fail(DH_EINVAL, "%s: too many instances", who);
    const double largest = set->basis->largest;
    TRY(shape_check_terms(dev, q.inst, q.n_inst, q.subjects, q.n_subjects, q.fit_rec, q.n, set->n, set->radius, largest, DH_SURFACE_MAX_SCALE, who));

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    SurfaceArgs g;
    memset(&g, 0, sizeof g);
    ShapeArgs &a = g.s;
    args_frames(a, q.n, q.w, q.h, q.K, q.cams, q.use_cams);
    a.np = set->n; a.nk = set->basis->k;
    a.radius = set->radius; a.largest = largest;
    a.n_inst = q.n_inst; a.n_subjects = q.n_subjects;
    a.min_points = prm.min_points; a.gate = prm.gate;
    g.models = set->table.get();
    g.nb = set->nb.get(); g.nbr_begin = set->nbr_begin.get(); g.nbr = set->nbr.get();
    g.offsets = set->offsets.get(); g.rows = set->rows.get(); g.tally = set->tally.get(); g.scratch = set->scratch.get();
    g.state = set->state.get();
    g.min_cos2 = prm.min_cos2; g.mu = prm.mu; g.eps = prm.eps; g.max_offset = set->max_offset;
    g.min_count = prm.min_count; g.iterations = prm.iterations;
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n * q.w * q.h);
    args.in(&a.inst, q.inst, q.n_inst);
    args.in(&a.subjects, q.subjects, q.n_inst);
    args.in(&g.fit_rec, q.fit_rec, q.n_inst);
    args.out(&g.rec, q.rec, q.n_subjects, set->srec.get());   // (a surface set allocates nothing after its creation)
    TRY(args.commit());
    // ---- the five stream-ordered operations
    TRY(hip_step(dh_launch_surface_clear(g, s), "k_surface_clear"));
    TRY(hip_step(dh_launch_surface_accumulate(g, s), "k_surface_accumulate"));
    TRY(hip_step(dh_launch_surface_solve(g, s), "k_surface_solve"));
    TRY(hip_step(dh_launch_subjects_update_surface(SurfacePointsArgs{subjects_args(set, nullptr, 0, q.n_subjects), set->nb.get(), set->offsets.get()}, false, s),
                 "k_subjects_points_surface"));
    return args.finish();
}
static int fit_surface_subjects_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set,
                                 const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                 const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records) {
    return surface_run(f, SurfaceReq{frames, n, w, h, K, nullptr, false, set, instances, n_instances, subjects, n_subjects, fit_records, params, records},
                       false, nullptr, "dh_fit_surface_subjects");
}
static int fit_surface_subjects_cameras_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, dh_fit_subjects *set,
                                         const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                         const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records) {
    return surface_run(f, SurfaceReq{frames, n, w, h, nullptr, c, true, set, instances, n_instances, subjects, n_subjects, fit_records, params, records},
                       false, nullptr, "dh_fit_surface_subjects_cameras");
}
static int fit_surface_subjects_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set,
                                        const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                        const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records, void *stream) {
    return surface_run(f, SurfaceReq{frames, n, w, h, K, nullptr, false, set, instances, n_instances, subjects, n_subjects, fit_records, params, records},
                       true, (hipStream_t)stream, "dh_fit_surface_subjects_device");
}
static int fit_surface_subjects_cameras_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, dh_fit_subjects *set,
                                                const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                                                const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records, void *stream) {
    return surface_run(f, SurfaceReq{frames, n, w, h, nullptr, c, true, set, instances, n_instances, subjects, n_subjects, fit_records, params, records},
                       true, (hipStream_t)stream, "dh_fit_surface_subjects_cameras_device");
}

// ---- identifying the subject of a fitted head
static int fit_ident_params_default_(dh_ident_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_fit_ident_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->iterations = 4; p->min_points = 64;
    p->gate = 25.0; p->lambda = 1e-3;
    p->max_rms = DH_IDENT_DEFAULT_MAX_RMS; p->min_ratio = 1.0;
    return DH_OK;
}
// The refusals of an identify call's dh_ident_params in the header's order (NULL: the defaults with `default_max_rms`, section
// 27's or section 28's); *out is what the call runs with.
static int ident_params_check(const dh_ident_params *in, double default_max_rms, dh_ident_params *out, const char *who) {
    dh_ident_params prm;
    (void)fit_ident_params_default_(&prm);
    prm.max_rms = default_max_rms;
    if (in) prm = *in;
    if (std::isnan(prm.gate) || std::isnan(prm.lambda) || std::isnan(prm.max_rms) || std::isnan(prm.min_ratio))
        return fail(DH_EINVAL, "%s: gate %g, lambda %g, max_rms %g, min_ratio %g: a value is NaN", who, prm.gate, prm.lambda, prm.max_rms, prm.min_ratio);
    if (prm.iterations > 64) return fail(DH_EINVAL, "%s: iterations = %u above 64", who, prm.iterations);
    if (!(prm.gate > 0.0 && prm.gate <= 4096.0)) return fail(DH_EINVAL, "%s: gate = %g outside (0, 4096]", who, prm.gate);
    if (!(prm.lambda >= 0.0) || !std::isfinite(prm.lambda)) return fail(DH_EINVAL, "%s: lambda %g, expected a finite value >= 0", who, prm.lambda);
    if (prm.min_points < 6) return fail(DH_EINVAL, "%s: min_points %u below 6", who, prm.min_points);
    if (!(prm.max_rms > 0.0)) return fail(DH_EINVAL, "%s: max_rms = %g, expected a value > 0", who, prm.max_rms);
    if (!(prm.min_ratio >= 1.0)) return fail(DH_EINVAL, "%s: min_ratio = %g below 1", who, prm.min_ratio);
    if (prm.reserved[0] || prm.reserved[1] || prm.reserved[2]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    *out = prm;
    return DH_OK;
}
// (dh_runtime_fit.h: what the subject fit tracker's creation reads of a set and checks of its dh_ident_params)
void dh_fit_subjects_view_(const dh_fit_subjects *set, SubjectsView *v, FitModel *models) {
    *v = SubjectsView{set->device, set->n, set->n_subjects, set->radius, set->basis->largest, set->table.get()};
    if (models)
        for (uint32_t s = 0; s < set->n_subjects; ++s) models[s] = FitModel{set->models[s]->pts.get(), set->models[s]->nrm.get(), set->n, 0};
}
int dh_ident_params_check_(const dh_ident_params *in, dh_ident_params *out, const char *who) {
    return ident_params_check(in, DH_IDENT_DEFAULT_MAX_RMS, out, who);
}
int dh_ident_views_params_check_(const dh_ident_params *in, dh_ident_params *out, const char *who) {
    return ident_params_check(in, DH_IDENT_VIEWS_DEFAULT_MAX_RMS, out, who);
}
// The half of an IdentArgs or IdentViewsArgs that the set, the subject count and the (checked) params fill.
template <typename G>
static void ident_args_common(G &g, const dh_fit_subjects *set, uint32_t n_subjects, const dh_ident_params &prm) {
    g.f.coarse = 0; g.f.full = prm.iterations; g.f.min_points = prm.min_points;
    g.f.gate[0] = prm.gate; g.f.gate[1] = prm.gate;
    g.f.lam1 = 1.0 + prm.lambda;
    g.models = set->table.get();
    g.np = set->n; g.n_subjects = n_subjects;
    g.radius = set->radius; g.largest = set->basis->largest;
    g.max_ms = prm.max_rms * prm.max_rms; g.min_ratio = prm.min_ratio;
}
// One identify call.  dev: frames / instances / enrolled / fit records / every output are device pointers and `stream` the caller's.
struct IdentReq {
    const uint16_t *frames; int n, w, h;
    const float *K; const dh_cameras *cams; bool use_cams;
    const dh_fit_subjects *set;
    const dh_render_instance *inst; uint32_t n_inst;
    const uint8_t *enrolled; uint32_t n_subjects;
    const dh_fit_record *fit_rec;
    const dh_ident_params *prm;
    uint32_t *subjects_out; dh_ident_record *rec; dh_render_instance *poses_out; dh_fit_record *scores;
};
static int ident_run(dh_fitter *f, const IdentReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.subjects_out) return fail(DH_EINVAL, "%s: NULL subjects_out", who);
    if (!q.rec) return fail(DH_EINVAL, "%s: NULL records", who);
    if (!q.set) return fail(DH_EINVAL, "%s: NULL subject set", who);
    TRY(check_frames(q.n, q.w, q.h, q.K, q.cams, q.use_cams, f->device, "fitter", who));
    const dh_fit_subjects *set = q.set;
    TRY(check_subjects(f, set, q.n_subjects, false, who));
    dh_ident_params prm;
    TRY(ident_params_check(q.prm, DH_IDENT_DEFAULT_MAX_RMS, &prm, who));
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    const uint64_t pairs = (uint64_t)q.n_inst * q.n_subjects;
    if (pairs > DH_IDENT_MAX_PAIRS)
        return fail(DH_EINVAL, "%s: %u instances times %u subjects exceed %u pairs", who, q.n_inst, q.n_subjects, DH_IDENT_MAX_PAIRS);
    if (q.n_inst == 0) return DH_OK;
    const double largest = set->basis->largest;
    if (!dev)
        for (uint32_t i = 0; i < q.n_inst; ++i) {
            if (q.fit_rec && q.fit_rec[i].status != DH_FIT_OK) continue;
            const dh_render_instance &in = q.inst[i];
            if (in.frame >= (uint32_t)q.n) return fail(DH_EINVAL, "%s: instance %u names frame %u of %d", who, i, in.frame, q.n);
            TRY(instance_refusal(dh_fit_instance_fault(in, set->radius, largest), in.scale, i, set->radius, largest, who));
        }

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    IdentArgs g;
    memset(&g, 0, sizeof g);
    FitArgs &a = g.f;
    args_frames(a, q.n, q.w, q.h, q.K, q.cams, q.use_cams);
    a.n_inst = q.n_inst;
    ident_args_common(g, set, q.n_subjects, prm);
    // ---- the pair scratch: the fitter's, grown on demand (growing waits for the device, as the other tables do)
    const bool own_scores = !dev || !q.scores;
    if ((own_scores && f->ident_score.cap() < pairs) || f->ident_pose.cap() < pairs * 12) {
        HIP_TRY(hipDeviceSynchronize());
        if (own_scores) TRY(f->ident_score.grow((size_t)pairs));
        TRY(f->ident_pose.grow((size_t)pairs * 12));
    }
    g.pose = f->ident_pose.get();
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n * q.w * q.h);
    args.in(&a.inst, q.inst, q.n_inst);
    args.in(&g.enrolled, q.enrolled, q.n_subjects);
    args.in(&g.fit_rec, q.fit_rec, q.n_inst);
    args.out(&g.subjects_out, q.subjects_out, q.n_inst);
    args.out(&g.rec, q.rec, q.n_inst);
    args.out(&g.poses_out, q.poses_out, q.n_inst);
    args.out(&g.score, q.scores, (size_t)pairs, f->ident_score.get());
    TRY(args.commit());
    // ---- the two stream-ordered operations
    TRY(hip_step(dh_launch_ident_score(g, s), "k_ident_score"));
    TRY(hip_step(dh_launch_ident_decide(g, s), "k_ident_decide"));
    return args.finish();
}
static int fit_identify_subjects_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                                  const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects,
                                  const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                  dh_render_instance *poses_out, dh_fit_record *scores) {
    return ident_run(f, IdentReq{frames, n, w, h, K, nullptr, false, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                     false, nullptr, "dh_fit_identify_subjects");
}
static int fit_identify_subjects_cameras_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set,
                                          const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects,
                                          const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                          dh_render_instance *poses_out, dh_fit_record *scores) {
    return ident_run(f, IdentReq{frames, n, w, h, nullptr, c, true, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                     false, nullptr, "dh_fit_identify_subjects_cameras");
}
static int fit_identify_subjects_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                                         const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects,
                                         const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                         dh_render_instance *poses_out, dh_fit_record *scores, void *stream) {
    return ident_run(f, IdentReq{frames, n, w, h, K, nullptr, false, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                     true, (hipStream_t)stream, "dh_fit_identify_subjects_device");
}
static int fit_identify_subjects_cameras_device_(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set,
                                                 const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects,
                                                 const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                                 dh_render_instance *poses_out, dh_fit_record *scores, void *stream) {
    return ident_run(f, IdentReq{frames, n, w, h, nullptr, c, true, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                     true, (hipStream_t)stream, "dh_fit_identify_subjects_cameras_device");
}

// ---- identifying enrolled subjects across the views of a rig
static int fit_ident_views_params_default_(dh_ident_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_fit_ident_views_params_default: NULL argument");
    (void)fit_ident_params_default_(p);
    p->max_rms = DH_IDENT_VIEWS_DEFAULT_MAX_RMS;
    return DH_OK;
}
// What dh_shape_views_skip or dh_calib_skip found in instance i of a host multi-view call, as the call's refusal; DH_OK where the
// instance takes part or is left out.
static int views_skip_refusal(const ShapeViewsSkip &sk, const dh_view_instance &in, uint32_t i, int n, uint32_t set, uint32_t n_sets, uint32_t sj,
                              uint32_t n_subjects, double radius, double largest, const char *who) {
    switch (sk.why) {
    case DH_SHAPE_VIEWS_OK: case DH_SHAPE_VIEWS_SKIPPED: return DH_OK;
    case DH_SHAPE_VIEWS_NO_VIEW: return fail(DH_EINVAL, "%s: instance %u is seen by no view", who, i);
    case DH_SHAPE_VIEWS_CAMERA: return fail(DH_EINVAL, "%s: instance %u names camera %llu of %d", who, i, (unsigned long long)sk.last, n);
    case DH_SHAPE_VIEWS_SET: return fail(DH_EINVAL, "%s: instance %u names set %u of %u", who, i, set, n_sets);
    case DH_SHAPE_VIEWS_SUBJECT: return fail(DH_EINVAL, "%s: instance %u names subject %u of %u", who, i, sj, n_subjects);
    default: return instance_refusal(sk.fault, in.scale, i, radius, largest, who);
    }
}
// One multi-view identify call.  dev: frames / instances / sets / enrolled / fit records / every output are device pointers and
// `stream` the caller's.
struct IdentViewsReq {
    const uint16_t *frames; uint32_t n_sets; int w, h;
    const dh_fit_views *views;
    const dh_fit_subjects *set;
    const dh_view_instance *inst; uint32_t n_inst;
    const uint32_t *sets; const uint8_t *enrolled; uint32_t n_subjects;
    const dh_view_fit_record *fit_rec;
    const dh_ident_params *prm;
    uint32_t *subjects_out; dh_ident_record *rec; dh_view_instance *poses_out; dh_view_fit_record *scores;
};
static int ident_views_run(dh_fitter *f, const IdentViewsReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.subjects_out) return fail(DH_EINVAL, "%s: NULL subjects_out", who);
    if (!q.rec) return fail(DH_EINVAL, "%s: NULL records", who);
    if (!q.set) return fail(DH_EINVAL, "%s: NULL subject set", who);
    int n = 0;
    TRY(check_views(f, q.views, &q.n_sets, q.w, q.h, &n, who));
    const dh_fit_subjects *set = q.set;
    TRY(check_subjects(f, set, q.n_subjects, false, who));
    dh_ident_params prm;
    TRY(ident_params_check(q.prm, DH_IDENT_VIEWS_DEFAULT_MAX_RMS, &prm, who));
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    const uint64_t pairs = (uint64_t)q.n_inst * q.n_subjects;
    if (pairs > DH_IDENT_MAX_PAIRS)
        return fail(DH_EINVAL, "%s: %u instances times %u subjects exceed %u pairs", who, q.n_inst, q.n_subjects, DH_IDENT_MAX_PAIRS);
    if (q.n_inst == 0) return DH_OK;
    const double largest = set->basis->largest;
    if (!dev)
        for (uint32_t i = 0; i < q.n_inst; ++i) {
            const dh_view_instance &in = q.inst[i];
            const uint32_t st = q.sets ? q.sets[i] : 0u;
            const IdentViewsPart part = dh_ident_views_part(in, st, q.fit_rec ? q.fit_rec + i : nullptr, (uint32_t)n, q.n_sets, set->n, set->radius, largest);
            switch (part.why) {
            case DH_IDENT_VIEWS_OK: case DH_IDENT_VIEWS_RECORD: break;
            case DH_IDENT_VIEWS_WHERE: case DH_IDENT_VIEWS_FAULT:      // (the view, the camera or the set; R, t or scale)
                return views_skip_refusal(part.skip, in, i, n, st, q.n_sets, 0u, 1u, set->radius, largest, who);
            default:
                return fail(DH_EINVAL, "%s: instance %u sums %llu terms (%d views of %u points), above %u", who, i, (unsigned long long)part.terms,
                            __builtin_popcountll(in.views), set->n, DH_FIT_MAX_POINTS);
            }
        }

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    IdentViewsArgs g;
    memset(&g, 0, sizeof g);
    FitViewsArgs &a = g.f;
    a.n = n; a.w = q.w; a.h = q.h;
    a.cams = q.views->cams->dev.get();
    a.views = q.views->dev.get();
    a.n_inst = q.n_inst;
    ident_args_common(g, set, q.n_subjects, prm);
    g.n_sets = q.n_sets;
    // ---- the pair scratch: the fitter's, grown on demand (growing waits for the device, as the other tables do); the poses are
    // section 27's buffer, which is why all identify calls of a fitter must be stream-ordered with one another
    const bool own_scores = !dev || !q.scores;
    if ((own_scores && f->ident_vscore.cap() < pairs) || f->ident_pose.cap() < pairs * 12) {
        HIP_TRY(hipDeviceSynchronize());
        if (own_scores) TRY(f->ident_vscore.grow((size_t)pairs));
        TRY(f->ident_pose.grow((size_t)pairs * 12));
    }
    g.pose = f->ident_pose.get();
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n_sets * n * q.w * q.h);
    args.in(&a.inst, q.inst, q.n_inst);
    args.in(&g.sets, q.sets, q.n_inst);
    args.in(&g.enrolled, q.enrolled, q.n_subjects);
    args.in(&g.fit_rec, q.fit_rec, q.n_inst);
    args.out(&g.subjects_out, q.subjects_out, q.n_inst);
    args.out(&g.rec, q.rec, q.n_inst);
    args.out(&g.poses_out, q.poses_out, q.n_inst);
    args.out(&g.score, q.scores, (size_t)pairs, f->ident_vscore.get());
    TRY(args.commit());
    // ---- the two stream-ordered operations
    TRY(hip_step(dh_launch_ident_views_score(g, s), "k_ident_views_score"));
    TRY(hip_step(dh_launch_ident_views_decide(g, s), "k_ident_views_decide"));
    return args.finish();
}
static int fit_identify_subjects_views_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_subjects *set,
                                        const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects,
                                        const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                        dh_view_instance *poses_out, dh_view_fit_record *scores) {
    return ident_views_run(f, IdentViewsReq{frames, n_sets, w, h, views, set, instances, n_instances, sets, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                           false, nullptr, "dh_fit_identify_subjects_views");
}
static int fit_identify_subjects_views_device_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_subjects *set,
                                               const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects,
                                               const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                               dh_view_instance *poses_out, dh_view_fit_record *scores, void *stream) {
    return ident_views_run(f, IdentViewsReq{frames, n_sets, w, h, views, set, instances, n_instances, sets, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores},
                           true, (hipStream_t)stream, "dh_fit_identify_subjects_views_device");
}

// ------------------------------------------------------------------ adapting a model's shape across views
// One multi-view shape call. dev: frames / instances / sets / subjects / records are device pointers and `stream` the caller's.
struct ShapeViewsReq {
    const uint16_t *frames; uint32_t n_sets; int w, h;
    const dh_fit_views *views;
    const dh_fit_model *model; const dh_fit_basis *basis;
    const dh_view_instance *inst; uint32_t n_inst;
    const uint32_t *sets; const uint32_t *subjects; uint32_t n_subjects;
    const dh_shape_params *prm;
    dh_shape_record *rec;
};
static int shape_views_run(dh_fitter *f, const ShapeViewsReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    TRY(shape_check_pointers(f, q.frames, q.rec, q.model, q.basis, who));
    int n = 0;
    TRY(check_views(f, q.views, &q.n_sets, q.w, q.h, &n, who));
    dh_shape_params prm;
    TRY(shape_check_call(f, q.model, q.basis, q.n_subjects, q.prm, &prm, q.inst, q.n_inst, who));
    const dh_fit_model *m = q.model;
    const dh_fit_basis *b = q.basis;
    const uint32_t ranks = (uint32_t)std::min(64, n);
    if (dev) {
        if ((uint64_t)q.n_inst * ranks * m->n > DH_SHAPE_MAX_TERMS)
            return fail(DH_EINVAL, "%s: %u instances of %u views of %u points exceed %u terms", who, q.n_inst, ranks, m->n, DH_SHAPE_MAX_TERMS);
    } else {
        std::vector<uint64_t> per(q.n_subjects, 0);
        for (uint32_t i = 0; i < q.n_inst; ++i) {
            const dh_view_instance &in = q.inst[i];
            const uint32_t sj = q.subjects ? q.subjects[i] : 0u, set = q.sets ? q.sets[i] : 0u;
            const ShapeViewsSkip sk = dh_shape_views_skip(in, set, sj, (uint32_t)n, q.n_sets, q.n_subjects, m->radius, b->largest);
            TRY(views_skip_refusal(sk, in, i, n, set, q.n_sets, sj, q.n_subjects, m->radius, b->largest, who));
            if (sk.why == DH_SHAPE_VIEWS_SKIPPED) continue;
            per[sj] += (uint64_t)__builtin_popcountll(in.views) * m->n;
            if (per[sj] > DH_SHAPE_MAX_TERMS)
                return fail(DH_EINVAL, "%s: subject %u has more than %u terms (views times %u points)", who, sj, DH_SHAPE_MAX_TERMS, m->n);
        }
    }

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    if (!f->shape_sums) TRY(f->shape_sums.alloc((size_t)DH_SHAPE_MAX_SUBJECTS * DH_SHAPE_STRIDE));
    ShapeViewsArgs v;
    memset(&v, 0, sizeof v);
    ShapeArgs &a = v.s;
    a.n = n; a.w = q.w; a.h = q.h;
    a.cams = q.views->cams->dev.get();
    shape_args_common(a, f, m, b, q.n_inst, q.n_subjects, prm);
    v.views = q.views->dev.get();
    v.n_sets = q.n_sets; v.ranks = ranks;
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n_sets * n * q.w * q.h);
    args.in(&v.inst, q.inst, q.n_inst);
    args.in(&a.subjects, q.subjects, q.n_inst);
    args.in(&v.sets, q.sets, q.n_inst);
    args.out(&a.rec, q.rec, q.n_subjects);
    TRY(args.commit());
    // ---- the three stream-ordered operations
    TRY(hip_step(dh_launch_shape_clear(a, s), "k_shape_clear"));
    TRY(hip_step(dh_launch_shape_accumulate_views(v, s), "k_shape_accumulate_views"));
    TRY(hip_step(dh_launch_shape_solve(a, s), "k_shape_solve"));
    return args.finish();
}
static int fit_shape_views_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model,
                            const dh_fit_basis *basis, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets,
                            const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records) {
    return shape_views_run(f, ShapeViewsReq{frames, n_sets, w, h, views, model, basis, instances, n_instances, sets, subjects, n_subjects, params, records},
                           false, nullptr, "dh_fit_shape_views");
}
static int fit_shape_views_device_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model,
                                   const dh_fit_basis *basis, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets,
                                   const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records, void *stream) {
    return shape_views_run(f, ShapeViewsReq{frames, n_sets, w, h, views, model, basis, instances, n_instances, sets, subjects, n_subjects, params, records},
                           true, (hipStream_t)stream, "dh_fit_shape_views_device");
}

// ------------------------------------------------------------------ calibrating a view table
static int calib_params_default_(dh_calib_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_calib_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->gate = 25.0;
    p->lambda = 1e-3;
    p->min_points = 64;
    return DH_OK;
}
// One calibration call.  dev: frames / instances / sets / take / hold / records are device pointers and `stream` the caller's.
struct CalibReq {
    const uint16_t *frames; uint32_t n_sets; int w, h;
    const dh_fit_views *views;
    const dh_fit_model *model;
    const dh_view_instance *inst; uint32_t n_inst;
    const uint32_t *sets; const uint32_t *take; const uint8_t *hold;
    const dh_calib_params *prm;
    dh_calib_record *rec;
};
static int calib_run(dh_fitter *f, const CalibReq &q, bool dev, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!f) return fail(DH_EINVAL, "%s: NULL fitter", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    if (!q.rec) return fail(DH_EINVAL, "%s: NULL records", who);
    if (!q.model) return fail(DH_EINVAL, "%s: NULL model", who);
    int n = 0;
    TRY(check_views(f, q.views, &q.n_sets, q.w, q.h, &n, who));
    dh_calib_params prm;
    (void)calib_params_default_(&prm);
    if (q.prm) prm = *q.prm;
    if (!(prm.gate > 0.0 && prm.gate <= DH_SHAPE_MAX_GATE)) return fail(DH_EINVAL, "%s: gate = %g outside (0, %g]", who, prm.gate, DH_SHAPE_MAX_GATE);
    if (!(prm.lambda >= 0.0) || !std::isfinite(prm.lambda)) return fail(DH_EINVAL, "%s: lambda %g, expected a finite value >= 0", who, prm.lambda);
    if (prm.min_points < 1) return fail(DH_EINVAL, "%s: min_points 0 below 1", who);
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(prm.pivot[j])) return fail(DH_EINVAL, "%s: pivot[%d] is not finite", who, j);
    if (prm.reserved0 || prm.reserved[0] || prm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    const dh_fit_model *m = q.model;
    if (m->device != f->device) return fail(DH_EINVAL, "%s: the model lives on device %d, the fitter on %d", who, m->device, f->device);
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (q.n_inst > DH_SHAPE_MAX_TERMS) return fail(DH_EINVAL, "%s: too many instances", who);
    if (dev) {
        if ((uint64_t)q.n_inst * m->n > DH_SHAPE_MAX_TERMS)
            return fail(DH_EINVAL, "%s: %u instances of %u points exceed %u terms", who, q.n_inst, m->n, DH_SHAPE_MAX_TERMS);
    } else {
        std::vector<uint64_t> per((size_t)n, 0);
        for (uint32_t i = 0; i < q.n_inst; ++i) {
            const dh_view_instance &in = q.inst[i];
            const uint32_t tk = q.take ? q.take[i] : 0u, set = q.sets ? q.sets[i] : 0u;
            const ShapeViewsSkip sk = dh_calib_skip(in, set, tk, (uint32_t)n, q.n_sets, m->radius);
            TRY(views_skip_refusal(sk, in, i, n, set, q.n_sets, 0u, 1u, m->radius, 0.0, who));
            if (sk.why == DH_SHAPE_VIEWS_SKIPPED) continue;
            for (uint32_t k = 0; k < 64; ++k) {
                if (!((in.views >> k) & 1ull)) continue;
                const uint32_t c = in.first_cam + k;
                if (q.hold && q.hold[c] != 0) continue;                   // (a pair beyond the arm counts: only the device forms it)
                per[c] += m->n;
                if (per[c] > DH_SHAPE_MAX_TERMS)
                    return fail(DH_EINVAL, "%s: camera %u has more than %u terms (pairs times %u points)", who, c, DH_SHAPE_MAX_TERMS, m->n);
            }
        }
    }

    DeviceGuard guard(f->device);
    if (!guard.ok) return DH_EHIP;
    TRY(f->tab.init());
    hipStream_t s = dev ? stream : f->tab.s;
    const size_t words = (size_t)n * DH_CALIB_STRIDE;
    if (f->calib_sums.cap() < words) { HIP_TRY(hipDeviceSynchronize()); TRY(f->calib_sums.grow(words)); }
    CalibArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.w = q.w; a.h = q.h;
    a.cams = q.views->cams->dev.get();
    a.views = q.views->dev.get();
    a.pts = m->pts.get(); a.nrm = m->nrm.get(); a.np = m->n; a.radius = m->radius;
    a.n_inst = q.n_inst; a.n_sets = q.n_sets; a.ranks = (uint32_t)std::min(64, n);
    a.min_points = prm.min_points; a.gate = prm.gate; a.lam1 = 1.0 + prm.lambda;
    for (int j = 0; j < 3; ++j) a.pivot[j] = prm.pivot[j];
    a.sums = f->calib_sums.get();
    CallArgs args(f, dev, s);
    args.in(&a.frames, q.frames, (size_t)q.n_sets * n * q.w * q.h);
    args.in(&a.inst, q.inst, q.n_inst);
    args.in(&a.take, q.take, q.n_inst);
    args.in(&a.sets, q.sets, q.n_inst);
    args.in(&a.hold, q.hold, (size_t)n);
    args.out(&a.rec, q.rec, (size_t)n);
    TRY(args.commit());
    // ---- the three stream-ordered operations
    TRY(hip_step(dh_launch_calib_clear(a, s), "k_calib_clear"));
    TRY(hip_step(dh_launch_calib_accumulate(a, s), "k_calib_accumulate"));
    TRY(hip_step(dh_launch_calib_solve(a, s), "k_calib_solve"));
    return args.finish();
}
static int fit_calibrate_views_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model,
                                const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *take, const uint8_t *hold,
                                const dh_calib_params *params, dh_calib_record *records) {
    return calib_run(f, CalibReq{frames, n_sets, w, h, views, model, instances, n_instances, sets, take, hold, params, records}, false, nullptr,
                     "dh_fit_calibrate_views");
}
static int fit_calibrate_views_device_(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model,
                                       const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *take, const uint8_t *hold,
                                       const dh_calib_params *params, dh_calib_record *records, void *stream) {
    return calib_run(f, CalibReq{frames, n_sets, w, h, views, model, instances, n_instances, sets, take, hold, params, records}, true, (hipStream_t)stream,
                     "dh_fit_calibrate_views_device");
}

// ------------------------------------------------------------------ the C ABI (DH_API: dh_runtime.h)
DH_API(fit_model_create, (const float *points, const float *normals, uint32_t n, int device, dh_fit_model **out), (points, normals, n, device, out))
DH_API(fit_model_destroy, (dh_fit_model *m), (m))
DH_API(fit_model_info, (const dh_fit_model *m, uint32_t *n, double *radius), (m, n, radius))
DH_API(fit_params_default, (dh_fit_params *p), (p))
DH_API(fitter_create, (int device, dh_fitter **out), (device, out))
DH_API(fitter_destroy, (dh_fitter *f), (f))
DH_API(fit_depth, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records), (f, frames, n, w, h, K, models, n_models, instances, n_instances, params, out, records))
DH_API(fit_depth_cameras, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records), (f, frames, n, w, h, c, models, n_models, instances, n_instances, params, out, records))
DH_API(fit_depth_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream), (f, frames, n, w, h, K, models, n_models, instances, n_instances, params, out, records, stream))
DH_API(fit_depth_cameras_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream), (f, frames, n, w, h, c, models, n_models, instances, n_instances, params, out, records, stream))
DH_API(fit_views_create, (const dh_cameras *c, const float *V, const float *u, dh_fit_views **out), (c, V, u, out))
DH_API(fit_views_destroy, (dh_fit_views *v), (v))
DH_API(fit_views_info, (const dh_fit_views *v, int *n, int *device), (v, n, device))
DH_API(fit_depth_views, (dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views, const dh_fit_model *const *models, uint32_t n_models, const dh_view_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out, dh_view_fit_record *records), (f, frames, w, h, views, models, n_models, instances, n_instances, params, out, records))
DH_API(fit_depth_views_device, (dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views, const dh_fit_model *const *models, uint32_t n_models, const dh_view_instance *instances, uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out, dh_view_fit_record *records, void *stream), (f, frames, w, h, views, models, n_models, instances, n_instances, params, out, records, stream))
DH_API(fit_basis_create, (const float *fields, uint32_t n, uint32_t n_fields, int device, dh_fit_basis **out), (fields, n, n_fields, device, out))
DH_API(fit_basis_destroy, (dh_fit_basis *b), (b))
DH_API(fit_basis_info, (const dh_fit_basis *b, uint32_t *n, uint32_t *n_fields, double *largest), (b, n, n_fields, largest))
DH_API(shape_params_default, (dh_shape_params *p), (p))
DH_API(fit_shape, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model, const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records), (f, frames, n, w, h, K, model, basis, instances, n_instances, subjects, n_subjects, params, records))
DH_API(fit_shape_cameras, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *model, const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records), (f, frames, n, w, h, c, model, basis, instances, n_instances, subjects, n_subjects, params, records))
DH_API(fit_shape_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model, const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records, void *stream), (f, frames, n, w, h, K, model, basis, instances, n_instances, subjects, n_subjects, params, records, stream))
DH_API(fit_shape_cameras_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *model, const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records, void *stream), (f, frames, n, w, h, c, model, basis, instances, n_instances, subjects, n_subjects, params, records, stream))
DH_API(fit_shape_views, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model, const dh_fit_basis *basis, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records), (f, frames, n_sets, w, h, views, model, basis, instances, n_instances, sets, subjects, n_subjects, params, records))
DH_API(fit_shape_views_device, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model, const dh_fit_basis *basis, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records, void *stream), (f, frames, n_sets, w, h, views, model, basis, instances, n_instances, sets, subjects, n_subjects, params, records, stream))
DH_API(calib_params_default, (dh_calib_params *p), (p))
DH_API(fit_calibrate_views, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *take, const uint8_t *hold, const dh_calib_params *params, dh_calib_record *records), (f, frames, n_sets, w, h, views, model, instances, n_instances, sets, take, hold, params, records))
DH_API(fit_depth_carried_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_render_instance *carried, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream), (f, frames, n, w, h, K, models, n_models, instances, n_instances, carried, params, out, records, stream))
DH_API(fit_depth_cameras_carried_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_render_instance *carried, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records, void *stream), (f, frames, n, w, h, c, models, n_models, instances, n_instances, carried, params, out, records, stream))
DH_API(fit_subjects_create, (const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis, uint32_t n_subjects, double max_coeff, int device, dh_fit_subjects **out), (verts, n, tris, n_tris, basis, n_subjects, max_coeff, device, out))
DH_API(fit_subjects_destroy, (dh_fit_subjects *s), (s))
DH_API(fit_subjects_info, (const dh_fit_subjects *s, uint32_t *n, uint32_t *n_tris, uint32_t *n_fields, uint32_t *n_subjects, double *radius, int *device), (s, n, n_tris, n_fields, n_subjects, radius, device))
DH_API(fit_subjects_model, (const dh_fit_subjects *s, uint32_t subject, const dh_fit_model **model), (s, subject, model))
DH_API(fit_subjects_set_coeffs, (dh_fit_subjects *s, uint32_t first, uint32_t count, const double *coeffs), (s, first, count, coeffs))
DH_API(fit_subjects_state, (dh_fit_subjects *s, dh_subject_state *state), (s, state))
DH_API(fit_subjects_read, (dh_fit_subjects *s, uint32_t subject, float *points, float *normals), (s, subject, points, normals))
DH_API(fit_subjects_update, (dh_fit_subjects *s, const dh_shape_record *records), (s, records))
DH_API(fit_subjects_update_device, (dh_fit_subjects *s, const dh_shape_record *records, void *stream), (s, records, stream))
DH_API(fit_subjects_create_surface, (const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis, uint32_t n_subjects, double max_coeff, double max_offset, int device, dh_fit_subjects **out), (verts, n, tris, n_tris, basis, n_subjects, max_coeff, max_offset, device, out))
DH_API(fit_subjects_set_offsets, (dh_fit_subjects *s, uint32_t subject, const double *offsets), (s, subject, offsets))
DH_API(fit_subjects_read_offsets, (dh_fit_subjects *s, uint32_t subject, double *offsets, uint32_t *counts), (s, subject, offsets, counts))
DH_API(fit_surface_params_default, (dh_surface_params *p), (p))
DH_API(fit_surface_subjects, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records), (f, frames, n, w, h, K, set, instances, n_instances, subjects, n_subjects, fit_records, params, records))
DH_API(fit_surface_subjects_cameras, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records), (f, frames, n, w, h, c, set, instances, n_instances, subjects, n_subjects, fit_records, params, records))
DH_API(fit_surface_subjects_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records, void *stream), (f, frames, n, w, h, K, set, instances, n_instances, subjects, n_subjects, fit_records, params, records, stream))
DH_API(fit_surface_subjects_cameras_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records, void *stream), (f, frames, n, w, h, c, set, instances, n_instances, subjects, n_subjects, fit_records, params, records, stream))
DH_API(fit_ident_params_default, (dh_ident_params *p), (p))
DH_API(fit_identify_subjects, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_render_instance *poses_out, dh_fit_record *scores), (f, frames, n, w, h, K, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores))
DH_API(fit_identify_subjects_cameras, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_render_instance *poses_out, dh_fit_record *scores), (f, frames, n, w, h, c, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores))
DH_API(fit_identify_subjects_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_render_instance *poses_out, dh_fit_record *scores, void *stream), (f, frames, n, w, h, K, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores, stream))
DH_API(fit_identify_subjects_cameras_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_render_instance *poses_out, dh_fit_record *scores, void *stream), (f, frames, n, w, h, c, set, instances, n_instances, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores, stream))
DH_API(fit_ident_views_params_default, (dh_ident_params *p), (p))
DH_API(fit_identify_subjects_views, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_subjects *set, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects, const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_view_instance *poses_out, dh_view_fit_record *scores), (f, frames, n_sets, w, h, views, set, instances, n_instances, sets, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores))
DH_API(fit_identify_subjects_views_device, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_subjects *set, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects, const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records, dh_view_instance *poses_out, dh_view_fit_record *scores, void *stream), (f, frames, n_sets, w, h, views, set, instances, n_instances, sets, enrolled, n_subjects, fit_records, params, subjects_out, records, poses_out, scores, stream))
DH_API(fit_shape_subjects, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records), (f, frames, n, w, h, K, set, instances, n_instances, subjects, n_subjects, fit_records, params, records))
DH_API(fit_shape_subjects_cameras, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records), (f, frames, n, w, h, c, set, instances, n_instances, subjects, n_subjects, fit_records, params, records))
DH_API(fit_shape_subjects_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records, void *stream), (f, frames, n, w, h, K, set, instances, n_instances, subjects, n_subjects, fit_records, params, records, stream))
DH_API(fit_shape_subjects_cameras_device, (dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records, void *stream), (f, frames, n, w, h, c, set, instances, n_instances, subjects, n_subjects, fit_records, params, records, stream))
DH_API(fit_calibrate_views_device, (dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views, const dh_fit_model *model, const dh_view_instance *instances, uint32_t n_instances, const uint32_t *sets, const uint32_t *take, const uint8_t *hold, const dh_calib_params *params, dh_calib_record *records, void *stream), (f, frames, n_sets, w, h, views, model, instances, n_instances, sets, take, hold, params, records, stream))
