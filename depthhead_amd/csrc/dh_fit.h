// dh_fit.h -- what the fit family's kernels (k_fit.hip, k_fit_track.hip, k_fit_shape.hip, k_fit_views.hip, k_rig_fit_track.hip,
// k_fit_shape_views.hip, k_calib_views.hip, k_subjects.hip, k_surface.hip, k_ident.hip, k_ident_views.hip, k_subject_track.hip, k_rig_subject_track.hip) share with the host runtime (dh_api_fit.hip, dh_api_fit_track.hip): the argument blocks, table layouts and launchers, the layout of the sums, the seed
// words of both trackers, and the one test of whether an instance may be fitted (dh_fit_instance_fault: the host's refusals and
// the shape kernel's skips).  The device arithmetic the kernels share among themselves is in dh_fit_device.h.  Not part of the
// ABI.  The rules are stated in include/depthhead_hip.h (sections "fitting posed models to depth frames" and after) and
// DESIGN.md sections 18 - 30.
#pragma once
#include "dh_internal.h"
#include "dh_rig_fit.h"

static_assert(sizeof(dh_fit_params) == 56, "dh_fit_params: 56 bytes");
static_assert(sizeof(dh_fit_record) == 24, "dh_fit_record: 24 bytes");

#define DH_FIT_THREADS 256
// Fixed point of the sums: S = 2^20.  Magnitude: an instance's R is refused unless |R R^T - I| <= DH_FIT_R_TOLERANCE per element,
// so |R x| <= 1.03 |x|; normals have |m| <= 1.01: |nrm| <= 1.05, |J_a| <= 1.09 * 4096 (DH_FIT_MAX_EXTENT), and |r| <= 1.05 *
// (|p| / p.z) * gate with gates up to 4096.  While |p| <= 2 p.z (a field of view below 120 degrees) one product stays below
// 2^27; times 2^20, times 2^15 points (DH_FIT_MAX_POINTS): below 2^62 < 2^63.  The header says what holds outside that.
#define DH_FIT_S 1048576.0
#define DH_FIT_SUMS 29              // 21 A_ab (a <= b), 6 b_a, e and the count
// The words of the reduction: A_ab at DH_FIT_PAIR(6, a, b) (a <= b, row after row of the upper triangle), then b_a, e and the
// count; the multi-view fit keeps the mask of the views that were used in the word after them.
#define DH_FIT_B 21
#define DH_FIT_E 27
#define DH_FIT_COUNT 28
#define DH_FIT_USED 29
static_assert(DH_FIT_COUNT + 1 == DH_FIT_SUMS && DH_FIT_USED < 32, "29 words and the mask, in the 32 words of a kernel's s_sum");
// Where A_ab (a <= b) lies among sums laid out row after row as the upper triangle of a W x W matrix (the fit: 6, the shape step: 8)
#define DH_FIT_PAIR(W, a, b) ((a) * (W) - (a) * ((a) - 1) / 2 + ((b) - (a)))
// Points and normals are staged in LDS (24 bytes a point) up to this many points: 24 KB, which leaves six workgroups to a CU's
// 160 KB.  Larger models stream from global memory (L2-resident: every pass reads the same 24 n bytes).
#define DH_FIT_LDS_POINTS 1024

// One model of a fit call (device pointers of a dh_fit_model).
struct FitModel {
    const float *pts;         // [n][3]
    const float *nrm;         // [n][3]
    uint32_t n;
    uint32_t pad;
};

struct FitArgs {
    const uint16_t *frames;       // [n][h][w]
    int n, w, h;
    float k[9];                   // the one K of the batch (cams == NULL)
    const DhCam *cams;            // nullable [n]: frame f sees cams[f].k
    const FitModel *models;
    const dh_render_instance *inst;
    uint32_t n_inst;
    uint32_t coarse, full, min_points;
    double gate[2];
    double lam1;                  // 1.0 + lambda (computed on the host: one f64 sum)
    dh_render_instance *out;      // [n_inst]
    dh_fit_record *rec;           // [n_inst]
};

hipError_t dh_launch_fit(const FitArgs &a, hipStream_t s);

// Why an instance may not be fitted: the per-instance refusals of the header in their order, stated once for the host loops
// (which turn the answer into their messages) and the shape kernel (which skips).  The magnitude bounds of the int64 sums, here
// and at DH_SHAPE_*, rest on it.  radius: the model's largest |v|; largest: the basis's largest |B_k[i]| (0.0 where there is none).
// (instance_model_refusal, dh_api_fit.hip, relies on the order of these values: it reports what comes before EXTENT, then the model's
// own refusals, then the rest)
enum { DH_FIT_INST_OK = 0, DH_FIT_INST_NOT_FINITE, DH_FIT_INST_NOT_ORTHONORMAL, DH_FIT_INST_EXTENT, DH_FIT_INST_FIELD };
struct FitInstanceFault {
    int why;                      // DH_FIT_INST_*
    int a, b;                     // NOT_ORTHONORMAL: the first element of R R^T (row after row, a <= b) out of tolerance
    double g;                     //   and its value
};
// Instance: dh_render_instance or dh_view_instance (whose R and t are the world pose); R, t and scale are what is read.
template <typename Instance>
__host__ __device__ inline FitInstanceFault dh_fit_instance_fault(const Instance &in, double radius, double largest) {
    // Every test is made, none branches.  The tests run from the LAST refusal of the header's order to the FIRST and each
    // failure overwrites the answer, so what is left at the end is the first failure in the header's order -- for R, the
    // first (a, b) row after row, which the host message prints.
    FitInstanceFault f{DH_FIT_INST_OK, 0, 0, 0.0};
    const double sc = (double)in.scale;
    const double as = sc < 0.0 ? -sc : sc;
    if (!(as * largest <= DH_SHAPE_MAX_FIELD)) f.why = DH_FIT_INST_FIELD;
    if (!(as * radius <= DH_FIT_MAX_EXTENT)) f.why = DH_FIT_INST_EXTENT;
    // R must be near a rotation: |R x| <= 1.03 |x|
    for (int a = 2; a >= 0; --a)
        for (int b = 2; b >= a; --b) {
            const double g = ((double)in.R[3 * a] * (double)in.R[3 * b] + (double)in.R[3 * a + 1] * (double)in.R[3 * b + 1]) +
                             (double)in.R[3 * a + 2] * (double)in.R[3 * b + 2];
            const double d = g - (a == b ? 1.0 : 0.0);
            if (!((d < 0.0 ? -d : d) <= DH_FIT_R_TOLERANCE)) f = FitInstanceFault{DH_FIT_INST_NOT_ORTHONORMAL, a, b, g};
        }
    bool finite = sc - sc == 0.0;     // (x - x is 0.0 for a finite x alone)
    for (int q = 0; q < 9; ++q) { const double r = (double)in.R[q]; finite = finite && r - r == 0.0; }
    for (int q = 0; q < 3; ++q) { const double t = (double)in.t[q]; finite = finite && t - t == 0.0; }
    if (!finite) f = FitInstanceFault{DH_FIT_INST_NOT_FINITE, 0, 0, 0.0};
    return f;
}

// ---- carrying fitted poses across steps (k_fit_track.hip and k_fit's per-instance-schedule instance)
static_assert(sizeof(dh_fit_track_params) == 56, "dh_fit_track_params: 56 bytes");
static_assert(sizeof(dh_fit_track_state) == 76, "dh_fit_track_state: 76 bytes");
static_assert(sizeof(dh_fit_track_record) == 104, "dh_fit_track_record: 104 bytes");

// What a tracker's seed kernel (k_fit_track_seed for a camera, k_rig_fit_seed for a slot of a rig) decided: the start kind in
// the low byte, one numbering for both trackers, and above it the flags that are each tracker's own.
#define DH_FIT_SEED_NONE 0u           // nothing to fit and nothing tracked (the rig tracker: an unused slot, a record of zeros)
#define DH_FIT_SEED_DETECTED 1u       // a start from the forest's detection
#define DH_FIT_SEED_CARRIED 2u        // a start from the state
#define DH_FIT_SEED_ABSENT 3u         // the camera is absent / the rig has no present camera
#define DH_FIT_SEED_COAST 4u          // (the rig tracker) a tracked entry none of whose views is present
#define DH_FIT_SEED_VALID 0x100u      // (the camera tracker) the detection is valid
#define DH_FIT_TRACK_THREADS 64
// Whether the seed word gives the instance no start: the *_sched kernels then do no work for it.
__host__ __device__ inline bool dh_fit_seed_no_start(uint32_t seed) {
    const uint32_t kind = seed & 0xffu;
    return kind != DH_FIT_SEED_DETECTED && kind != DH_FIT_SEED_CARRIED;
}

// k_fit_sched: k_fit with each instance's (coarse, full) read from `sched` and no work for an instance without a start.
struct FitSchedArgs {
    FitArgs f;                    // coarse and full unused
    const uint32_t *sched;        // [n_inst][2]
    const uint32_t *seed;         // [n_inst] DH_FIT_SEED_*
};
hipError_t dh_launch_fit_sched(const FitSchedArgs &a, hipStream_t s);

struct FitTrackArgs {
    int n;                        // cameras
    uint32_t flags;               // DH_FIT_TRACK_*
    float scale;
    dh_fit_track_params prm;
    int64_t rms_lim;              // (int64)(rms_max * rms_max * 2^20), cast on the host
    double jump2;                 // max_jump * max_jump
    uint32_t coarse, full;        // the forest start's schedule
    const double *angles;         // [120][2] cos, sin
    const uint8_t *present;       // nullable [n]
    const dh_pose *poses;         // [n]
    const dh_support *support;    // [n]
    dh_fit_track_state *state;    // [n]
    dh_render_instance *start;    // [n] seed -> fit, update
    uint32_t *sched;              // [n][2]
    uint32_t *seed;               // [n]
    const dh_render_instance *fit_out;   // [n] fit -> update
    const dh_fit_record *fit_rec;        // [n]
    dh_fit_track_record *records;        // [n]
};
hipError_t dh_launch_fit_track_seed(const FitTrackArgs &a, hipStream_t s);
hipError_t dh_launch_fit_track_update(const FitTrackArgs &a, hipStream_t s);

// ---- adapting a model's shape to a subject (k_fit_shape.hip)
static_assert(sizeof(dh_shape_params) == 40, "dh_shape_params: 40 bytes");
static_assert(sizeof(dh_shape_record) == 88, "dh_shape_record: 88 bytes");

#define DH_SHAPE_THREADS 256
// The sums of one subject, S = 2^20 as in the fit.  Magnitude: the gate g <= 256 (DH_SHAPE_MAX_GATE) and |scale| * max |B_k[i]| <=
// 256 (DH_SHAPE_MAX_FIELD); with |R x| <= 1.03 |x| and |nrm| <= 1.05, |J_k| <= 1.05 * 1.03 * 256 < 277, and while |p| <= 2 p.z,
// |r| <= 1.05 * 2 * 256 < 538: J J < 2^17, J r < 2^18, r r < 2^19.  Times 2^20, times 2^23 point-instances of one subject
// (DH_SHAPE_MAX_TERMS): below 2^62 < 2^63.  The header says what holds outside that.
// The words: A_kl at DH_FIT_PAIR(8, k, l) (k <= l, rows of the 8 x 8 upper triangle whatever K is), b_k, e, count, used.
#define DH_SHAPE_B 36
#define DH_SHAPE_E 44
#define DH_SHAPE_COUNT 45
#define DH_SHAPE_USED 46
#define DH_SHAPE_SUMS 47
#define DH_SHAPE_STRIDE 48          // words of a subject's row

struct ShapeArgs {
    const uint16_t *frames;       // [n][h][w]
    int n, w, h;
    float k[9];                   // the one K of the batch (cams == NULL)
    const DhCam *cams;            // nullable [n]
    const float *pts, *nrm;       // the model: [np][3] each
    const float *basis;           // [nk][3][np]: one plane per field and axis, so a wave reads consecutive words
    uint32_t np, nk;
    double radius, largest;       // the model's largest |v|, the basis's largest |B_k[i]|
    const dh_render_instance *inst;   // [n_inst]
    const uint32_t *subjects;     // nullable [n_inst]
    uint32_t n_inst, n_subjects;
    uint32_t min_points;
    double gate;
    double lam1;                  // 1.0 + lambda (computed on the host: one f64 sum)
    unsigned long long *sums;     // [n_subjects][DH_SHAPE_STRIDE], cleared on the stream (k_shape_clear) before the launch
    dh_shape_record *rec;         // [n_subjects]
};
hipError_t dh_launch_shape_clear(const ShapeArgs &a, hipStream_t s);       // rows 0 .. n_subjects - 1 of a.sums
hipError_t dh_launch_shape_accumulate(const ShapeArgs &a, hipStream_t s);
hipError_t dh_launch_shape_solve(const ShapeArgs &a, hipStream_t s);

// ---- fitting one model to several views (k_fit_views.hip)
static_assert(sizeof(dh_view_instance) == 72, "dh_view_instance: 72 bytes");
static_assert(sizeof(dh_view_fit_record) == 32, "dh_view_fit_record: 32 bytes");
// DH_FIT_VIEW_TOLERANCE (the header: 0.001) and the magnitudes of the sums.  G = V V^T is symmetric and |G - I| <= e per element
// gives ||G - I||_2 <= 3 e (a row's absolute sum), so |V y|^2 = y^T V^T V y <= (1 + 3 e) |y|^2 (V^T V has G's eigenvalues), and
// the same for V^T.  With e_R = DH_FIT_R_TOLERANCE = 0.02: |R_w x| <= sqrt(1.06) |x| < 1.0296 |x| (the fit's 1.03); with e_V =
// 0.001: |V y| <= sqrt(1.003) |y| < 1.0015 |y|.  The composite R_v = V R_w (its nine elements rounded in f64: 1e-15 relative)
// therefore has |R_v x| <= 1.0296 * 1.0015 |x| < 1.032 |x|: THE ONE CONSTANT THAT CHANGES is 1.03 -> 1.032.  What the fit derives
// from it still holds with its own constants: |nrm| <= 1.032 * 1.01 < 1.043 <= 1.05; |q| = |R_v sv| <= 1.032 * 4096; |m| <= |q| |nrm|
// <= 1.032 * 1.043 * 4096 < 1.077 * 4096; the world row J = (V^T nrm, V^T m) has |J_a| <= 1.0015 * 1.077 * 4096 < 1.079 * 4096 <=
// 1.09 * 4096; and |r| <= 1.05 * (|p| / p.z) * gate per camera as before.  So while |p| <= 2 p.z in every view, J J <= (1.09 *
// 4096)^2 < 2^24.3, J r <= 1.09 * 4096 * 1.05 * 2 * 4096 < 2^25.2 and r r <= (1.05 * 2 * 4096)^2 < 2^26.2: every product below
// 2^27, times 2^20, times at most DH_FIT_MAX_POINTS = 2^15 (view, point) terms of an instance (refused above that): below 2^62.
// A tolerance of 0.02 for V as well would give 1.0296^2 = 1.06 |x| and 1.06 * 1.01 = 1.071 > 1.05 for |nrm|: hence a small one.
static_assert(DH_FIT_VIEW_TOLERANCE <= 0.001, "the magnitude argument above is made for a tolerance of at most 0.001");

// One camera of a dh_fit_views table: camera-space point = V x + u for a world point x.
struct FitView {
    float V[9];                   // row-major
    float u[3];                   // mm
};

struct FitViewsArgs {
    const uint16_t *frames;       // [n][h][w]: frame c is camera c's
    int n, w, h;
    const DhCam *cams;            // [n]
    const FitView *views;         // [n]
    const FitModel *models;
    const dh_view_instance *inst;
    uint32_t n_inst;
    uint32_t coarse, full, min_points;
    double gate[2];
    double lam1;                  // 1.0 + lambda (computed on the host: one f64 sum)
    dh_view_instance *out;        // [n_inst]
    dh_view_fit_record *rec;      // [n_inst]
};
hipError_t dh_launch_fit_views(const FitViewsArgs &a, hipStream_t s);

// ---- adapting a model's shape across views (k_fit_shape_views.hip)
// Magnitudes.  A view's terms are section 20's with the composite R_v = V R_w for R, and the section above gives |R_v x| <=
// 1.032 |x| for a view table within DH_FIT_VIEW_TOLERANCE and an R_w within DH_FIT_R_TOLERANCE: THE ONE CONSTANT THAT CHANGES
// is again 1.03 -> 1.032.  |nrm| <= 1.032 * 1.01 < 1.043 <= 1.05 as there, so |J_k| <= 1.05 * 1.032 * 256 < 278 < 2^9 and, while
// |p| <= 2 p.z in every view, |r| <= 1.05 * 2 * 256 < 538 < 2^10: J J < 2^17, J r < 2^18, r r < 2^19 as in section 20, every
// product below 2^19.  Times 2^20, times DH_SHAPE_MAX_TERMS = 2^23 terms of one subject -- which now counts its (view, point)
// pairs: the host form adds popcount(views) * points per instance, the _device form bounds the call by n_instances *
// min(64, n) * points -- below 2^62 < 2^63.

// The r-th set bit of `mask`, counted from bit 0 (r = 0: the lowest); 64 where the mask has r set bits or fewer.  Six halvings:
// the answer lies in the low half of the window when that half holds more than r set bits, else in the high half with r
// lowered by the low half's count.
__host__ __device__ inline uint32_t dh_shape_view_bit(uint64_t mask, uint32_t r) {
    uint32_t pos = 0;
    for (uint32_t width = 32; width; width >>= 1) {
        const uint32_t low = (uint32_t)__builtin_popcountll(mask & ((1ull << width) - 1ull));
        if (r >= low) { r -= low; mask >>= width; pos += width; }
    }
    return (mask & 1ull) != 0 && r == 0 ? pos : 64u;
}

// Why an instance of a multi-view shape step takes no part: DH_SHAPE_SKIP first (no refusal: the caller asked for it), then the
// per-instance refusals of the header in their order.  Stated once for the host loop (which turns the answer into its messages)
// and k_shape_accumulate_views (which skips the instance as a whole).  n: the view table's cameras; a NaN fails each test.
// An instance that passes names only cameras < n and a set < n_sets: no index formed from it leads out of a buffer.
enum { DH_SHAPE_VIEWS_OK = 0, DH_SHAPE_VIEWS_SKIPPED, DH_SHAPE_VIEWS_NO_VIEW, DH_SHAPE_VIEWS_CAMERA, DH_SHAPE_VIEWS_SET, DH_SHAPE_VIEWS_SUBJECT,
       DH_SHAPE_VIEWS_FAULT };
struct ShapeViewsSkip {
    int why;                      // DH_SHAPE_VIEWS_*
    uint64_t last;                // CAMERA: the camera the highest set bit names
    FitInstanceFault fault;       // FAULT: what dh_fit_instance_fault found
};
__host__ __device__ inline ShapeViewsSkip dh_shape_views_skip(const dh_view_instance &in, uint32_t set, uint32_t subject, uint32_t n, uint32_t n_sets,
                                                              uint32_t n_subjects, double radius, double largest) {
    ShapeViewsSkip s{DH_SHAPE_VIEWS_OK, 0, FitInstanceFault{DH_FIT_INST_OK, 0, 0, 0.0}};
    if (subject == DH_SHAPE_SKIP) { s.why = DH_SHAPE_VIEWS_SKIPPED; return s; }
    if (in.views == 0) { s.why = DH_SHAPE_VIEWS_NO_VIEW; return s; }
    s.last = (uint64_t)in.first_cam + (63u - (uint32_t)__builtin_clzll(in.views));
    if (s.last >= (uint64_t)n) { s.why = DH_SHAPE_VIEWS_CAMERA; return s; }
    if (set >= n_sets) { s.why = DH_SHAPE_VIEWS_SET; return s; }
    if (subject >= n_subjects) { s.why = DH_SHAPE_VIEWS_SUBJECT; return s; }
    s.fault = dh_fit_instance_fault(in, radius, largest);
    if (s.fault.why != DH_FIT_INST_OK) s.why = DH_SHAPE_VIEWS_FAULT;
    return s;
}

// k_shape_accumulate_views: one workgroup per (instance, view) pair of a grid of n_inst * ranks.  The clear and the solve of the
// call are section 20's, launched with `s`.
struct ShapeViewsArgs {
    ShapeArgs s;                  // frames [n_sets][n][h][w]; n: the view table's cameras; cams [n]; inst and k unused
    const FitView *views;         // [n]
    const dh_view_instance *inst; // [n_inst]
    const uint32_t *sets;         // nullable [n_inst]
    uint32_t n_sets;
    uint32_t ranks;               // min(64, n): the views an instance can have
};
hipError_t dh_launch_shape_accumulate_views(const ShapeViewsArgs &a, hipStream_t s);

// ---- calibrating a view table (k_calib_views.hip)
static_assert(sizeof(dh_calib_params) == 64, "dh_calib_params: 64 bytes");
static_assert(sizeof(dh_calib_record) == 120, "dh_calib_record: 120 bytes");
static_assert(DH_CALIB_SKIP == DH_SHAPE_SKIP, "take[i] is handed to dh_shape_views_skip as the subject");
// Magnitudes.  A pair's point pass is section 21's at the composite (R_v, t_v), so |p - t_v| = |R_v sv| <= 1.032 * 4096 < 4228 and
// |nrm| <= 1.05 as derived above.  A pair takes part only while |t_v[i] - g_c[i]| <= DH_CALIB_MAX_ARM = 2048 per component, so
// |t_v - g_c| <= 2048 sqrt(3) < 3548 and |q| = |p - g_c| <= 4228 + 3548 < 7776.  The cross product has |m| <= |q| |nrm| <= 1.05 *
// 7776 < 8165, and the rotation columns are m / DH_CALIB_ARM_UNIT: |J_3..5| < 8165 / 64 < 127.6 < 2^7; |J_0..2| <= 1.05.  The
// gate lies in (0, DH_SHAPE_MAX_GATE = 256], so while |p| <= 2 p.z, |r| <= 1.05 * 2 * 256 < 538.  Products: J J < 127.6^2 <
// 16282 < 2^14, J r < 127.6 * 538 < 68649 < 2^16.1, r r < 538^2 < 2^18.2: every one below section 20's 2^19.  Times 2^20, times
// DH_SHAPE_MAX_TERMS = 2^23 terms of one CAMERA -- the host form adds the model's points per pair that takes part, the _device
// form bounds the call by n_instances * points (an instance gives a camera at most one pair) -- below 2^62 < 2^63.  Without
// the arm unit |J_3..5| would reach 2^13 and J J 2^26: 2^23 terms would not fit.  Without the arm limit |q| is unbounded.
static_assert(DH_CALIB_ARM_UNIT == 64.0 && DH_CALIB_MAX_ARM == 2048.0 && DH_SHAPE_MAX_GATE <= 256.0, "the magnitude argument above");
#define DH_CALIB_THREADS 256
#define DH_CALIB_STRIDE 32            // words of a camera's row: the fit's 29 at their offsets, the pair count at DH_FIT_USED

// Why an (instance, view) pair of a calibration step takes no part, stated once for the host loop (which turns the whole-
// instance answers into its messages and counts the pairs that are left) and k_calib_accumulate (which skips).  The whole
// instance first: DH_CALIB_SKIP, then the per-instance refusals of the header in their order -- dh_shape_views_skip's with
// `take` for the subject, one subject and no basis (largest 0.0: the field test passes whenever the scale is finite).
__host__ __device__ inline ShapeViewsSkip dh_calib_skip(const dh_view_instance &in, uint32_t set, uint32_t take, uint32_t n, uint32_t n_sets, double radius) {
    return dh_shape_views_skip(in, set, take == DH_CALIB_SKIP ? DH_SHAPE_SKIP : 0u, n, n_sets, 1u, radius, 0.0);
}
// Then the pair, of an instance that passed: the composite camera pose of the view (section 21's expressions), the camera's
// pivot g_c, and whether the pair is left out -- the camera is held, or a component of t_v - g_c exceeds DH_CALIB_MAX_ARM (a NaN
// fails).  Neither is a refusal.
enum { DH_CALIB_PAIR_OK = 0, DH_CALIB_PAIR_HELD, DH_CALIB_PAIR_ARM };
struct CalibPair {
    int why;                      // DH_CALIB_PAIR_*
    double R[9], t[3];            // (R_v, t_v)
    double g[3];                  // g_c
};
// g_c alone (the solve needs it for a camera no pair names)
__host__ __device__ inline void dh_calib_pivot(const FitView &vw, const double o[3], double g[3]) {
    for (int i = 0; i < 3; ++i)
        g[i] = (((double)vw.V[3 * i] * o[0] + (double)vw.V[3 * i + 1] * o[1]) + (double)vw.V[3 * i + 2] * o[2]) + (double)vw.u[i];
}
__host__ __device__ inline CalibPair dh_calib_pair(const dh_view_instance &in, const FitView &vw, const double o[3], bool held) {
    CalibPair c;
    c.why = DH_CALIB_PAIR_OK;
    for (int i = 0; i < 3; ++i) {
        const double v0 = (double)vw.V[3 * i], v1 = (double)vw.V[3 * i + 1], v2 = (double)vw.V[3 * i + 2];
        for (int j = 0; j < 3; ++j) c.R[3 * i + j] = (v0 * (double)in.R[j] + v1 * (double)in.R[3 + j]) + v2 * (double)in.R[6 + j];
        c.t[i] = ((v0 * (double)in.t[0] + v1 * (double)in.t[1]) + v2 * (double)in.t[2]) + (double)vw.u[i];
    }
    dh_calib_pivot(vw, o, c.g);
    for (int i = 2; i >= 0; --i) {
        const double arm = c.t[i] - c.g[i];
        if (!((arm < 0.0 ? -arm : arm) <= DH_CALIB_MAX_ARM)) c.why = DH_CALIB_PAIR_ARM;
    }
    if (held) c.why = DH_CALIB_PAIR_HELD;
    return c;
}

struct CalibArgs {
    const uint16_t *frames;       // [n_sets][n][h][w]
    int n, w, h;                  // n: the view table's cameras
    const DhCam *cams;            // [n]
    const FitView *views;         // [n]
    const float *pts, *nrm;       // the model: [np][3] each
    uint32_t np;
    double radius;                // the model's largest |v|
    const dh_view_instance *inst; // [n_inst]
    const uint32_t *sets;         // nullable [n_inst]
    const uint32_t *take;         // nullable [n_inst]
    const uint8_t *hold;          // nullable [n]
    uint32_t n_inst, n_sets;
    uint32_t ranks;               // min(64, n): the views an instance can have
    uint32_t min_points;
    double gate;
    double lam1;                  // 1.0 + lambda (computed on the host: one f64 sum)
    double pivot[3];              // o
    unsigned long long *sums;     // [n][DH_CALIB_STRIDE], cleared on the stream (k_calib_clear) before the accumulation
    dh_calib_record *rec;         // [n]
};
hipError_t dh_launch_calib_clear(const CalibArgs &a, hipStream_t s);       // rows 0 .. n - 1 of a.sums
hipError_t dh_launch_calib_accumulate(const CalibArgs &a, hipStream_t s);  // one workgroup per (instance, view) pair: n_inst * ranks
hipError_t dh_launch_calib_solve(const CalibArgs &a, hipStream_t s);       // one lane per camera

// ---- carrying each rig person's fitted world pose across steps (k_rig_fit_track.hip and k_fit_views' per-instance-schedule
// instance).  The bind of a step is stated in dh_rig_fit.h.
// What k_rig_fit_seed decided for a slot: a DH_FIT_SEED_* kind in the low byte (ABSENT: the state is kept), and what the slot is.
#define DH_RIG_FIT_SEED_IS_SEEN 0x100u    // who[slot] is the slot's person
#define DH_RIG_FIT_SEED_IS_ENTRY 0x200u   // the slot is an entry of the state (else an unbound person)
#define DH_RIG_FIT_THREADS 64

// k_fit_views_sched: k_fit_views with each instance's (coarse, full) read from `sched` and no work for a slot without a start.
struct FitViewsSchedArgs {
    FitViewsArgs f;               // coarse and full unused
    const uint32_t *sched;        // [n_inst][2]
    const uint32_t *seed;         // [n_inst] DH_FIT_SEED_* | DH_RIG_FIT_SEED_*
    uint32_t group;               // slots of a group (a rig's DH_RIG_MAX_TRACKS); n_inst is a multiple of it
};
hipError_t dh_launch_fit_views_sched(const FitViewsSchedArgs &a, hipStream_t s);

struct RigFitArgs {
    int n_rigs, n_cams, max_heads;
    uint32_t flags;               // DH_FIT_TRACK_*
    float scale;
    dh_rig_fit_track_params prm;
    int64_t rms_lim;              // (int64)(rms_max * rms_max * 2^20), cast on the host
    double jump2;                 // max_jump * max_jump
    uint32_t coarse, full;        // the detected start's schedule
    const double *angles;         // [120][2] cos, sin
    const int32_t *rig_begin;     // [n_rigs + 1]
    const FitView *views;         // [n_cams]
    const uint8_t *present;       // nullable [n_cams]
    const uint32_t *n_heads;      // [n_cams]
    const dh_head *heads;         // [n_cams][max_heads]
    const uint32_t *n_persons;    // [n_rigs]
    const dh_rig_person *persons; // [n_rigs][DH_RIG_MAX_PERSONS]
    dh_rig_fit_state *state;      // [n_rigs][DH_RIG_MAX_TRACKS]
    dh_view_instance *start;      // [n_rigs][DH_RIG_MAX_TRACKS] seed -> fit, update
    uint32_t *sched;              // [slots][2]
    uint32_t *seed;               // [slots]
    uint32_t *who;                // [slots] the slot's person or DH_RIG_FIT_NO_PERSON
    const dh_view_instance *fit_out;     // [slots] fit -> update
    const dh_view_fit_record *fit_rec;   // [slots]
    dh_rig_fit_record *records;          // [slots]
};
hipError_t dh_launch_rig_fit_seed(const RigFitArgs &a, hipStream_t s);
hipError_t dh_launch_rig_fit_update(const RigFitArgs &a, hipStream_t s);

// ---- a shape per subject (k_subjects.hip)
#define DH_SUBJECTS_THREADS 256         // the points and normals kernels of a set (k_subjects.hip, k_surface.hip): one lane per vertex
static_assert(sizeof(dh_subject_state) == 80, "dh_subject_state: 80 bytes");
// Magnitudes.  A model of a set is v'_i = fl32(v_i + sum_k c_k B_k[i]) with |c_k| <= max_coeff (the clamp of the update and the
// refusal of dh_fit_subjects_set_coeffs: no other path writes a coefficient), so |v'_i| <= |v_i| + K max_coeff max |B_k[i]| <= the
// set's bound radius(base) + K * max_coeff * largest, up to the roundings: the K f64 products and sums (K * 2^-52 relative) and
// the one rounding to f32 (2^-24 relative per component).  Together below 1.2e-7 relative, which the fit's constant absorbs:
// section 21 derives |R x| <= 1.0296 |x| and the argument is made with 1.03, a margin of 3.9e-4.  The extent test of
// dh_fit_instance_fault with the BOUND for the radius therefore gives |scale| |v'| <= 4096 (1 + 1.2e-7) for every coefficient the
// device can reach, and sections 18 - 24 hold for a model of a set as they stand.
// The normals.  The points are f32 widened, so a difference of two is 0 or at least 2^-149 in magnitude, a product of two
// differences 0 or at least 2^-298 (and at most 2^258), and a face product and any sum of them 0 or a multiple of 2^-350: a
// component of the summed normal is exactly 0.0 or at least 2^-350, and at most 3 * 131072 * 2^259 < 2^278.  q = (n0 n0 + n1 n1)
// + n2 n2 is then exactly 0.0 or in [2^-700, 2^558]: never subnormal, never infinite, its relative error below 2^-51.  With a
// correctly rounded square root |n / ln| <= 1 + 2^-50 before the rounding to f32: a normal of a set has |nrm| <= 1 + 1e-7 <= 1.01,
// which is what dh_fit_model_create demands of a caller's, or it is (0, 0, 0): such a point has c = 0.0, fails `c < 0.0` and
// never reaches a sum.

// The set's bound on |v'| (f64, computed once at creation): radius(base) + (K * max_coeff) * largest.
inline double dh_subjects_radius_bound(double base_radius, uint32_t n_fields, double max_coeff, double largest) {
    return base_radius + ((double)n_fields * max_coeff) * largest;
}
// Each vertex's incident corners in ascending (triangle, corner) order: begin [n + 1] and corners [3 n_tris], corner t * 3 + c
// being corner c of triangle t.  A counting sort, so a vertex's run is ascending by construction.  false: an index >= n, and
// *bad_tri names the first triangle that holds one.
inline bool dh_subjects_corner_lists(const uint32_t *tris, uint32_t n_tris, uint32_t n, uint32_t *begin, uint32_t *corners, uint32_t *bad_tri) {
    for (uint32_t i = 0; i <= n; ++i) begin[i] = 0;
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) {
            const uint32_t v = tris[(size_t)t * 3 + c];
            if (v >= n) { if (bad_tri) *bad_tri = t; return false; }
            ++begin[v + 1];
        }
    for (uint32_t i = 0; i < n; ++i) begin[i + 1] += begin[i];
    for (uint32_t q = 0; q < 3 * n_tris; ++q) corners[begin[tris[q]]++] = q;     // ascending q: each run fills from its front,
    for (uint32_t i = n; i > 0; --i) begin[i] = begin[i - 1];                    // which leaves begin[v] at the run's end:
    begin[0] = 0;                                                                // the next vertex's beginning
    return true;
}
// The first vertex of the mesh pts [n][3] whose summed normal has length 0 (k_subjects_normals' arithmetic on the host: the gather
// over the corner list, q, one square root), or n where there is none.  What dh_fit_subjects_create refuses a base mesh by.
inline uint32_t dh_subjects_first_zero_normal(const float *pts, const uint32_t *tris, const uint32_t *begin, const uint32_t *corners, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        double s[3] = {0.0, 0.0, 0.0};
        for (uint32_t j = begin[i]; j < begin[i + 1]; ++j) {
            const uint32_t *tri = tris + (size_t)(corners[j] / 3u) * 3;
            const float *pa = pts + (size_t)tri[0] * 3, *pb = pts + (size_t)tri[1] * 3, *pc = pts + (size_t)tri[2] * 3;
            double u[3], w[3];
            for (int c = 0; c < 3; ++c) { u[c] = (double)pb[c] - (double)pa[c]; w[c] = (double)pc[c] - (double)pa[c]; }
            s[0] = s[0] + (u[1] * w[2] - u[2] * w[1]);
            s[1] = s[1] + (u[2] * w[0] - u[0] * w[2]);
            s[2] = s[2] + (u[0] * w[1] - u[1] * w[0]);
        }
        const double q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
        if (!(__builtin_sqrt(q) > 0.0)) return i;
    }
    return n;
}

// One model of a set as the update kernels write it.
struct SubjectModel {
    float *pts;                   // [n][3]
    float *nrm;                   // [n][3]
};
struct SubjectsArgs {
    const float *base;            // [n][3] the base mesh
    const float *basis;           // [nk][3][n]
    const uint32_t *tris;         // [n_tris][3]
    const uint32_t *corner_begin; // [n + 1]
    const uint32_t *corners;      // [3 n_tris]
    const SubjectModel *models;   // [S]
    dh_subject_state *state;      // [S]
    const dh_shape_record *rec;   // nullable [S]: NULL evaluates the coefficients as they are
    uint32_t n, nk;
    uint32_t first, count;        // the subjects that are applied and evaluated
    double max_coeff;
};
hipError_t dh_launch_subjects_update(const SubjectsArgs &a, hipStream_t s);       // k_subjects_apply, _points, _normals

// k_shape_accumulate_subjects: section 20's accumulation with the model of each instance's subject.
struct ShapeSubjectsArgs {
    ShapeArgs s;                  // pts and nrm unused; radius: the set's bound
    const SubjectModel *models;   // [S] (n_subjects <= S)
    const dh_fit_record *fit_rec; // nullable [n_inst]: an instance whose fit did not end DH_FIT_OK takes no part
};
hipError_t dh_launch_shape_accumulate_subjects(const ShapeSubjectsArgs &a, hipStream_t s);
// k_fit_carry: the R and t of a fit call's uploaded instances replaced by those of `carried` (device, [n_inst]) where they are
// finite and within DH_FIT_R_TOLERANCE of a rotation.
hipError_t dh_launch_fit_carry(dh_render_instance *inst, const dh_render_instance *carried, uint32_t n_inst, hipStream_t s);

// ---- a surface per subject (k_surface.hip)
static_assert(sizeof(dh_surface_params) == 64, "dh_surface_params: 64 bytes");
static_assert(sizeof(dh_surface_record) == 40, "dh_surface_record: 40 bytes");
// Magnitudes.  A model of a surface set is v'_i = fl32((v_i + sum_k c_k B_k[i]) + o_i nb_i) with |o_i| <= max_offset (the clamp of
// the solve and the refusal of dh_fit_subjects_set_offsets: no other path writes an offset) and |nb_i| <= 1 + 1e-7 <= 1.01 (the
// base normals are normals of section 25), so |v'_i| <= section 25's bound + 1.01 max_offset, up to three more f64 roundings
// (3 * 2^-52 relative) that the same margin absorbs: the extent test with this bound keeps sections 18 - 25 closed.
// The sums of a vertex, S = 2^20.  sb = nb * scale has |sb| <= 1.01 |scale|, w = R sb has |w| <= 1.03 * 1.01 |scale|, and with
// |nrm| <= 1.05, |J| <= 1.05 * 1.0403 |scale| < 1.1 |scale|.  |scale| is not bounded by the extent test alone (a small model may
// carry a large scale), so an instance takes part only while |scale| <= DH_SURFACE_MAX_SCALE = 64: |J| < 70.4.  The gate lies in
// (0, 256], so while |p| <= 2 p.z, |res| < 538 (section 20).  J J < 4957 < 2^12.3, J res < 37876 < 2^15.3; times 2^20, times the
// instances that can add to ONE vertex's words -- one term per instance, and a call has at most DH_SHAPE_MAX_TERMS = 2^23
// instances -- below 2^58.3 < 2^63.  The subject's e is section 20's word: res res < 2^18.2, times 2^20, times at most 2^23
// (instance, point) terms of one subject (the host forms count them per subject, the _device forms bound the call by
// n_instances * n): below 2^61.2.  cnt, points and instances count terms: below 2^23.
static_assert(DH_SURFACE_MAX_SCALE <= 64.0 && DH_SHAPE_MAX_GATE <= 256.0 && DH_SHAPE_MAX_TERMS <= 8388608u, "the magnitude argument above");
#define DH_SURFACE_NB_BOUND 1.01
#define DH_SURFACE_THREADS 256          // accumulate: one workgroup per instance
#define DH_SURFACE_SOLVE_THREADS 512    // solve: one workgroup per subject
// The words of a vertex's row, and of a subject's tally.  The solve reuses words A and B of a row for the two values of the
// vertex that no sweep changes (the numerator's constant part and the denominator), as f64 bit patterns: the sums are spent by then.
#define DH_SURFACE_A 0
#define DH_SURFACE_B 1
#define DH_SURFACE_CNT 2
#define DH_SURFACE_ROW 3
#define DH_SURFACE_E 0
#define DH_SURFACE_POINTS 1
#define DH_SURFACE_USED 2
#define DH_SURFACE_TALLY 4
// The solve keeps u and u' in LDS while two f64 arrays of n fit beside its 2 KB of counters in the 160 KB a workgroup may have on
// gfx950: 16 n <= 163840 - 2048.  Above that they lie in the set's scratch.
#define DH_SURFACE_LDS_POINTS 10112u
static_assert(16u * DH_SURFACE_LDS_POINTS + 2048u <= 163840u, "two f64 arrays and the counters in 160 KB");

// The set's bound on |v'| with offsets: section 25's bound + max_offset * 1.01.
inline double dh_surface_radius_bound(double base_radius, uint32_t n_fields, double max_coeff, double largest, double max_offset) {
    return dh_subjects_radius_bound(base_radius, n_fields, max_coeff, largest) + max_offset * DH_SURFACE_NB_BOUND;
}
// Each vertex's neighbours -- the unique vertices other than itself that share an edge of a triangle with it -- ascending, in CSR
// form: begin [n + 1] and list [begin[n]], at most 6 n_tris entries (`list` must hold that many).  Every triangle gives each of
// its corners the other two; a vertex's run is sorted and its duplicates and the vertex itself are dropped.  false: an index >= n,
// *bad_tri names the first triangle that holds one.  `work` is scratch of 6 n_tris words.
inline bool dh_subjects_neighbour_lists(const uint32_t *tris, uint32_t n_tris, uint32_t n, uint32_t *begin, uint32_t *list, uint32_t *work,
                                        uint32_t *bad_tri) {
    for (uint32_t i = 0; i <= n; ++i) begin[i] = 0;
    for (uint32_t t = 0; t < n_tris; ++t)
        for (int c = 0; c < 3; ++c) {
            const uint32_t v = tris[(size_t)t * 3 + c];
            if (v >= n) { if (bad_tri) *bad_tri = t; return false; }
            begin[v + 1] += 2;
        }
    for (uint32_t i = 0; i < n; ++i) begin[i + 1] += begin[i];
    for (uint32_t t = 0; t < n_tris; ++t)                                          // work: every vertex's raw run, begin[v] moving to its end
        for (int c = 0; c < 3; ++c) {
            const uint32_t v = tris[(size_t)t * 3 + c];
            work[begin[v]++] = tris[(size_t)t * 3 + (c + 1) % 3];
            work[begin[v]++] = tris[(size_t)t * 3 + (c + 2) % 3];
        }
    uint32_t out = 0, from = 0;
    for (uint32_t v = 0; v < n; ++v) {
        const uint32_t to = begin[v];                                              // the raw run is work[from .. to)
        for (uint32_t a = from + 1; a < to; ++a) {                                 // insertion sort: runs are short
            const uint32_t x = work[a];
            uint32_t b = a;
            for (; b > from && work[b - 1] > x; --b) work[b] = work[b - 1];
            work[b] = x;
        }
        begin[v] = out;
        for (uint32_t a = from; a < to; ++a)
            if (work[a] != v && (a == from || work[a] != work[a - 1])) list[out++] = work[a];
        from = to;
    }
    begin[n] = out;
    return true;
}

// k_subjects_points_surface: k_subjects_points' tree, then the offset along the base normal.
struct SurfacePointsArgs {
    SubjectsArgs a;
    const float *nb;              // [n][3] the base normals
    const double *offsets;        // [S][n]
};
struct SurfaceArgs {
    ShapeArgs s;                  // pts, nrm, basis, nk, lam1, sums and rec unused; np: the set's n; radius: the set's bound
    const SubjectModel *models;   // [S] (n_subjects <= S)
    const dh_fit_record *fit_rec; // nullable [n_inst]
    const float *nb;              // [n][3]
    const uint32_t *nbr_begin;    // [n + 1]
    const uint32_t *nbr;          // [nbr_begin[n]]
    double *offsets;              // [S][n]
    unsigned long long *rows;     // [S][n][DH_SURFACE_ROW]
    unsigned long long *tally;    // [S][DH_SURFACE_TALLY]
    double *scratch;              // [S][2][n]: u and u' of a model above DH_SURFACE_LDS_POINTS
    dh_subject_state *state;      // [S]: zero_normals back to 0 for the normals pass
    dh_surface_record *rec;       // [n_subjects]
    double min_cos2, mu, eps, max_offset;
    uint32_t min_count, iterations;
};
hipError_t dh_launch_surface_clear(const SurfaceArgs &a, hipStream_t s);       // the rows and tallies of subjects 0 .. n_subjects - 1
hipError_t dh_launch_surface_accumulate(const SurfaceArgs &a, hipStream_t s);  // one workgroup per instance
hipError_t dh_launch_surface_solve(const SurfaceArgs &a, hipStream_t s);       // one workgroup per subject
// Once per set, at its creation on the set's device: lets k_surface_solve take the dynamic LDS a model of n vertices needs, so that
// a step is its five launches and no other runtime call.
hipError_t dh_surface_solve_prepare(uint32_t n);
// k_subjects_apply where rec is given, then k_subjects_points_surface and k_subjects_normals, for subjects a.a.first .. + a.a.count - 1
hipError_t dh_launch_subjects_update_surface(const SurfacePointsArgs &a, bool apply, hipStream_t s);
// (k_subjects.hip) its kernels one by one, for the evaluation of a surface set
hipError_t dh_launch_subjects_apply(const SubjectsArgs &a, hipStream_t s);
hipError_t dh_launch_subjects_normals(const SubjectsArgs &a, hipStream_t s);

// ---- identifying the subject of a fitted head (k_ident.hip)
static_assert(sizeof(dh_ident_params) == 64, "dh_ident_params: 64 bytes");
static_assert(sizeof(dh_ident_record) == 40, "dh_ident_record: 40 bytes");
static_assert(DH_IDENT_UNKNOWN == DH_SHAPE_SKIP, "subjects_out is handed to a shape or surface step as its subjects");
// Magnitudes.  A pair's passes are section 18's at a model of the set, and the instance takes part only while |scale| * (the
// set's bound) <= DH_FIT_MAX_EXTENT: sections 25 and 26 show that this keeps section 18's argument closed for every model the
// set can hold.  The 29 words are the fit's as they stand.
#define DH_IDENT_THREADS 64             // k_ident_decide: one wave per instance

// The mean square of a score: two correctly rounded divisions.  points > 0.
__host__ __device__ inline double dh_ident_mean(int64_t sum_r2_fixed, uint32_t points) {
    return ((double)sum_r2_fixed / DH_FIT_S) / (double)points;
}
// Whether (m_a, a) precedes (m_b, b): the smaller mean square, a tie to the lower index.  (a NaN precedes nothing and nothing
// precedes it; an eligible m is finite)
__host__ __device__ inline bool dh_ident_precedes(double m_a, uint32_t a, double m_b, uint32_t b) {
    return m_a < m_b || (m_a == m_b && a < b);
}
// The status of an instance that takes part, from |E|, the best and second mean squares and the limits (max_ms = max_rms *
// max_rms, formed on the host); m_second is read only where eligible > 1.
__host__ __device__ inline uint32_t dh_ident_status(uint32_t eligible, double m_best, double m_second, double max_ms, double min_ratio) {
    if (eligible == 0) return DH_IDENT_NO_CANDIDATE;
    if (!(m_best <= max_ms)) return DH_IDENT_FAR;
    if (eligible > 1 && !(m_second >= min_ratio * m_best)) return DH_IDENT_AMBIGUOUS;
    return DH_IDENT_OK;
}
// The best and the second of the candidates seen so far: (+inf, DH_IDENT_UNKNOWN) where there is none, which every eligible
// candidate precedes.  add: one more candidate; merge: the picks of two disjoint sets of candidates (the decide wave's shuffle
// reduction).  Both keep best before second under dh_ident_precedes.
struct IdentPick {
    double m_best, m_second;
    uint32_t best, second;
};
__host__ __device__ inline IdentPick dh_ident_pick_none() {
    return IdentPick{__builtin_huge_val(), __builtin_huge_val(), DH_IDENT_UNKNOWN, DH_IDENT_UNKNOWN};
}
__host__ __device__ inline void dh_ident_pick_add(IdentPick &p, double m, uint32_t s) {
    if (dh_ident_precedes(m, s, p.m_best, p.best)) { p.m_second = p.m_best; p.second = p.best; p.m_best = m; p.best = s; }
    else if (dh_ident_precedes(m, s, p.m_second, p.second)) { p.m_second = m; p.second = s; }
}
__host__ __device__ inline void dh_ident_pick_merge(IdentPick &p, const IdentPick &o) {
    if (dh_ident_precedes(o.m_best, o.best, p.m_best, p.best)) {          // the other's best wins: the second is the better of my best and its second
        if (dh_ident_precedes(o.m_second, o.second, p.m_best, p.best)) { p.m_second = o.m_second; p.second = o.second; }
        else { p.m_second = p.m_best; p.second = p.best; }
        p.m_best = o.m_best; p.best = o.best;
    } else if (dh_ident_precedes(o.m_best, o.best, p.m_second, p.second)) { p.m_second = o.m_best; p.second = o.best; }
}

struct IdentArgs {
    FitArgs f;                    // frames, n, w, h, k, cams, inst, n_inst; coarse 0, full = iterations, both gates = gate, lam1, min_points; models, out and rec unused
    const SubjectModel *models;   // [S] (n_subjects <= S)
    uint32_t np, n_subjects;      // the set's points; the candidates' range
    double radius, largest;       // the set's bound, the basis's largest |B_k[i]|
    const uint8_t *enrolled;      // nullable [n_subjects]
    const dh_fit_record *fit_rec; // nullable [n_inst]
    dh_fit_record *score;         // [n_inst][n_subjects]: the caller's `scores` or the fitter's scratch
    float *pose;                  // [n_inst][n_subjects][12]: R then t of each pair's refit (the fitter's scratch)
    double max_ms, min_ratio;     // max_rms * max_rms (one f64 product on the host), min_ratio
    uint32_t *subjects_out;       // [n_inst]
    dh_ident_record *rec;         // [n_inst]
    dh_render_instance *poses_out;// nullable [n_inst]
};
hipError_t dh_launch_ident_score(const IdentArgs &a, hipStream_t s);       // one workgroup per pair, the subject the fast index
hipError_t dh_launch_ident_decide(const IdentArgs &a, hipStream_t s);      // one wave per instance

// ---- identifying enrolled subjects across the views of a rig (k_ident_views.hip)
// Magnitudes.  A pair's passes are section 21's at a model of the set: the extent test with the set's bound keeps |scale| |v'| <=
// 4096 for every model the set can hold (sections 25 and 26), the view table is within DH_FIT_VIEW_TOLERANCE by construction, and
// an instance takes part only while popcount(views) * (the set's points) <= DH_FIT_MAX_POINTS: section 21's 2^62 stands.  The
// decision reads scores and is section 27's functions above as they are.

// Why an instance of a multi-view identification takes no part, the header's six tests in their order, stated once for the
// host loop (which refuses what is no SKIP of the fit record) and for both kernels (which skip the instance as a whole).  Tests
// 1 - 3 and 5 are dh_shape_views_skip's with subject 0 of 1: it makes 5 after 3, and the fit record's test is put between them
// here.  fit_rec: the instance's own record, or NULL; np: the set's points; a NaN fails each test.  An instance that passes names
// only cameras < n and a set < n_sets, and sums at most DH_FIT_MAX_POINTS (view, point) terms.
enum { DH_IDENT_VIEWS_OK = 0, DH_IDENT_VIEWS_WHERE, DH_IDENT_VIEWS_RECORD, DH_IDENT_VIEWS_FAULT, DH_IDENT_VIEWS_TERMS };
struct IdentViewsPart {
    int why;                      // DH_IDENT_VIEWS_*
    ShapeViewsSkip skip;          // WHERE (no view, a camera >= n, a set >= n_sets) and FAULT: what dh_shape_views_skip found
    uint64_t terms;               // TERMS: popcount(views) * np
};
__host__ __device__ inline IdentViewsPart dh_ident_views_part(const dh_view_instance &in, uint32_t set, const dh_view_fit_record *fit_rec, uint32_t n,
                                                              uint32_t n_sets, uint32_t np, double radius, double largest) {
    IdentViewsPart p{DH_IDENT_VIEWS_OK, dh_shape_views_skip(in, set, 0u, n, n_sets, 1u, radius, largest), 0};
    p.terms = (uint64_t)__builtin_popcountll(in.views) * np;
    if (p.skip.why != DH_SHAPE_VIEWS_OK && p.skip.why != DH_SHAPE_VIEWS_FAULT) p.why = DH_IDENT_VIEWS_WHERE;
    else if (fit_rec && fit_rec->status != DH_FIT_OK) p.why = DH_IDENT_VIEWS_RECORD;
    else if (p.skip.why == DH_SHAPE_VIEWS_FAULT) p.why = DH_IDENT_VIEWS_FAULT;
    else if (p.terms > DH_FIT_MAX_POINTS) p.why = DH_IDENT_VIEWS_TERMS;
    return p;
}

struct IdentViewsArgs {
    FitViewsArgs f;               // frames [n_sets][n][h][w], n, w, h, cams, views, inst, n_inst; coarse 0, full = iterations, both gates = gate, lam1, min_points; models, out and rec unused
    const SubjectModel *models;   // [S] (n_subjects <= S)
    uint32_t np, n_subjects;      // the set's points; the candidates' range
    double radius, largest;       // the set's bound, the basis's largest |B_k[i]|
    const uint32_t *sets;         // nullable [n_inst]
    uint32_t n_sets;
    const uint8_t *enrolled;      // nullable [n_subjects]
    const dh_view_fit_record *fit_rec;   // nullable [n_inst]
    dh_view_fit_record *score;    // [n_inst][n_subjects]: the caller's `scores` or the fitter's scratch
    float *pose;                  // [n_inst][n_subjects][12]: R then t of each pair's refit (the fitter's scratch, section 27's)
    double max_ms, min_ratio;     // max_rms * max_rms (one f64 product on the host), min_ratio
    uint32_t *subjects_out;       // [n_inst]
    dh_ident_record *rec;         // [n_inst]
    dh_view_instance *poses_out;  // nullable [n_inst]
};
hipError_t dh_launch_ident_views_score(const IdentViewsArgs &a, hipStream_t s);    // one workgroup per pair, the subject the fast index
hipError_t dh_launch_ident_views_decide(const IdentViewsArgs &a, hipStream_t s);   // one wave per instance

// ---- following each tracked head with its own subject's model (k_subject_track.hip)
static_assert(sizeof(dh_subject_track_params) == 24, "dh_subject_track_params: 24 bytes");
static_assert(sizeof(dh_subject_track_state) == 92, "dh_subject_track_state: 92 bytes");
static_assert(sizeof(dh_subject_track_record) == 160, "dh_subject_track_record: 160 bytes");
// Magnitudes.  The step's fit is section 18's over a table whose entries are the set's models and the generic one: creation
// refuses a scale whose product with the set's bound or with the generic radius exceeds DH_FIT_MAX_EXTENT, so every start
// instance passes the extent test for whichever entry it names.  A wanted pair is section 27's as it stands.

// The four words of a binding (the tail of dh_subject_track_state and of dh_rig_subject_state), and the two places of the rule that
// change them, stated once for k_subject_track.hip, k_rig_subject_track.hip and tests/host/subject_bind_check.cpp.
struct SubjectBinding {
    uint32_t subject, wait, tries, bound_age;
};
__host__ __device__ inline uint32_t dh_sat_inc(uint32_t v) { return v == 0xffffffffu ? v : v + 1u; }
__host__ __device__ inline void dh_subject_unbind(uint32_t &subject, uint32_t &wait, uint32_t &tries, uint32_t &bound_age) {
    subject = DH_IDENT_UNKNOWN; wait = 0; tries = 0; bound_age = 0;
}
// THE BINDING LIFECYCLE (rule 2) of one camera or entry on the state the fit's outcome left: tracked, and whether this step's fit
// was accepted.  true: the camera or entry wants identification in this step.
__host__ __device__ inline bool dh_subject_lifecycle(bool tracked, bool accepted, uint32_t max_tries, uint32_t &subject, uint32_t &wait,
                                                     uint32_t &tries, uint32_t &bound_age) {
    if (!tracked) { dh_subject_unbind(subject, wait, tries, bound_age); return false; }
    if (!accepted) return false;
    if (subject != DH_IDENT_UNKNOWN) { bound_age = dh_sat_inc(bound_age); return false; }
    if (wait == 0 && (max_tries == 0 || tries < max_tries)) return true;
    if (wait > 0) wait -= 1;
    return false;
}
// What an identification that ran makes of the words (rule 3): DH_IDENT_OK binds `best`, any other status counts a try and waits.
__host__ __device__ inline void dh_subject_bind_or_retry(uint32_t status, uint32_t best, uint32_t retry, uint32_t &subject, uint32_t &wait,
                                                         uint32_t &tries, uint32_t &bound_age) {
    if (status == DH_IDENT_OK) { subject = best; bound_age = 0; }
    else { tries = dh_sat_inc(tries); wait = retry; }
}

// One step's four launches beside k_fit_sched share one block: section 19's (its state and records unused: the state here is
// 92 bytes a camera, the record 160), section 27's (inst and fit_rec: the step's fitted instances and their records, n_inst the
// cameras; score and pose: the tracker's scratch of cameras * S pairs; subjects_out, rec and poses_out unused) and the tracker's own.
struct SubjectTrackArgs {
    FitTrackArgs a;
    IdentArgs q;                  // q.enrolled is never NULL here: the tracker holds a mask of ones for "all"
    dh_subject_track_state *state;       // [n]
    dh_subject_track_record *records;    // [n]
    uint32_t retry, max_tries;
    uint32_t *want;               // [n] the cameras that want identification, in no particular order
    uint32_t *n_want;             // [1] how many: cleared by the seed kernel, grown by the update kernel
    uint32_t *wants;              // [n] 0 or 1 per camera: what the list holds, indexed by camera
    uint32_t grid;                // workgroups of the score kernel, fixed at creation
};
hipError_t dh_launch_subject_track_seed(const SubjectTrackArgs &g, hipStream_t s);     // one lane per camera
hipError_t dh_launch_subject_track_update(const SubjectTrackArgs &g, hipStream_t s);   // one lane per camera
hipError_t dh_launch_subject_track_score(const SubjectTrackArgs &g, hipStream_t s);    // g.grid workgroups over the list's pairs
hipError_t dh_launch_subject_track_bind(const SubjectTrackArgs &g, hipStream_t s);     // one wave per camera

// ---- following each rig person with its own subject's model (k_rig_subject_track.hip)
static_assert(sizeof(dh_rig_subject_state) == 104, "dh_rig_subject_state: 104 bytes");
static_assert(sizeof(dh_rig_subject_record) == 184, "dh_rig_subject_record: 184 bytes");
static_assert(sizeof(SubjectBinding) == 16, "the four words of an entry, beside its dh_rig_fit_state");
// Magnitudes.  The step's fit is section 21's over a table whose entries are the set's models and the generic one: creation
// refuses a scale whose product with the set's bound or with the generic radius exceeds DH_FIT_MAX_EXTENT, and (cameras of the
// largest rig) * points above DH_FIT_MAX_POINTS, so every start and every wanted pair sums below section 21's 2^62 for whichever
// entry it names and whichever mask it holds.  A wanted pair is section 28's as it stands.

// The state of an entry lives in two device arrays -- section 22's dh_rig_fit_state, on which dh_rig_fit_bind and the shared
// pieces of dh_fit_device.h run as they are, and the SubjectBinding beside it; dh_rig_subject_fit_tracker_state interleaves them.
// One step's four launches beside k_fit_views_sched share one block: section 22's (its records unused: the record here is 184
// bytes a slot), section 28's (inst and fit_rec: the step's fitted instances and their records, n_inst the slots, sets NULL and
// n_sets 1; score and pose: the tracker's scratch of slots * S pairs; subjects_out, rec and poses_out unused) and the tracker's own.
struct RigSubjectArgs {
    RigFitArgs a;
    IdentViewsArgs q;             // q.enrolled is never NULL here: the tracker holds a mask of ones for "all"
    SubjectBinding *bound;        // [slots]
    dh_rig_subject_record *records;      // [slots]
    uint32_t retry, max_tries;
    uint32_t *want;               // [slots] the slots that want identification, in no particular order
    uint32_t *n_want;             // [1] how many: cleared by the seed kernel, grown by the update kernel
    uint32_t *wants;              // [slots] 0 or 1 per slot: what the list holds, indexed by slot
    uint32_t grid;                // workgroups of the score kernel, fixed at creation
};
hipError_t dh_launch_rig_subject_seed(const RigSubjectArgs &g, hipStream_t s);     // one workgroup per rig
hipError_t dh_launch_rig_subject_update(const RigSubjectArgs &g, hipStream_t s);   // one lane per slot
hipError_t dh_launch_rig_subject_score(const RigSubjectArgs &g, hipStream_t s);    // g.grid workgroups over the list's pairs
hipError_t dh_launch_rig_subject_bind(const RigSubjectArgs &g, hipStream_t s);     // one wave per slot
// dh_rig_subject_fit_tracker_bind: the entry of `rig` that holds `id` (none: nothing) gets (subject, 0, 0, 0); one wave.
hipError_t dh_launch_rig_subject_set(const dh_rig_fit_state *state, SubjectBinding *bound, int rig, uint32_t id, uint32_t subject, hipStream_t s);
