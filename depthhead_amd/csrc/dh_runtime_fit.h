// dh_runtime_fit.h -- what the fit family's unit (dh_api_fit.hip) and the fit trackers' (dh_api_fit_track.hip) both use: the model
// and view-table handles, and the check and the argument half of a call's dh_fit_params.  Everything is static, as in dh_runtime.h.
// Not part of the ABI; only those two units include it.
#pragma once
#include "dh_runtime.h"
#include "dh_fit.h"

// A model: points and unit normals on one device, immutable.
struct dh_fit_model {
    int device = 0;
    uint32_t n = 0;
    double radius = 0.0;          // the largest |v|
    Buf<float> pts, nrm;
};

static int fit_params_default_(dh_fit_params *p) {
    if (!p) return fail(DH_EINVAL, "dh_fit_params_default: NULL argument");
    memset(p, 0, sizeof *p);
    p->coarse_iterations = 6; p->iterations = 14;
    p->gate[0] = 120.0; p->gate[1] = 25.0;
    p->lambda = 1e-3;
    p->min_points = 16;
    return DH_OK;
}

// The refusals of a call's dh_fit_params (NULL: the defaults); *out is what the call runs with.
static int fit_params_check(const dh_fit_params *in, dh_fit_params *out, const char *who) {
    dh_fit_params prm;
    (void)fit_params_default_(&prm);
    if (in) prm = *in;
    if ((uint64_t)prm.coarse_iterations + prm.iterations > 64)
        return fail(DH_EINVAL, "%s: coarse_iterations %u + iterations %u above 64", who, prm.coarse_iterations, prm.iterations);
    for (int g = 0; g < 2; ++g)
        if (!(prm.gate[g] > 0.0 && prm.gate[g] <= 4096.0)) return fail(DH_EINVAL, "%s: gate[%d] = %g outside (0, 4096]", who, g, prm.gate[g]);
    if (!(prm.lambda >= 0.0) || !std::isfinite(prm.lambda)) return fail(DH_EINVAL, "%s: lambda %g, expected a finite value >= 0", who, prm.lambda);
    if (prm.min_points < 6) return fail(DH_EINVAL, "%s: min_points %u below 6", who, prm.min_points);
    if (prm.reserved0 || prm.reserved[0] || prm.reserved[1]) return fail(DH_EINVAL, "%s: a reserved word of the params is not 0", who);
    *out = prm;
    return DH_OK;
}
// The half of a FitArgs or FitViewsArgs that the (checked) params fill.
template <typename A>
static void fit_args_params(A &a, const dh_fit_params &prm) {
    a.coarse = prm.coarse_iterations; a.full = prm.iterations; a.min_points = prm.min_points;
    a.gate[0] = prm.gate[0]; a.gate[1] = prm.gate[1];
    a.lam1 = 1.0 + prm.lambda;
}

// A view table: one world-to-camera transform per camera of a camera table, on that table's device, immutable.
struct dh_fit_views {
    int device = 0;
    int n = 0;
    const dh_cameras *cams = nullptr;        // the table it is bound to (which outlives it)
    Buf<FitView> dev;
};

// What the subject fit tracker (dh_api_fit_track.hip) reads of a subject set and of an identify call's
// params, defined in dh_api_fit.hip beside the set and the check they belong to (dh_host.h's names for internal symbols).
struct dh_fit_subjects;
struct SubjectsView {
    int device;
    uint32_t n, n_subjects;       // the points of a model, S
    double radius, largest;       // the set's bound on |v'|, the basis's largest |B_k[i]|
    const SubjectModel *table;    // device, [S]: what the identify kernels read
};
// *v, and where `models` is given (host, [S]) each model's device pointers as an entry of a fit's model table.
void dh_fit_subjects_view_(const dh_fit_subjects *set, SubjectsView *v, FitModel *models);
// ident_params_check with section 27's default max_rms.
int dh_ident_params_check_(const dh_ident_params *in, dh_ident_params *out, const char *who);
// the same with section 28's default max_rms (the rig subject fit tracker's)
int dh_ident_views_params_check_(const dh_ident_params *in, dh_ident_params *out, const char *who);
