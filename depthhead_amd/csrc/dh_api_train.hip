// dh_api_train.hip -- the trainer's runtime (HoughLearning): the sample pool on the device and the device half of tree growing;
// dh_train.cpp is the host half, k_train.hip the kernels.
#include "dh_runtime.h"

// ------------------------------------------------------------------ trainer (HoughLearning, prediction.rs:103-234)
// The pool of samples lives on the device (rectangle-sum images, labels, truth) with a host copy of the truth, which the
// host half of tree growing (dh_train.cpp) reads.  Calls are synchronous on the trainer's own stream.
struct dh_trainer {
    int device = 0;
    dh_train_params p{};
    TrainGeom g;                       // rectangle size and sample image size (frame-independent)
    hipStream_t s = nullptr;
    uint64_t frames = 0;
    size_t pool = 0, cap = 0;
    Buf<uint32_t> box;                 // [cap][bh][bw]
    Buf<uint8_t> lab;
    Buf<float> off;
    Buf<double> rot;
    std::vector<uint8_t> h_lab;
    std::vector<float> h_off;
    std::vector<double> h_rot;
    uint64_t neg_det = 0;
    std::vector<TrainLevelStat> stats;   // of the last fit
};

static int trainer_destroy_(dh_trainer *t) {
    if (!t) return DH_OK;
    DeviceGuard guard(t->device);
    if (t->s) (void)hipStreamDestroy(t->s);
    delete t;
    return DH_OK;
}

static int trainer_create_(const dh_train_params *prm, int device, dh_trainer **out) {
    if (!out) return fail(DH_EINVAL, "dh_trainer_create: NULL argument");
    *out = nullptr;
    TRY(dh_train_validate_(prm));
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(DH_EINVAL, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    std::unique_ptr<dh_trainer> t(new dh_trainer);
    t->device = device;
    t->p = *prm;
    TRY(dh_train_geom_(t->p, (int)prm->subimage_width, (int)prm->subimage_height, t->g));
    TRY(hip_step(hipStreamCreateWithFlags(&t->s, hipStreamNonBlocking), "hipStreamCreate"));
    *out = t.release();
    return DH_OK;
}

// Capacity for `need` samples; the resident ones are kept.
template <typename T>
static int train_grow(Buf<T> &b, size_t old_elems, size_t new_elems, hipStream_t s) {
    Buf<T> nb;
    TRY(nb.alloc(new_elems));
    if (old_elems) HIP_TRY(hipMemcpyAsync(nb.get(), b.get(), old_elems * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    b = std::move(nb);
    return DH_OK;
}
static int trainer_reserve(dh_trainer *t, size_t need) {
    if (need <= t->cap) return DH_OK;
    const size_t cap = std::max(need, t->cap * 2 + 1024), st = (size_t)t->g.bw * t->g.bh;
    TRY(train_grow(t->box, t->pool * st, cap * st, t->s));
    TRY(train_grow(t->lab, t->pool, cap, t->s));
    TRY(train_grow(t->off, t->pool * 3, cap * 3, t->s));
    TRY(train_grow(t->rot, t->pool * 3, cap * 3, t->s));
    t->cap = cap;
    return DH_OK;
}

static int trainer_add_frames_(dh_trainer *t, const uint16_t *frames, const uint8_t *masks, int n, int w, int h, const float *K,
                               const float *pos3d, const float *rot_deg) {
    if (!t) return fail(DH_EINVAL, "dh_trainer_add_frames: NULL trainer");
    if (n < 0) return fail(DH_EINVAL, "negative frame count");
    if (n == 0) return DH_OK;
    if (!frames || !masks || !K || !pos3d || !rot_deg) return fail(DH_EINVAL, "dh_trainer_add_frames: NULL argument");
    TrainGeom g;
    TRY(dh_train_geom_(t->p, w, h, g));
    TRY(dh_train_check_rotations_(rot_deg, n));
    if ((uint64_t)g.nx * g.ny > 0xffffffffull) return fail(DH_ESIZE, "too many windows per frame");
    DeviceGuard guard(t->device);
    if (!guard.ok) return DH_EHIP;
    const int chunk = std::min(n, dh_train_chunk_frames_(w, h));
    const size_t px = (size_t)w * h, spx = (size_t)(w + 1) * (h + 1);
    Buf<uint16_t> d_frames;
    Buf<uint8_t> d_masks;
    Buf<uint32_t> d_sat, d_sel, d_cnt;
    Buf<float> d_kinv, d_pos, d_rot;
    Buf<uint4> d_list;
    TRY(d_frames.alloc(chunk * px));
    TRY(d_masks.alloc(chunk * px));
    TRY(d_sat.alloc(chunk * spx));
    TRY(d_sel.alloc((size_t)chunk * 2 * DH_TRAIN_KEEP));
    TRY(d_cnt.alloc((size_t)chunk * 2));
    TRY(d_kinv.alloc((size_t)chunk * 9));
    TRY(d_pos.alloc((size_t)chunk * 3));
    TRY(d_rot.alloc((size_t)chunk * 3));
    TRY(d_list.alloc((size_t)chunk * 2 * DH_TRAIN_KEEP));
    std::vector<float> kinv((size_t)chunk * 9);
    std::vector<uint32_t> sel((size_t)chunk * 2 * DH_TRAIN_KEEP), cnt((size_t)chunk * 2);
    std::vector<uint4> list;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        for (int i = 0; i < m; ++i) dh_mat3_inv_f32_(K + (size_t)(c0 + i) * 9, &kinv[(size_t)i * 9]);   // IntrinsicMatrix::inv (types.rs:436-441)
        HIP_TRY(hipMemcpyAsync(d_frames.get(), frames + c0 * px, m * px * 2, hipMemcpyHostToDevice, t->s));
        HIP_TRY(hipMemcpyAsync(d_masks.get(), masks + c0 * px, m * px, hipMemcpyHostToDevice, t->s));
        HIP_TRY(hipMemcpyAsync(d_kinv.get(), kinv.data(), (size_t)m * 36, hipMemcpyHostToDevice, t->s));
        HIP_TRY(hipMemcpyAsync(d_pos.get(), pos3d + (size_t)c0 * 3, (size_t)m * 12, hipMemcpyHostToDevice, t->s));
        HIP_TRY(hipMemcpyAsync(d_rot.get(), rot_deg + (size_t)c0 * 3, (size_t)m * 12, hipMemcpyHostToDevice, t->s));
        TrainWinArgs wa{};
        wa.frames = d_frames.get(); wa.masks = d_masks.get(); wa.sat = d_sat.get();
        wa.n = m; wa.w = w; wa.h = h;
        wa.W = t->p.subimage_width; wa.H = t->p.subimage_height; wa.step = t->p.stepwidth;
        wa.lw = g.lw; wa.lh = g.lh; wa.nx = g.nx; wa.ny = g.ny;
        wa.seed = t->p.seed; wa.frame0 = t->frames;
        wa.sel = d_sel.get(); wa.cnt = d_cnt.get();
        TRY(hip_step(dh_launch_train_windows(wa, t->s), "k_train_select"));
        HIP_TRY(hipMemcpyAsync(sel.data(), d_sel.get(), sel.size() * 4, hipMemcpyDeviceToHost, t->s));
        HIP_TRY(hipMemcpyAsync(cnt.data(), d_cnt.get(), cnt.size() * 4, hipMemcpyDeviceToHost, t->s));
        HIP_TRY(hipStreamSynchronize(t->s));
        // pool order: frame after frame, each frame's negatives before its positives (prediction.rs:212-215)
        list.clear();
        for (int i = 0; i < m; ++i) {
            const uint32_t k = cnt[(size_t)i * 2] + cnt[(size_t)i * 2 + 1];
            for (uint32_t j = 0; j < k; ++j)
                list.push_back(make_uint4((uint32_t)i, sel[(size_t)i * 2 * DH_TRAIN_KEEP + j], (uint32_t)(t->pool + list.size()), 0u));
        }
        TRY(trainer_reserve(t, t->pool + list.size()));
        if (!list.empty()) {
            HIP_TRY(hipMemcpyAsync(d_list.get(), list.data(), list.size() * sizeof(uint4), hipMemcpyHostToDevice, t->s));
            TrainExtractArgs ea{};
            ea.frames = d_frames.get(); ea.masks = d_masks.get(); ea.sat = d_sat.get();
            ea.w = w; ea.h = h;
            ea.W = wa.W; ea.H = wa.H; ea.step = wa.step; ea.lw = g.lw; ea.lh = g.lh; ea.nx = g.nx;
            ea.rw = g.rw; ea.rh = g.rh; ea.bw = g.bw; ea.bh = g.bh;
            ea.list = d_list.get(); ea.n_list = (uint32_t)list.size();
            ea.kinv = d_kinv.get(); ea.pos3d = d_pos.get(); ea.rot_deg = d_rot.get();
            ea.box = t->box.get(); ea.lab = t->lab.get(); ea.off = t->off.get(); ea.rot = t->rot.get();
            TRY(hip_step(dh_launch_train_extract(ea, t->s), "k_train_extract"));
            const size_t k = list.size(), b = t->pool;
            t->h_lab.resize(b + k);
            t->h_off.resize((b + k) * 3);
            t->h_rot.resize((b + k) * 3);
            HIP_TRY(hipMemcpyAsync(t->h_lab.data() + b, t->lab.get() + b, k, hipMemcpyDeviceToHost, t->s));
            HIP_TRY(hipMemcpyAsync(t->h_off.data() + b * 3, t->off.get() + b * 3, k * 12, hipMemcpyDeviceToHost, t->s));
            HIP_TRY(hipMemcpyAsync(t->h_rot.data() + b * 3, t->rot.get() + b * 3, k * 24, hipMemcpyDeviceToHost, t->s));
            HIP_TRY(hipStreamSynchronize(t->s));
            t->pool += k;
        }
        t->frames += (uint64_t)m;
    }
    return DH_OK;
}

// stamm's tree growing, breadth-first over every tree at once (PARITY UNPINNED): per level the host
// applies early_stop, the device scores every (node, candidate) pair and picks each node's best split and the samples'
// sides, the host partitions stably and records leaves.
static int trainer_fit_(dh_trainer *t, dh_forest **out) {
    if (!t || !out) return fail(DH_EINVAL, "dh_trainer_fit: NULL argument");
    *out = nullptr;
    if (t->pool == 0) return fail(DH_ESTATE, "dh_trainer_fit: no samples (add frames with a non-background window first)");
    if ((uint64_t)t->p.n_trees * t->p.subset_per_tree > 0xffffffffull) return fail(DH_ESIZE, "n_trees * subset_per_tree above 2^32");
    DeviceGuard guard(t->device);
    if (!guard.ok) return DH_EHIP;
    TrainGrower gr(t->p, t->h_lab.data(), t->h_off.data(), t->h_rot.data(), t->pool);
    std::vector<uint32_t> idx, nidx;
    std::vector<TrainNode> level, split, next;
    std::vector<TrainBest> best;
    std::vector<uint8_t> side;
    gr.roots(idx, level);
    Buf<uint32_t> d_idx;
    Buf<TrainNode> d_nodes;
    Buf<double> d_score;
    Buf<TrainBest> d_best;
    Buf<uint8_t> d_side;
    Buf<unsigned long long> d_neg;
    TRY(d_neg.alloc(1));
    HIP_TRY(hipMemsetAsync(d_neg.get(), 0, 8, t->s));
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 2; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_own{ev};
    for (auto &e : ev) TRY(hip_step(hipEventCreate(&e), "hipEventCreate"));
    const uint32_t F = t->p.features_per_node;
    std::vector<float> ms;
    uint32_t depth = 0;
    for (;; ++depth) {
        gr.stop_rules(depth, idx, level, split);
        if (split.empty()) break;
        const size_t m = split.size();
        TRY(d_idx.grow(idx.size()));
        TRY(d_nodes.grow(m));
        TRY(d_score.grow(m * F));
        TRY(d_best.grow(m));
        TRY(d_side.grow(idx.size()));
        HIP_TRY(hipMemcpyAsync(d_idx.get(), idx.data(), idx.size() * 4, hipMemcpyHostToDevice, t->s));
        HIP_TRY(hipMemcpyAsync(d_nodes.get(), split.data(), m * sizeof(TrainNode), hipMemcpyHostToDevice, t->s));
        TrainLevelArgs la{};
        la.box = t->box.get(); la.stride = (size_t)t->g.bw * t->g.bh; la.bw = t->g.bw;
        la.area = (double)t->g.rw * (double)t->g.rh;
        la.lab = t->lab.get(); la.off = t->off.get(); la.rot = t->rot.get();
        la.idx = d_idx.get(); la.nodes = d_nodes.get();
        la.n_nodes = (uint32_t)m; la.F = F; la.cblocks = (F + 255) / 256;
        la.seed = t->p.seed;
        la.W = t->p.subimage_width; la.H = t->p.subimage_height; la.rw = t->g.rw; la.rh = t->g.rh;
        la.scale = t->p.subrect_feature_scale;
        la.wdepth = 1.0 - exp(-((double)depth / t->p.steepness));       // (1 - e^(-rel!(depth, steepness))), houghforest.rs:289-292
        la.score = d_score.get(); la.best = d_best.get(); la.side = d_side.get(); la.neg_det = d_neg.get();
        HIP_TRY(hipEventRecord(ev[0], t->s));
        TRY(hip_step(dh_launch_train_level(la, t->s), "k_train_score"));
        HIP_TRY(hipEventRecord(ev[1], t->s));
        best.resize(m);
        side.resize(idx.size());
        HIP_TRY(hipMemcpyAsync(best.data(), d_best.get(), m * sizeof(TrainBest), hipMemcpyDeviceToHost, t->s));
        HIP_TRY(hipMemcpyAsync(side.data(), d_side.get(), idx.size(), hipMemcpyDeviceToHost, t->s));
        HIP_TRY(hipStreamSynchronize(t->s));
        float e_ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&e_ms, ev[0], ev[1]));
        ms.push_back(e_ms);
        gr.apply(idx, split, best.data(), side.data(), nidx, next);
        idx.swap(nidx);
        level.swap(next);
        if (level.empty()) break;
    }
    unsigned long long neg = 0;
    HIP_TRY(hipMemcpyAsync(&neg, d_neg.get(), 8, hipMemcpyDeviceToHost, t->s));
    HIP_TRY(hipStreamSynchronize(t->s));
    TRY(gr.assemble(out));
    t->neg_det = neg;
    t->stats = gr.stats;
    for (size_t i = 0; i < ms.size() && i < t->stats.size(); ++i) t->stats[i].ms = ms[i];
    return DH_OK;
}

static int trainer_stats_(const dh_trainer *t, dh_train_stats *out, uint32_t *nodes, uint32_t *leaves, float *level_ms, uint32_t cap) {
    if (!t || !out) return fail(DH_EINVAL, "dh_trainer_stats: NULL argument");
    *out = dh_train_stats{};
    out->frames = t->frames;
    out->pool_size = t->pool;
    for (uint8_t l : t->h_lab) out->pool_positives += l;
    out->neg_det = t->neg_det;
    out->levels = (uint32_t)t->stats.size();
    for (uint32_t i = 0; i < cap; ++i) {
        const bool have = i < t->stats.size();
        if (nodes) nodes[i] = have ? t->stats[i].nodes : 0;
        if (leaves) leaves[i] = have ? t->stats[i].leaves : 0;
        if (level_ms) level_ms[i] = have ? t->stats[i].ms : 0.f;
    }
    return DH_OK;
}

static int forest_export_(const dh_forest *f, int32_t *roots, dh_node *nodes, double *leaf_prob, uint32_t *off_begin, uint32_t *rot_begin,
                          float *offsets, double *rotations, uint32_t *n_off, uint32_t *n_rot) {
    if (!f) return fail(DH_EINVAL, "dh_forest_export: NULL forest");
    if (n_off) *n_off = (uint32_t)(f->offsets.size() / 3);
    if (n_rot) *n_rot = (uint32_t)(f->rotations.size() / 3);
    if (roots) std::copy(f->roots.begin(), f->roots.end(), roots);
    if (nodes) std::copy(f->nodes.begin(), f->nodes.end(), nodes);
    if (leaf_prob) std::copy(f->leaf_prob.begin(), f->leaf_prob.end(), leaf_prob);
    if (off_begin) std::copy(f->off_begin.begin(), f->off_begin.end(), off_begin);
    if (rot_begin) std::copy(f->rot_begin.begin(), f->rot_begin.end(), rot_begin);
    if (offsets) std::copy(f->offsets.begin(), f->offsets.end(), offsets);
    if (rotations) std::copy(f->rotations.begin(), f->rotations.end(), rotations);
    return DH_OK;
}

// ------------------------------------------------------------------ the C ABI (DH_API: dh_runtime.h)
DH_API(trainer_create, (const dh_train_params *p, int device, dh_trainer **out), (p, device, out))
DH_API(trainer_destroy, (dh_trainer *t), (t))
DH_API(trainer_add_frames, (dh_trainer *t, const uint16_t *frames, const uint8_t *masks, int n, int w, int h, const float *K, const float *pos3d, const float *rot_deg), (t, frames, masks, n, w, h, K, pos3d, rot_deg))
DH_API(trainer_fit, (dh_trainer *t, dh_forest **out), (t, out))
DH_API(trainer_stats, (const dh_trainer *t, dh_train_stats *out, uint32_t *nodes_per_level, uint32_t *leaves_per_level, float *level_ms, uint32_t cap_levels), (t, out, nodes_per_level, leaves_per_level, level_ms, cap_levels))
DH_API(forest_export, (const dh_forest *f, int32_t *roots, dh_node *nodes, double *leaf_prob, uint32_t *off_begin, uint32_t *rot_begin, float *offsets, double *rotations, uint32_t *n_off, uint32_t *n_rot), (f, roots, nodes, leaf_prob, off_begin, rot_begin, offsets, rotations, n_off, n_rot))
