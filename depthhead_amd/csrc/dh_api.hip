// dh_api.hip -- host runtime behind the C ABI of include/depthhead_hip.h: forest validation,
// HBM residency of the forest and its per-leaf tables, the per-batch workspace, kernel sequencing
// on a caller-supplied HIP stream, profiling events and the parity taps.
//
// Sits where HoughPrediction::predict_parameter_generic sits in the reference
// (src/hough/prediction.rs:421-493); the unit of work is a batch of frames.
//
// This unit holds the predictor and the calls that build a request for it and run it: camera batches, support, heads, the
// trackers, rigs.  The trainer, the renderer, the fit family and the fit trackers have units of their own
// (dh_api_train.hip, dh_api_render.hip, dh_api_fit.hip, dh_api_fit_track.hip) and share with this one what dh_runtime.h holds;
// the fit trackers also share dh_runtime_track.h with the trackers here, and call the three functions it declares.
#include "dh_runtime.h"
#include "dh_render.h"
#include "dh_runtime_track.h"

extern "C" const char *dh_last_error(void) { return dh_err_get_(); }
extern "C" int dh_version(void) { return DH_VERSION; }

// ------------------------------------------------------------------ forest (host side: dh_host.cpp validates and copies)
static int forest_create_(const dh_forest_desc *d, dh_forest **out) { return dh_forest_build_(d, out); }

static int forest_destroy_(dh_forest *f) {
    delete f;
    return DH_OK;
}

static int forest_info_(const dh_forest *f, uint32_t *n_trees, uint32_t *n_nodes, uint32_t *n_leaves, uint32_t *max_depth) {
    if (!f) return fail(DH_EINVAL, "dh_forest_info: NULL forest");
    if (n_trees) *n_trees = (uint32_t)f->roots.size();
    if (n_nodes) *n_nodes = (uint32_t)f->nodes.size();
    if (n_leaves) *n_leaves = (uint32_t)f->leaf_prob.size();
    if (max_depth) *max_depth = f->max_depth;
    return DH_OK;
}

// ------------------------------------------------------------------ geometry (dh_host.cpp)
static int patch_grid_(const dh_params *p, int w, int h, int *nx, int *ny) {
    if (!p || !nx || !ny) return fail(DH_EINVAL, "dh_patch_grid: NULL argument");
    return dh_patch_grid_(*p, w, h, nx, ny);
}

// ------------------------------------------------------------------ predictor
#define DH_MAX_CHUNKS 8
#define DH_MIN_CHUNK_FRAMES 16

// Everything reserve() sizes for a batch of frames of one geometry.  It is replaced as a whole: a captured batch has its
// pointers baked in, so replacing it drops the graph (free_workspace).
struct Workspace {
    Geom geom;
    int cap_frames = 0;
    Buf<HitRec> hits;
    Buf<HitBox> hit_box;
    Buf<HitRot> hit_rot;
    uint32_t hits_cap = 0;             // hit records per frame
    Buf<uint32_t> box;                 // [cap][box_rows][m][box_plane] rectangle-sum images (uniform path)
    Buf<unsigned long long> box_mask;  // [cap][ceil(box_rows / 32)][box_parts] which lanes wrote non-zero sums last time (BoxArgs::blk_mask)
    int blk_shift = 5;                 // log2 height of k_boxsum's mask blocks in this workspace (BoxArgs::blk_shift)
    Buf<uint32_t> tile_list;           // [DH_MAX_CHUNKS] x ([8][ceil(cap / 8) * tiles] uint2 entries + [8] counts behind them) (k_tile_list, k_tile_shift)
    size_t tile_list_stride = 0;       // entries per x
    TileShifts shifts;                 // the shifts of the tile grid a frame of this workspace chooses from (dh_tile_shifts_)
    Buf<uint32_t> tile_shift;          // [cap] sx | sy << 16 chosen for each frame of the last batch (k_tile_shift; zero otherwise)
    bool last_gated = false;           // the last batch's tiles gated their own windows (dh_tile_gate_; debug_window_totals_)
    int list_chunks = 0;               // kernel sequences of the last batch that ran with tile lists (debug_tile_shifts_)
    uint32_t *list_ptr(int chunk) const { return tile_list.get() + (size_t)chunk * 8 * (2 * tile_list_stride + 1); }
    Buf<uint32_t> win_patch;           // [cap][win_cap] window list: position in the window grid
    Buf<uint8_t> win_leaf;             // [cap][T][win_cap] window list: leaf per tree (u16 entries for forests of <= 65 535 leaves, else i32)
    int leaf_ls = 2;                   // log2 of its entry size
    Buf<uint32_t> pre_region;          // [pre_cap][2][64^3] the cells of both accumulators around the initial guesses, gathered by k_region (small batches with many hit records)
    int pre_cap = 0;
    uint32_t pre_min_hits = 0;         // frames with fewer hit records are gathered by k_cluster alone
    Buf<uint32_t> counters;            // the per-batch counter block: reached only through `lay` and the accessors below
    CounterLayout lay;
    Buf<dh_pose> poses;                // [cap] host entry points: poses and guesses of a slice on the device
    Buf<float> midp;
    Buf<double> rot;
    Buf<uint8_t> mask;
    Buf<uint16_t> frames;              // host entry points: frame staging (ensure_frame_staging)
    // leaf-id outputs for predict_mask / the 2-D Hough image, allocated on first use (aux_reserve)
    Buf<int32_t> aux_leaf;
    Buf<uint8_t> aux_flags;
    Buf<uint32_t> aux_u32;
    int aux_cap = 0;
    Buf<uint8_t> aux_out;
    // taps
    Buf<int32_t> dbg_leaf;
    Buf<uint8_t> dbg_flags;
    Buf<int32_t> dbg_guess, dbg_trace;
    Buf<uint32_t> dbg_steps;
    Buf<int32_t> dbg_votes;            // 16-byte vote records (debug_votes_)
    Buf<uint32_t> dbg_vcount;
    bool dbg_valid = false;
    // vote support (k_support), allocated by the first support call of this workspace (support_reserve): nothing else reads them,
    // so allocating them leaves every other buffer -- and a captured batch -- as it is
    Buf<uint32_t> hit_win;             // [cap][hits_cap] window of every hit record (k_emit's SUP instance)
    Buf<SupAcc> sup_acc;               // [cap] per-frame accumulators, zero between calls
    Buf<uint32_t> sup_bits;            // [cap][sup_words] window bitmaps, zero between calls
    uint32_t sup_words = 0;
    Buf<dh_support> sup;               // [cap] host entry points: the support records of a slice on the device
    // several heads per frame (k_heads.hip), allocated by the first heads call of this workspace (heads_reserve) beside the support
    // scratch, and like it read by nothing else; the arrays marked "zero" are zero between calls (their readers clear them)
    Buf<int32_t> hd_pick;              // [cap][DH_MAX_HEADS] seed cells
    Buf<uint32_t> hd_nseed;            // [cap]
    Buf<HdMom> hd_mom;                 // [cap][DH_MAX_HEADS] zero
    Buf<dh_pose> hd_pose;              // [cap][DH_MAX_HEADS]
    Buf<SupAcc> hd_acc;                // [cap][DH_MAX_HEADS] zero
    Buf<uint32_t> hd_bits;             // [cap][DH_MAX_HEADS][sup_words] zero
    Buf<dh_support> hd_sup;            // [cap][DH_MAX_HEADS]
    Buf<uint8_t> hd_mask;              // [cap][hits_cap]
    Buf<uint32_t> hd_rgrid;            // [cap][DH_MAX_HEADS][8000] zero
    Buf<dh_head> hd_out;               // [cap][DH_MAX_HEADS] host entry points: the heads of a slice on the device
    Buf<uint32_t> hd_n;                // [cap] host entry points

    // frame f0's entries of the counter block (CounterLayout, dh_host.h)
    uint32_t *hit_count(int f0) const { return counters.get() + lay.hit_count + f0; }
    uint32_t *pos_grid(int f0) const { return counters.get() + lay.pos_grid + (size_t)f0 * DH_POSGRID; }
    uint32_t *rot_grid(int f0) const { return counters.get() + lay.rot_grid + (size_t)f0 * DH_GRID3; }
    uint8_t *tile_flags(int f0) const { return (uint8_t *)(counters.get() + lay.tile_flags) + (size_t)f0 * lay.tiles; }
    uint32_t *win_count(int f0) const { return counters.get() + lay.win_count + (size_t)f0 * lay.tiles; }
    uint32_t *win_total(int f0) const { return counters.get() + lay.win_count + f0; }   // (gated batches only: CounterLayout, dh_host.h)
    uint32_t *leaf_hits(int f0) const { return lay.leaves ? counters.get() + lay.leaf_hits + (size_t)f0 * lay.leaves : nullptr; }
};

struct dh_predictor {
    int device = 0;
    Knobs knobs;
    dh_params params{};
    uint32_t n_trees = 0, n_nodes = 0, n_leaves = 0, n_off = 0, n_rot = 0, max_depth = 0;
    DevForest dev{};
    std::vector<Buf<uint8_t>> forest;   // the tables `dev` points into (forest_alloc)
    Buf<float> kern_r2;          // DH_KERN_R2 floats: the mean-shift kernel by squared distance
    Buf<uint16_t> zeros;         // 64 zero bytes (k_boxsum reads them for columns right of the image)
    bool f_uniform = false;      // forest has one split-rectangle size
    int f_rw = 0, f_rh = 0;
    Buf<NodeG> nodes_g;          // [n_nodes] general-path nodes with integer split bounds (patches up to 255 x 255), else empty
    Buf<uint4> nodes_u;          // 16-byte compact nodes for the current region layout (uniform path)
    Buf<uint4> nodes_a;          // NodeU[n_nodes + n_amb + 1]: the same nodes as the walk table of walk_absorb (children as byte offsets), or empty
    Buf<uint32_t> amb_flag;      // one word: number of nodes with an ambiguity band (k_nodes_compact's probe pass)
    Buf<uint32_t> amb_list;      // their indices (at most DH_AMB_CAP)
    uint32_t n_amb = 0;
    bool absorb_ok = false;      // the uniform path walks nodes_a (at most DH_AMB_CAP ambiguous nodes, table offsets fit 32 bits)
    Buf<uint32_t> top_tab;       // [T][2^top_levels] {offsets, ilo} heap + [T][2^top_levels] entry offsets (k_top_build), copied to LDS by every tile
    int top_levels = -1;         // DH_TOP_LEVELS, or -1: choose_tile decides per geometry
    long long nodes_u_key = 0;   // (ss_row, swizzle) the compact nodes were built for
    Buf<uint32_t> gen;           // [DH_MAX_CHUNKS] tile-flag tags, one per kernel sequence in flight (BoxArgs::gen)
    hipStream_t own_stream = nullptr;
    hipStream_t copy_stream = nullptr;    // host entry points: uploads run here, ahead of the kernels on own_stream
    hipEvent_t ev_stage[DH_STAGE_EVENTS] = {};   // chunk k uploaded (recorded on an upload stream, waited for on own_stream)
    hipEvent_t ev_slice = nullptr;        // the kernels that read the staging buffers are done (recorded on own_stream)
    Buf<uint8_t, PINNED> pin_small;       // page-locked staging of a slice's small host arrays: guesses in (small_stage)
    Buf<uint8_t, PINNED> pin_out;         // ... and its poses, support records and heads out (download)
    // run-length coded input (dh_predict_batch_rle): pinned staging + device copies of payload blob and run table
    Buf<uint8_t, PINNED> pin_blob;
    Buf<uint2, PINNED> pin_runs;
    Buf<uint32_t, PINNED> pin_begin;
    Buf<uint8_t> dev_blob;
    Buf<uint2> dev_runs;
    Buf<uint32_t> dev_begin;
    int chunks = 1;                       // sub-batches per call (env DH_CHUNKS)
    hipStream_t aux_stream[DH_MAX_CHUNKS - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[DH_MAX_CHUNKS - 1] = {};
    Workspace ws;
    Buf<float> blur_kern;        // gaussian_kernel_f32(gaussian_sigma) of the 2-D Hough variant, built on first use
    int blur_klen = 0;
    float blur_sigma = 0.0f;
    // captured batch (hipGraph)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    bool capturing = false;          // inside dh_graph_capture: one ordered pass on the capture stream
    bool graph_stale = false;        // the workspace a captured batch points into was reallocated: dh_graph_launch refuses
    bool debug = false;              // taps
    // last batch
    int last_n = 0;
    const uint16_t *last_frames = nullptr;
    // profiling
    bool profiling = false;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // start, emit end, vote end, cluster end, boxsum end, traverse end
    bool ev_valid = false;
#ifdef DH_PROFILING_KNOBS
    Buf<unsigned long long> trav_stamps, cl_stamps;   // DH_TRAV_STAMPS / DH_CL_STAMPS: cycles per phase, allocated on first use
#endif
};

// A table of the forest, owned by p->forest; the kernels see it through DevForest.
template <typename T>
static int forest_alloc(dh_predictor *p, T **out, size_t count) {
    Buf<uint8_t> b;
    TRY(b.alloc(std::max<size_t>(count, 1) * sizeof(T)));
    *out = (T *)b.get();
    p->forest.push_back(std::move(b));
    return DH_OK;
}
template <typename T>
static int upload(dh_predictor *p, const T **out, const std::vector<T> &v) {
    T *d = nullptr;
    TRY(forest_alloc(p, &d, v.size()));
    if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return DH_OK;
}

static int build_kernel_table(dh_predictor *p) {
    std::vector<float> r2;
    dh_build_kernel_r2_(p->params.gaussian_sigma, r2, DH_KERN_R2);    // get_or_build_kernel caches it per sigma (prediction.rs:310-317)
    HIP_TRY(hipMemcpy(p->kern_r2.get(), r2.data(), r2.size() * sizeof(float), hipMemcpyHostToDevice));
    return DH_OK;
}

static void drop_graph(dh_predictor *p) {
    if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
    if (p->graph) (void)hipGraphDestroy(p->graph);
    p->graph_exec = nullptr; p->graph = nullptr;
}

static void free_workspace(dh_predictor *p) {
    // a captured batch has the old workspace pointers baked in: replaying it would touch freed memory
    if (p->graph_exec) { drop_graph(p); p->graph_stale = true; }
    p->ws = Workspace{};
}

static int predictor_destroy_(dh_predictor *p) {
    if (!p) return DH_OK;
    DeviceGuard guard(p->device);      // (alive until the buffers have gone with `delete p`)
    if (p->own_stream) (void)hipStreamSynchronize(p->own_stream);
    for (auto &st : p->aux_stream) if (st) (void)hipStreamSynchronize(st);
    if (p->copy_stream) (void)hipStreamSynchronize(p->copy_stream);
    drop_graph(p);
    for (auto &e : p->ev) if (e) (void)hipEventDestroy(e);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    for (auto &e : p->ev_join) if (e) (void)hipEventDestroy(e);
    for (auto &e : p->ev_stage) if (e) (void)hipEventDestroy(e);
    if (p->ev_slice) (void)hipEventDestroy(p->ev_slice);
    for (auto &st : p->aux_stream) if (st) (void)hipStreamDestroy(st);
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    delete p;
    return DH_OK;
}

static int predictor_build(dh_predictor *p, const dh_forest *f, const dh_params *prm, int device);

static int predictor_create_(const dh_forest *f, const dh_params *prm, int device, dh_predictor **out) {
    if (!f || !prm || !out) return fail(DH_EINVAL, "dh_predictor_create: NULL argument");
    *out = nullptr;
    if (prm->stepwidth == 0 || prm->subimage_width == 0 || prm->subimage_height == 0) return fail(DH_EINVAL, "zero stepwidth / patch size");
    if (prm->subimage_width > 4096 || prm->subimage_height > 4096) return fail(DH_ESIZE, "patch larger than 4096");
    // rect sums are taken modulo 2^32: exact while sw*sh*65535 < 2^32
    if ((uint64_t)prm->subimage_width * prm->subimage_height * 65535ull >= (1ull << 32)) return fail(DH_ESIZE, "patch area %ux%u too large for u32 rectangle sums", prm->subimage_width, prm->subimage_height);
    if (!(prm->gaussian_sigma == prm->gaussian_sigma)) return fail(DH_EINVAL, "sigma is NaN");
    if (f->max_x > prm->subimage_width || f->max_y > prm->subimage_height)
        return fail(DH_EFOREST, "a split rectangle (max corner %u,%u) leaves the %ux%u patch", f->max_x, f->max_y, prm->subimage_width, prm->subimage_height);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(DH_EINVAL, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;

    dh_predictor *p = new (std::nothrow) dh_predictor;
    if (!p) return fail(DH_ENOMEM, "out of host memory");
    // (a host allocation failing half-way -- the packed vote arrays, the general-path nodes -- must not leak the device side)
    int rc = dh_guard_("dh_predictor_create", [&]() -> int { return predictor_build(p, f, prm, device); });
    if (rc != DH_OK) {
        const std::string keep = dh_err_get_();
        predictor_destroy_(p);
        dh_err_set_(keep.c_str());
        return rc;
    }
    *out = p;
    return DH_OK;
}

// A failure returns at once: predictor_create_ destroys what has been built.
static int predictor_build(dh_predictor *p, const dh_forest *f, const dh_params *prm, int device) {
    p->device = device;
    p->params = *prm;
    p->knobs = dh_read_knobs_();   // the only place the environment is read
    p->chunks = p->knobs.chunks;
    p->n_trees = (uint32_t)f->roots.size(); p->n_nodes = (uint32_t)f->nodes.size(); p->n_leaves = (uint32_t)f->leaf_prob.size();
    p->n_off = f->off_begin.back(); p->n_rot = f->rot_begin.back(); p->max_depth = f->max_depth;
    p->f_uniform = f->uniform; p->f_rw = f->rw; p->f_rh = f->rh;
    DevForest &d = p->dev;
    d.n_trees = p->n_trees; d.n_nodes = p->n_nodes; d.n_leaves = p->n_leaves; d.n_off = p->n_off; d.n_rot = p->n_rot;
    TRY(upload(p, &d.roots, f->roots));
    TRY(upload(p, &d.nodes, f->nodes));
    TRY(upload(p, &d.leaf_prob, f->leaf_prob));
    TRY(upload(p, &d.off_begin, f->off_begin));
    TRY(upload(p, &d.rot_begin, f->rot_begin));
    TRY(upload(p, &d.offsets, f->offsets));
    {
        // the offset votes once more as (x, y, z, 0) records, every leaf's run on a 64-byte boundary: the kernels
        // that walk a leaf's votes (k_vote, k_cluster) then touch whole cache lines with one 16-byte load per lane
        std::vector<uint32_t> b4;
        std::vector<float> o4f;
        dh_pack_off4_(*f, b4, o4f);
        std::vector<float4> o4(o4f.size() / 4);
        memcpy(o4.data(), o4f.data(), o4f.size() * sizeof(float));
        TRY(upload(p, &d.off4, o4));
        TRY(upload(p, &d.off4_begin, b4));
    }
    TRY(upload(p, &d.rotations, f->rotations));
    TRY(forest_alloc(p, &d.leaf_v, p->n_leaves));
    TRY(forest_alloc(p, &d.leaf_flags, p->n_leaves));
    TRY(forest_alloc(p, &d.rot_bin, p->n_rot));
    TRY(forest_alloc(p, &d.rot_rough, p->n_rot));
    TRY(forest_alloc(p, &d.rot_mult, p->n_rot));
    TRY(forest_alloc(p, &d.rough_mult, p->n_rot));
    TRY(forest_alloc(p, &d.rough_cell, p->n_rot));
    TRY(forest_alloc(p, &d.off_min, (size_t)p->n_leaves * 3));
    TRY(forest_alloc(p, &d.off_max, (size_t)p->n_leaves * 3));
    TRY(forest_alloc(p, &d.rbin_box, p->n_leaves));
    TRY(forest_alloc(p, &d.rbin_box_hi, p->n_leaves));
    TRY(forest_alloc(p, &d.tpl, p->n_leaves));
    TRY(forest_alloc(p, &d.rot_dir, p->n_leaves));
    TRY(p->kern_r2.alloc(DH_KERN_R2));
    TRY(p->zeros.alloc(32));
    TRY(p->gen.alloc(DH_MAX_CHUNKS));
    TRY(p->nodes_u.alloc(p->n_nodes));
    if (p->n_nodes > 0 && (size_t)p->n_nodes + p->n_leaves + 2 * DH_AMB_CAP < ((size_t)1 << 27) && !p->knobs.no_absorb) {   // (byte offsets into the table stay below 2^31)
        TRY(p->amb_flag.alloc(1));
        TRY(p->amb_list.alloc(DH_AMB_CAP));
    }
    if (prm->subimage_width <= 255 && prm->subimage_height <= 255 && p->n_nodes > 0) {
        // Integer split bounds of the general path (NodeG: dh_host.h, k_traverse.hip)
        std::vector<NodeG> ng;
        dh_build_nodes_g_(*f, ng);
        TRY(p->nodes_g.alloc(p->n_nodes));
        if (hipMemcpy(p->nodes_g.get(), ng.data(), ng.size() * sizeof(NodeG), hipMemcpyHostToDevice) != hipSuccess) return fail(DH_EHIP, "hipMemcpy(NodeG)");
    }
    TRY(hip_step(hipMemset(p->zeros.get(), 0, 64), "hipMemset"));
    const uint32_t ones[DH_MAX_CHUNKS] = {1, 1, 1, 1, 1, 1, 1, 1};
    TRY(hip_step(hipMemcpy(p->gen.get(), ones, sizeof ones, hipMemcpyHostToDevice), "hipMemcpy(gen)"));
    TRY(hip_step(dh_kernels_init(device), "hipFuncSetAttribute"));
    TRY(hip_step(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking), "hipStreamCreate"));
    TRY(hip_step(dh_launch_leaf_prepare(d, p->own_stream), "k_leaf_prepare launch"));
    TRY(hip_step(hipStreamSynchronize(p->own_stream), "k_leaf_prepare"));
    if (p->amb_flag && p->f_uniform) {
        // which nodes carry an ambiguity band?  (independent of the region layout: probed once with a dummy one)
        uint32_t n_amb = DH_AMB_CAP + 1;
        TRY(hip_step(hipMemsetAsync(p->amb_flag.get(), 0, sizeof(uint32_t), p->own_stream), "hipMemset"));
        TRY(hip_step(dh_launch_nodes_compact(d, 1, 0, 4, (uint32_t)(p->f_rw * p->f_rh), nullptr, nullptr, p->amb_flag.get(), p->amb_list.get(), 0, p->own_stream), "k_nodes_compact launch"));
        TRY(hip_step(hipMemcpyAsync(&n_amb, p->amb_flag.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, p->own_stream), "hipMemcpy"));
        TRY(hip_step(hipStreamSynchronize(p->own_stream), "k_nodes_compact"));
        // (the walk table keeps 12 bytes of LDS per tree even with no level in LDS: not for forests of thousands of trees)
        p->absorb_ok = n_amb <= DH_AMB_CAP && (size_t)p->n_trees * 12 <= 8 * 1024;
        if (p->absorb_ok) {
            p->n_amb = n_amb;
            TRY(p->nodes_a.alloc((size_t)p->n_nodes + n_amb + 1));
            p->top_levels = p->knobs.top_levels;          // -1: choose_tile decides per geometry
            TRY(p->top_tab.alloc((size_t)p->n_trees * (1u << 8) * 3));      // room for the 8 levels choose_tile may go to
        }
    }
    TRY(build_kernel_table(p));
    for (auto &e : p->ev) TRY(hip_step(hipEventCreate(&e), "hipEventCreate"));
    TRY(hip_step(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming), "hipEventCreate"));
    TRY(hip_step(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking), "hipStreamCreate"));
    for (auto &e : p->ev_stage) TRY(hip_step(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate"));
    TRY(hip_step(hipEventCreateWithFlags(&p->ev_slice, hipEventDisableTiming), "hipEventCreate"));
    for (int i = 0; i < DH_MAX_CHUNKS - 1; ++i) {
        TRY(hip_step(hipStreamCreateWithFlags(&p->aux_stream[i], hipStreamNonBlocking), "hipStreamCreate"));
        TRY(hip_step(hipEventCreateWithFlags(&p->ev_join[i], hipEventDisableTiming), "hipEventCreate"));
    }
    return DH_OK;
}

static int predictor_update_sigma_(dh_predictor *p, float val) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    if (val == p->params.gaussian_sigma || val <= 0.0f || val != val) return DH_OK;   // prediction.rs:321-323
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipDeviceSynchronize());
    p->params.gaussian_sigma = val;
    return build_kernel_table(p);
}
static int predictor_sigma_(const dh_predictor *p, float *out) {
    if (!p || !out) return fail(DH_EINVAL, "NULL argument");
    *out = p->params.gaussian_sigma;
    return DH_OK;
}

static int choose_tile(const dh_predictor *p, Geom &g, int cap) {
    TileQuery q;
    q.one_pass = cap == 1 && p->knobs.tile_x == 0;     // (a workspace for ONE frame: see dh_choose_tile_)
    q.params = p->params; q.f_rw = p->f_rw; q.f_rh = p->f_rh; q.n_trees = p->n_trees; q.absorb_ok = p->absorb_ok; q.top_levels = p->top_levels;
    q.lds_budget_kb = p->knobs.lds_budget_kb; q.tile_x = p->knobs.tile_x; q.tile_y = p->knobs.tile_y; q.box_band = p->knobs.box_band;
    return dh_choose_tile_(q, g);
}

// A workspace for at least n frames of w x h.  The old one is freed before the new one is allocated, so the two never hold
// memory at once; a failure leaves none.
static int reserve(dh_predictor *p, int n, int w, int h) {
    if (n <= 0) return fail(DH_EINVAL, "batch size must be positive");
    Geom g;
    g.w = w; g.h = h;
    TRY(dh_patch_grid_(p->params, w, h, &g.nx, &g.ny));
    g.npatch = g.nx * g.ny;
    bool same_geom = p->ws.geom.w == w && p->ws.geom.h == h;
    bool dbg_ok = !p->debug || p->ws.dbg_leaf;
    if (same_geom && n <= p->ws.cap_frames && dbg_ok) return DH_OK;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    int cap = std::max(n, same_geom ? p->ws.cap_frames : 0);
    free_workspace(p);
    if (g.npatch > 0) {
        // uniform-rectangle fast path: one rectangle size (<= 96 x 96, so a k_boxsum wave yields
        // >= 160 columns), rectangle sums fit i32
        g.uniform = p->f_uniform && (long)p->f_rw * p->f_rh <= 32768 && p->f_rw <= kBoxMaxRect && p->f_rh <= kBoxMaxRect && !p->knobs.force_general;
        int rc = choose_tile(p, g, cap);
        if (rc > 0) { g.uniform = false; rc = choose_tile(p, g, cap); }   // no tile fits the uniform layout
        if (rc) return rc;
    }
    Workspace ws;
    // k_boxsum's band / mask-block height: the shortest of 8, 16, 32 rows whose waves (12 per CU) still fit the chip at once for a
    // workspace of this many frames -- with few frames a wave's march of band + rh - 1 rows IS that kernel's duration
    if (g.uniform && g.box_rows > 0)
        for (int sh = 3; sh < 5; ++sh)
            if ((long)cap * g.box_parts * ((g.box_rows + (1 << sh) - 1) >> sh) <= 12L * 256) { ws.blk_shift = sh; break; }
    size_t hits_cap = std::max<size_t>((size_t)g.npatch * p->n_trees, 1);
    if (hits_cap > 0xffffffffull) return fail(DH_ESIZE, "too many (patch, tree) pairs per frame");
    ws.hits_cap = (uint32_t)hits_cap;
    TRY(ws.hits.alloc((size_t)cap * hits_cap));
    TRY(ws.hit_box.alloc((size_t)cap * hits_cap));
    TRY(ws.hit_rot.alloc((size_t)cap * hits_cap));
    const bool leaf_hist = p->n_leaves <= p->knobs.leaf_hist_max && !p->knobs.no_leaf_hist;
    // k_region pays a fixed ~20 us (second initial guess, flush, launch) for spreading the first region gather over
    // several workgroups: worth it from ~8 k hit records per frame on the rotation-record path of large forests, from
    // ~65 k with the leaf histogram (measured: config 3 cluster 0.77 -> 0.34 ms; config 5, 38 k records per frame, would lose)
    ws.pre_min_hits = p->knobs.region_min_hits > 0 ? (uint32_t)p->knobs.region_min_hits : (leaf_hist ? 65536u : 8192u);
    // (only where a frame of this geometry can plausibly hold that many records: a few per cent of its (window, tree) pairs vote)
    if (!p->knobs.no_region && hits_cap >= (leaf_hist ? 8 : 4) * (size_t)ws.pre_min_hits) {
        // k_region serves batches of up to 128 frames (beyond that the (frame, accumulator) workgroups of k_cluster fill the chip themselves)
        ws.pre_cap = std::min(cap, 128);
        TRY(ws.pre_region.alloc((size_t)ws.pre_cap * 2 * DH_SUPER_CELLS));   // (2 MB per frame; zeroed per batch, before k_region)
    }
    TRY(ws.win_patch.alloc((size_t)cap * std::max(g.win_cap, 1)));
    ws.leaf_ls = p->n_leaves <= 65535u ? 1 : 2;
    TRY(ws.win_leaf.alloc(((size_t)cap * std::max(g.win_cap, 1) * p->n_trees) << ws.leaf_ls));
    if (!p->knobs.no_tile_list && g.npatch > 0) {
        ws.tile_list_stride = (size_t)((cap + 7) / 8) * g.tiles_x * g.tiles_y;
        if (ws.tile_list_stride < ((size_t)1 << 30)) TRY(ws.tile_list.alloc((size_t)DH_MAX_CHUNKS * 8 * (2 * ws.tile_list_stride + 1)));
    }
    TRY(dh_tile_shifts_(g, (int)p->params.stepwidth, ws.blk_shift, p->knobs, &ws.shifts));
    if (!ws.tile_list) ws.shifts.on = false;
    if (ws.shifts.on) {
        TRY(ws.tile_shift.alloc(cap));
        if (hipMemsetAsync(ws.tile_shift.get(), 0, (size_t)cap * sizeof(uint32_t), p->own_stream) != hipSuccess) return fail(DH_EHIP, "hipMemset(tile_shift)");
    }
    if (g.uniform) {
        const size_t words = (size_t)cap * g.box_rows * ((size_t)g.box_plane << g.swz_log2);
        TRY(ws.box.alloc(words));
        // (the slack columns stay 0.  Zero-fills of a new workspace are ordered explicitly: issued on the predictor's stream and
        // waited for below -- the streams here are non-blocking ones, which the legacy stream of a plain hipMemset does not order)
        if (hipMemsetAsync(ws.box.get(), 0, words * sizeof(uint32_t), p->own_stream) != hipSuccess) return fail(DH_EHIP, "hipMemset(box)");
        if (!p->knobs.box_dense) {
            // zeroed together with the images: "cell non-zero => mask bit set" holds from the start
            const size_t mw = (size_t)cap * ((g.box_rows + 7) / 8) * g.box_parts;        // (sized for 8-row blocks: single-frame workspaces)
            TRY(ws.box_mask.alloc(mw));
            if (hipMemsetAsync(ws.box_mask.get(), 0, mw * sizeof(unsigned long long), p->own_stream) != hipSuccess) return fail(DH_EHIP, "hipMemset(box_mask)");
        }
    }
    if (hipStreamSynchronize(p->own_stream) != hipSuccess) return fail(DH_EHIP, "zero-fill of the rectangle-sum images");
    // one block, one memset per batch: hit counters | guess grids | tile flags | window counts | leaf histogram
    ws.lay = dh_counter_layout_(cap, g.flag_words, (size_t)g.tiles_x * g.tiles_y, leaf_hist ? p->n_leaves : 0);
    TRY(ws.counters.alloc(ws.lay.alloc_words));
    // (zeroed once here: the tile flags carry tags and get no fill of their own when k_boxsum clears the other counters)
    if (hipMemsetAsync(ws.counters.get(), 0, ws.lay.alloc_words * sizeof(uint32_t), p->own_stream) != hipSuccess ||
        hipStreamSynchronize(p->own_stream) != hipSuccess) return fail(DH_EHIP, "zero-fill of the counters");
    TRY(ws.poses.alloc(cap));
    TRY(ws.midp.alloc((size_t)cap * 3));
    TRY(ws.rot.alloc((size_t)cap * 3));
    TRY(ws.mask.alloc(cap));
    if (p->debug) {
        TRY(ws.dbg_leaf.alloc((size_t)cap * std::max(g.npatch, 1) * p->n_trees));
        TRY(ws.dbg_flags.alloc((size_t)cap * std::max(g.npatch, 1)));
        TRY(ws.dbg_guess.alloc((size_t)cap * 6));
        TRY(ws.dbg_trace.alloc((size_t)2 * cap * (p->params.meanshift_iterations + 1) * 3));
        TRY(ws.dbg_steps.alloc((size_t)2 * cap));
        TRY(ws.dbg_vcount.alloc(1));
    }
    const long long nkey = ((long long)g.ss_row << 32) | ((long long)g.top_levels << 24) | ((long long)g.swz_q << 4) | g.swz_log2;
    if (g.npatch > 0 && g.uniform && p->nodes_u_key != nkey) {     // compact nodes carry LDS offsets for this row stride
        hipError_t e = dh_launch_nodes_compact(p->dev, g.ss_row, g.swz_log2, g.swz_q, (uint32_t)(p->f_rw * p->f_rh), p->nodes_u.get(),
                                               p->absorb_ok ? p->nodes_a.get() : nullptr, nullptr, p->amb_list.get(), p->n_amb, p->own_stream);
        if (e == hipSuccess && p->absorb_ok) e = dh_launch_top_build(p->dev, p->nodes_a.get(), p->n_amb, g.top_levels, p->top_tab.get(), p->own_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->own_stream);
        if (e != hipSuccess) return fail(DH_EHIP, "k_nodes_compact: %s", hipGetErrorString(e));
        p->nodes_u_key = nkey;
    }
    ws.geom = g;
    ws.cap_frames = cap;
    p->ws = std::move(ws);
    return DH_OK;
}

static int predictor_set_forking_(dh_predictor *p, int chunks) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    if (chunks < 0 || chunks > DH_MAX_CHUNKS) return fail(DH_EINVAL, "dh_predictor_set_forking: chunks = %d, expected 0 .. %d", chunks, DH_MAX_CHUNKS);
    p->chunks = chunks;
    return DH_OK;
}
static int predictor_reserve_(dh_predictor *p, int n, int w, int h) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    return reserve(p, n, w, h);
}

// Which intrinsics a batch's frames see: one K for the whole batch (no table), or frame i -> camera c0 + i of a table.
struct CamSel {
    const dh_cameras *c = nullptr;
    int c0 = 0;
    CamSel at(int f) const { return CamSel{c, c0 + f}; }
    const DhCam *dev() const { return c ? c->dev.get() + c0 : nullptr; }
    // every camera of frames [0, n) is pinhole: the launch may take k_vote's PIN instance
    bool all_pin(int n) const {
        for (int i = 0; i < n; ++i) if (!c->host[(size_t)c0 + i].pin) return false;
        return true;
    }
    // k_vote's approximate cell quotient covers every camera of frames [0, n) (dh_vote_cell_fast_)
    bool all_cell_fast(int n, int w, int h) const {
        for (int i = 0; i < n; ++i) if (!dh_vote_cell_fast_(c->host[(size_t)c0 + i].k, w, h)) return false;
        return true;
    }
};

// One prediction: n frames of w x h seen through one K (cams.c == NULL) or frame i -> camera cams.c0 + i, per-frame guesses (each
// optional), and what it writes: poses into `out`, with `support` also each pose's vote support, or with `heads` the heads of
// every frame instead.  Its pointers are host or device ones, as the driver that runs it expects.  at(f) is the same request
// from frame f on: slices, forked sub-batches and staged chunks all take theirs that way.
enum ReqKind { POSES, SUPPORT, HEADS };     // the outputs an entry point promises (check_req)
template <typename T>
static T *off(T *ptr, size_t k) { return ptr ? ptr + k : nullptr; }
struct BatchReq {
    const uint16_t *frames = nullptr;
    int n = 0, w = 0, h = 0;
    const float *K = nullptr;
    CamSel cams;
    const float *midp = nullptr;       // guesses: [n][3], [n][3], [n] (bit0 midpoint, bit1 rotation)
    const double *rot = nullptr;
    const uint8_t *mask = nullptr;
    dh_pose *out = nullptr;            // [n] (unused with heads)
    ReqKind kind = POSES;
    uint32_t radius = 0;               // support and heads
    dh_support *support = nullptr;     // [n] non-NULL: k_emit's SUP instance, then k_support after k_cluster
    dh_head *heads = nullptr;          // [n][max_heads] non-NULL: k_emit's SUP instance, then the heads kernels in place of
    uint32_t *n_heads = nullptr;       // [n]              k_region / k_cluster
    int max_heads = 0;
    BatchReq at(int f) const {
        BatchReq r = *this;
        r.n = n - f; r.frames = off(frames, (size_t)f * w * h); r.cams = cams.at(f);
        r.midp = off(midp, (size_t)f * 3); r.rot = off(rot, (size_t)f * 3); r.mask = off(mask, f);
        r.out = off(out, f); r.support = off(support, f); r.heads = off(heads, (size_t)f * max_heads); r.n_heads = off(n_heads, f);
        return r;
    }
};

// How enqueue_range runs the kernels of a request.
struct EnqueueOpts {
    bool profile = false;           // events and roctx ranges (dh_set_profiling)
    int32_t *leaf_out = nullptr;    // k_traverse's leaf ids and patch flags into these instead of the taps (mask / 2-D Hough)
    uint8_t *flags_out = nullptr;
    bool traverse_only = false;     // stop after k_traverse
    int chunk = 0;                  // forked sub-batch: its tile-flag tag and tile list
    bool zero_fold = false;         // k_boxsum zeroes the counters: no fill of their own
};

// What the stages of enqueue_range share: frames [f0, f0 + n) of a resident slice, their place in the workspace, and what is
// decided once for the whole kernel sequence.  enqueue_range gives the first six (and kinv); the rest follows from them.  Every
// stage takes it by const reference.
struct Launch {
    dh_predictor *p;
    const BatchReq q;                  // the range's request, sl.at(f0): inputs and outputs from its first frame on
    const int f0, n; const hipStream_t s; const EnqueueOpts &o;
    float kinv[9];                     // inverse of K (below)
    const Workspace &ws = p->ws; const Geom &g = ws.geom;
    const int w = q.w, h = q.h; const DhCam *cams = q.cams.dev();
    const float *K = q.cams.c ? q.cams.c->host[q.cams.c0].k : q.K;   // one K, or the range's first camera: kernel-argument stand-ins there (the CAM instances read the records, `cams`)
    uint32_t *gen = p->gen.get() + o.chunk;      // this kernel sequence's tile-flag tag
    // the range's entries of the counter block (its window counts: set_windows); the tile flags are one byte per tile, frames packed back to back
    uint32_t *hit_count = ws.hit_count(f0), *pos_grid = ws.pos_grid(f0), *rot_grid = ws.rot_grid(f0), *leaf_hits = ws.leaf_hits(f0);
    uint8_t *tile_flags = ws.tile_flags(f0);
    size_t hoff = (size_t)f0 * ws.hits_cap;      // the range's first hit record
    // uniform path: its rectangle-sum images, how k_boxsum cuts them, its sparse-store masks
    uint32_t *box = g.uniform ? ws.box.get() + (size_t)f0 * g.box_rows * ((size_t)g.box_plane << g.swz_log2) : nullptr;
    BoxPlan bp = g.uniform ? dh_box_plan_(n, g, p->f_rh, ws.blk_shift, p->knobs) : BoxPlan();
    unsigned long long *blk_mask = ws.box_mask ? ws.box_mask.get() + (size_t)f0 * bp.mask_blocks * g.box_parts : nullptr;
    int step = (int)p->params.stepwidth, lw = (int)p->params.subimage_width / 2, lh = (int)p->params.subimage_height / 2;   // the window grid's stride, half a window
    // an unshifted tile on the image its flags come from: pitch, and the footprint of its windows -- in pixels, on the uniform path
    // less rw - 1, rh - 1 (the rectangle-sum image holds one cell per rectangle origin)
    int tpx = g.px * step, tpy = g.py * step;
    int tw = (g.px - 1) * step + (int)p->params.subimage_width - (g.uniform ? p->f_rw - 1 : 0);
    int th = (g.py - 1) * step + (int)p->params.subimage_height - (g.uniform ? p->f_rh - 1 : 0);
    bool use_list = dh_use_tile_list_((bool)ws.tile_list, g.npatch, o.leaf_out || o.flags_out || p->debug, n, g.tiles_x * g.tiles_y);   // product mode: the flagged tiles as compact lists
    uint2 *tl_list = use_list ? (uint2 *)ws.list_ptr(o.chunk) : nullptr;
    uint32_t *tl_count = use_list ? ws.list_ptr(o.chunk) + 16 * ws.tile_list_stride : nullptr;
    uint8_t *dbg_flags = o.flags_out ? o.flags_out : p->debug ? ws.dbg_flags.get() + (size_t)f0 * g.npatch : nullptr;   // k_traverse's and k_emit's patch flags: the caller's array, else the taps'
};

// The hit records of the frames from f0 on, for every argument block that reads or writes them.
template <typename A>
static void set_hits(A &a, const Workspace &ws, int f0) {
    const size_t hoff = (size_t)f0 * ws.hits_cap;
    a.hits = ws.hits.get() + hoff; a.hit_box = ws.hit_box.get() + hoff; a.hit_rot = ws.hit_rot.get() + hoff;
    a.hit_count = ws.hit_count(f0); a.hits_cap = ws.hits_cap;
}
// The window lists of the frames from f0 on: k_traverse writes them, k_emit and k_window_totals read them.
template <typename A>
static void set_windows(A &a, const Workspace &ws, int f0, uint32_t n_trees) {
    a.win_count = ws.win_count(f0); a.win_cap = ws.geom.win_cap; a.leaf_ls = ws.leaf_ls;
    a.win_patch = ws.win_patch.get() + (size_t)f0 * a.win_cap; a.win_leaf = ws.win_leaf.get() + (((size_t)f0 * a.win_cap * n_trees) << ws.leaf_ls);
}
#ifdef DH_PROFILING_KNOBS
// A kernel's cycle stamps (`words` of them, at most 16): allocated on first use; from then on every launch first prints, through
// `print`, what the last one summed.  Cleared either way.
template <typename Print>
static int next_stamps(Buf<unsigned long long> &buf, size_t words, unsigned long long **out, Print print) {
    if (!buf) TRY(buf.alloc(words));
    else {
        unsigned long long hst[16];
        HIP_TRY(hipMemcpy(hst, buf.get(), words * 8, hipMemcpyDeviceToHost));
        print(hst);
    }
    HIP_TRY(hipMemset(buf.get(), 0, words * 8));
    *out = buf.get();
    return DH_OK;
}
#endif

// Tile flags: k_boxsum with the rectangle-sum images (uniform path), else k_pixflags.
static int enqueue_flags(const Launch &L) {
    const Workspace &ws = L.ws; const Geom &g = L.g;
    if (!g.uniform) {
        PixFlagArgs fa{};
        fa.frames = L.q.frames; fa.n_frames = L.n; fa.w = L.w; fa.h = L.h; fa.tile_flags = L.tile_flags; fa.gen = L.gen;
        fa.tiles_x = g.tiles_x; fa.tiles_y = g.tiles_y; fa.tpx = L.tpx; fa.tpy = L.tpy; fa.tfw = L.tw; fa.tfh = L.th;
        { Range r(L.o.profile, "dh:pixflags"); HIP_TRY(dh_launch_pixflags(fa, L.s)); }
        return DH_OK;
    }
    BoxArgs ba{};
    ba.frames = L.q.frames; ba.zeros = L.p->zeros.get(); ba.n_frames = L.n; ba.w = L.w; ba.h = L.h; ba.rw = L.p->f_rw; ba.rh = L.p->f_rh;
    ba.tile_flags = L.tile_flags; ba.tiles_x = g.tiles_x; ba.tiles_y = g.tiles_y; ba.gen = L.gen; ba.tpx = L.tpx; ba.tpy = L.tpy; ba.tbw = L.tw; ba.tbh = L.th;
    if (L.o.zero_fold) { ba.zero_ptr = ws.counters.get(); ba.zero_lo = (uint32_t)ws.lay.zero_lo; ba.zero_hi = (uint32_t)ws.lay.zero_hi; ba.zero_end = (uint32_t)ws.lay.zero_words; }
    ba.out = L.box; ba.plane = g.box_plane; ba.rows = g.box_rows; ba.lg = g.swz_log2; ba.ow = g.box_ow; ba.parts = g.box_parts;
    ba.ring = L.bp.ring; ba.oh = L.bp.oh; ba.bands = L.bp.bands; ba.blocks_per_frame = L.bp.blocks_per_frame;
    ba.blk_shift = ws.blk_shift; ba.mask_blocks = L.bp.mask_blocks; ba.blk_mask = L.blk_mask;
    if (L.use_list && ws.shifts.on) ba.list_count = L.tl_count;     // k_tile_shift appends to the lists
    { Range r(L.o.profile, "dh:boxsum"); HIP_TRY(dh_launch_boxsum(ba, L.s)); }
    return DH_OK;
}
// The tile lists of a launch that uses them.  A workspace whose frames choose the shift of their tile grid: k_tile_shift counts the
// flagged tiles of every allowed shift on k_boxsum's masks and writes the lists of the best one (k_boxsum's flags then serve the
// other paths only); else k_tile_list compacts the flags.
static int enqueue_tile_list(const Launch &L) {
    const Workspace &ws = L.ws; const Geom &g = L.g;
    Range r(L.o.profile, "dh:tile_list");
    if (!ws.shifts.on) { HIP_TRY(dh_launch_tile_list(L.tile_flags, L.gen, L.n, g.tiles_x * g.tiles_y, L.tl_list, L.tl_count, (uint32_t)ws.tile_list_stride, L.s)); return DH_OK; }
    TileShiftArgs sa{};
    sa.n_frames = L.n; sa.blk_shift = ws.blk_shift; sa.mask_blocks = L.bp.mask_blocks; sa.parts = g.box_parts; sa.blk_mask = L.blk_mask; sa.ow4 = g.box_ow / 4; sa.nc = g.box_parts * sa.ow4;
    sa.tiles_x = g.tiles_x; sa.tiles_y = g.tiles_y; sa.step = L.step; sa.tpx = L.tpx; sa.tpy = L.tpy; sa.tbw = L.tw; sa.tbh = L.th;
    sa.sx0 = ws.shifts.sx0; sa.sy0 = ws.shifts.sy0; sa.gx = ws.shifts.gx; sa.nsx = ws.shifts.nsx; sa.nsy = ws.shifts.nsy;
    sa.list = L.tl_list; sa.count = L.tl_count; sa.stride = (uint32_t)ws.tile_list_stride; sa.shift_out = ws.tile_shift.get() + L.f0;
    HIP_TRY(dh_launch_tile_shift(sa, L.s));
    return DH_OK;
}
// k_traverse.  *gated: its tiles gate their own windows, and k_emit takes the pre-gated lists (enqueue_emit).
static int enqueue_traverse(const Launch &L, bool *gated) {
    dh_predictor *p = L.p;
    const Workspace &ws = L.ws; const Geom &g = L.g;
    TraverseArgs ta{};
    ta.frames = L.q.frames; ta.n_frames = L.n; ta.w = L.w; ta.h = L.h;
    ta.step = L.step; ta.sw = (int)p->params.subimage_width; ta.sh = (int)p->params.subimage_height;
    ta.nx = g.nx; ta.ny = g.ny; ta.px = g.px; ta.py = g.py; ta.tiles_x = g.tiles_x; ta.tiles_y = g.tiles_y;
    ta.ss_max = g.ss_max; ta.ss_row = g.ss_row; ta.swz_log2 = g.swz_log2; ta.swz_q = g.swz_q;
    ta.uniform = g.uniform ? 1 : 0; ta.rw = p->f_rw; ta.rh = p->f_rh; ta.area = (uint32_t)(p->f_rw * p->f_rh);
    ta.nodes_u = p->nodes_u.get(); ta.nodes_a = p->absorb_ok ? p->nodes_a.get() : nullptr; ta.walk_lb = (p->n_nodes + p->n_amb) << 4; ta.amb_list = p->amb_list.get();
    ta.top_tab = p->top_tab.get(); ta.top_levels = g.top_levels; ta.nodes_g = p->knobs.no_general_int ? nullptr : p->nodes_g.get();
    ta.box = L.box; ta.box_plane = g.box_plane; ta.box_rows = g.box_rows; ta.tile_flags = L.tile_flags; ta.gen = L.gen;
#ifdef DH_PROFILING_KNOBS
    ta.stop_phase = p->knobs.trav_stop;
    if (p->knobs.trav_stamps)
        TRY(next_stamps(p->trav_stamps, 8, &ta.dbg_stamps, [](const unsigned long long *hst) {
            fprintf(stderr, "[k_traverse cycles/phase summed over the workgroups that reach it] region=%llu gate=%llu walks=%llu gated tail=%llu\n", hst[0], hst[1], hst[2], hst[3]);
        }));
#endif
    ta.f = p->dev; set_windows(ta, ws, L.f0, p->n_trees);
    // the tiles gate their own windows wherever the rule allows (dh_host.h); a launch that stops here feeds the taps' arrays
    *gated = !L.o.traverse_only && !L.o.leaf_out && !L.o.flags_out && dh_tile_gate_(g, ws.cap_frames, p->absorb_ok, p->n_trees, p->debug, p->knobs);
    if (*gated) { ta.tile_gate = 1; ta.win_total = ws.win_total(L.f0); }
    if (!L.o.traverse_only) p->ws.last_gated = *gated;
    ta.dbg_flags = L.dbg_flags; ta.dbg_leaf = L.o.leaf_out ? L.o.leaf_out : p->debug ? ws.dbg_leaf.get() + (size_t)L.f0 * g.npatch * p->n_trees : nullptr;
    if (L.use_list) { ta.tile_list = L.tl_list; ta.tile_list_count = L.tl_count; ta.tile_list_stride = (uint32_t)ws.tile_list_stride; }
    { Range r(L.o.profile, "dh:traverse"); HIP_TRY(dh_launch_traverse(ta, g.lds, L.s)); }
    return DH_OK;
}
// k_emit on the window lists enqueue_traverse left: pre-gated ones where its tiles gated.
static int enqueue_emit(const Launch &L, bool gated) {
    const Geom &g = L.g;
    EmitArgs ea{};
    ea.frames = L.q.frames; ea.n_frames = L.n; ea.w = L.w; ea.h = L.h;
    ea.step = L.step; ea.lw = L.lw; ea.lh = L.lh; ea.nx = g.nx; ea.npatch = g.npatch; ea.px = g.px; ea.py = g.py; ea.tiles = g.tiles_x * g.tiles_y;
    memcpy(ea.kinv, L.kinv, sizeof ea.kinv);
    ea.cams = L.cams; ea.f = L.p->dev; set_windows(ea, L.ws, L.f0, L.p->n_trees);
    if (gated) { ea.pre_gated = 1; ea.win_total = L.ws.win_total(L.f0); }
    set_hits(ea, L.ws, L.f0);
    // (a heads batch keeps every hit's rotation record: its rotation votes are restricted per head, hit by hit)
    ea.leaf_hits = L.q.heads ? nullptr : L.leaf_hits;
    ea.gen = L.gen; ea.dbg_flags = L.dbg_flags;
    if (L.q.support || L.q.heads) ea.hit_win = L.ws.hit_win.get() + L.hoff;
#ifdef DH_PROFILING_KNOBS
    ea.stop = L.p->knobs.emit_stop;
#endif
    { Range r(L.o.profile, "dh:emit"); HIP_TRY(dh_launch_emit(ea, L.s)); }
    return DH_OK;
}
static int enqueue_vote(const Launch &L) {
    const CamSel &cs = L.q.cams;
    VoteArgs va{};
    va.n_frames = L.n; va.w = L.w; va.h = L.h;
    va.cell_fast = !L.p->knobs.vote_exact && (!cs.c || cs.all_cell_fast(L.n, L.w, L.h)) ? 1 : 0;   // (one K: dh_launch_vote decides)
    memcpy(va.k, L.K, sizeof va.k);
    va.cams = L.cams; va.cams_pin = cs.c && cs.all_pin(L.n) ? 1 : 0; va.f = L.p->dev;
    set_hits(va, L.ws, L.f0);
    va.pos_grid = L.pos_grid; va.rot_grid = L.rot_grid; va.leaf_hits = L.q.heads ? nullptr : L.leaf_hits;
#ifdef DH_PROFILING_KNOBS
    va.stop = L.p->knobs.vote_stop;
#endif
    { Range r(L.o.profile, "dh:vote"); HIP_TRY(dh_launch_vote(va, L.s)); }
    return DH_OK;
}
// What k_cluster's pose instances and its HEADS instances take alike; the rotation grid, the leaf histogram and the outputs differ.
static ClusterArgs cluster_args(const Launch &L) {
    ClusterArgs ca{};
    ca.frames = L.q.frames; ca.n_frames = L.n; ca.w = L.w; ca.h = L.h;
    memcpy(ca.kinv, L.kinv, sizeof ca.kinv);
    ca.cams = L.cams; ca.f = L.p->dev; set_hits(ca, L.ws, L.f0);
    ca.pos_grid = L.pos_grid; ca.kern_r2 = L.p->kern_r2.get(); ca.iterations = L.p->params.meanshift_iterations;
    return ca;
}
// [k_region,] k_cluster: one pose per frame.
static int enqueue_cluster(const Launch &L) {
    dh_predictor *p = L.p; const Workspace &ws = L.ws;
    ClusterArgs ca = cluster_args(L);
    ca.leaf_hits = L.leaf_hits; ca.rot_grid = L.rot_grid;
#ifdef DH_PROFILING_KNOBS
    ca.stop = p->knobs.cl_stop;
    if (p->knobs.cl_stamps)
        TRY(next_stamps(p->cl_stamps, 16, &ca.dbg_stamps, [](const unsigned long long *hst) {
            fprintf(stderr, "[k_cluster rotation workgroups, cycles summed] guess=%llu zero=%llu gather=%llu | sums: count sweep=%llu (4)=%llu scan+park=%llu (6)=%llu chain=%llu update=%llu | sums=%llu workgroups=%llu\n",
                    hst[0], hst[1], hst[2], hst[3], hst[4], hst[5], hst[6], hst[7], hst[8], hst[14], hst[15]);
        }));
#endif
    ca.midp_guess = L.q.midp; ca.rot_guess = L.q.rot; ca.guess_mask = L.q.mask; ca.out = L.q.out;
    if (p->debug) { ca.dbg_guess = ws.dbg_guess.get(); ca.dbg_trace = ws.dbg_trace.get(); ca.dbg_steps = ws.dbg_steps.get(); }
    // few frames with many hit records each: the first region of every accumulator is gathered by several workgroups
    const int slices = std::min(16, 256 / std::max(L.n, 1));
    if (ws.pre_region && slices >= 2 && L.f0 + L.n <= ws.pre_cap && ca.iterations > 0) {
        ca.pre_region = ws.pre_region.get() + (size_t)L.f0 * 2 * DH_SUPER_CELLS; ca.pre_slices = slices; ca.pre_min_hits = ws.pre_min_hits;
        // (a kernel node inside a captured graph, like the counters' fill)
        const size_t pre_bytes = (size_t)L.n * 2 * DH_SUPER_CELLS * sizeof(uint32_t);
        if (p->capturing) HIP_TRY(dh_launch_zero(ca.pre_region, pre_bytes, L.s));
        else HIP_TRY(hipMemsetAsync(ca.pre_region, 0, pre_bytes, L.s));
        { Range r(L.o.profile, "dh:region"); HIP_TRY(dh_launch_region(ca, L.s)); }
    }
    { Range r(L.o.profile, "dh:cluster"); HIP_TRY(dh_launch_cluster(ca, L.s)); }
    return DH_OK;
}
// Several heads per frame: seeds, their moments, position mean shifts, support (+ head masks and rotation grids), rotation mean
// shifts, merge (k_heads.hip), in place of k_region / k_cluster.
static int enqueue_heads(const Launch &L) {
    const Workspace &ws = L.ws; const BatchReq &q = L.q;
    HeadsArgs ha{};
    ha.n_frames = L.n; ha.w = L.w; ha.h = L.h; ha.max_heads = q.max_heads;
    memcpy(ha.k, L.K, sizeof ha.k);
    ha.cams = L.cams; ha.off4 = L.p->dev.off4; ha.rough_cell = L.p->dev.rough_cell;
    set_hits(ha, ws, L.f0);
    ha.hit_win = ws.hit_win.get() + L.hoff; ha.pos_grid = L.pos_grid;
    const size_t hk = (size_t)L.f0 * DH_MAX_HEADS;
    ha.pick = ws.hd_pick.get() + hk; ha.nseed = ws.hd_nseed.get() + L.f0; ha.mom = ws.hd_mom.get() + hk;
    ha.nx = L.g.nx; ha.step = L.step; ha.lw = L.lw; ha.lh = L.lh; ha.radius = q.radius; ha.n_heads = q.n_heads; ha.heads = q.heads;
    ha.hpose = ws.hd_pose.get() + hk; ha.acc = ws.hd_acc.get() + hk; ha.bits = ws.hd_bits.get() + hk * ws.sup_words; ha.bit_words = ws.sup_words;
    ha.hsup = ws.hd_sup.get() + hk; ha.hmask = ws.hd_mask.get() + L.hoff; ha.rgrid = ws.hd_rgrid.get() + hk * DH_GRID3;
    ClusterArgs ca = cluster_args(L);
    ca.rot_grid = ha.rgrid; ca.out = ws.hd_pose.get() + hk; ca.hd_nseed = ha.nseed; ca.hd_mom = ha.mom; ca.hd_rgrid = ha.rgrid; ca.hd_mask = ha.hmask;
    Range r(L.o.profile, "dh:heads");
    HIP_TRY(dh_launch_heads_seeds(ha, L.s));
    HIP_TRY(dh_launch_heads_moments(ha, L.s));
    ca.hd_which = 0;
    HIP_TRY(dh_launch_cluster_heads(ca, q.max_heads, L.s));
    HIP_TRY(dh_launch_heads_support(ha, L.s));
    ca.hd_which = 1;
    HIP_TRY(dh_launch_cluster_heads(ca, q.max_heads, L.s));
    HIP_TRY(dh_launch_heads_finish(ha, L.s));
    return DH_OK;
}
// k_support: each pose's vote support, after k_cluster.
static int enqueue_support(const Launch &L) {
    const Workspace &ws = L.ws;
    SupportArgs sa{};
    sa.n_frames = L.n; sa.nx = L.g.nx; sa.step = L.step; sa.lw = L.lw; sa.lh = L.lh;
    sa.radius = L.q.radius; sa.poses = L.q.out; sa.out = L.q.support;
    sa.hits = ws.hits.get() + L.hoff; sa.hit_box = ws.hit_box.get() + L.hoff; sa.hit_win = ws.hit_win.get() + L.hoff;
    sa.hit_count = L.hit_count; sa.hits_cap = ws.hits_cap; sa.off4 = L.p->dev.off4;
    sa.acc = ws.sup_acc.get() + L.f0; sa.bits = ws.sup_bits.get() + (size_t)L.f0 * ws.sup_words; sa.bit_words = ws.sup_words;
    { Range r(L.o.profile, "dh:support"); HIP_TRY(dh_launch_support(sa, L.s)); }
    return DH_OK;
}

// Enqueue the kernels (k_boxsum / k_pixflags, k_traverse, k_emit, k_vote, then [k_region,] k_cluster [, k_support] or the heads
// kernels) for frames [f0, f0 + n) of the resident slice sl on stream s: sl.at(f0) gives their inputs and outputs, f0 their place
// in the workspace.  This is the sequence and the profiling events; each stage above fills its own argument blocks.
static int enqueue_range(dh_predictor *p, const BatchReq &sl, int f0, int n, hipStream_t s, const EnqueueOpts &o) {
    Launch L{p, sl.at(f0), f0, n, s, o};
    if (L.q.cams.c) memcpy(L.kinv, L.q.cams.c->host[L.q.cams.c0].kinv, sizeof L.kinv);
    else dh_mat3_inv_f32_(L.K, L.kinv);   // cached in a RefCell by the reference (types.rs:436-441)
    if (L.use_list) p->ws.list_chunks = std::max(p->ws.list_chunks, o.chunk + 1);
    const bool windows = L.g.npatch > 0;
    char batch_name[48];
    snprintf(batch_name, sizeof batch_name, "dh:batch n=%d %dx%d", n, L.w, L.h);
    Range batch_range(o.profile, batch_name);
    if (o.profile) HIP_TRY(hipEventRecord(p->ev[0], s));
    if (windows) TRY(enqueue_flags(L));
    if (L.use_list) TRY(enqueue_tile_list(L));
    if (o.profile) HIP_TRY(hipEventRecord(p->ev[4], s));
    bool gated = false;
    if (windows) TRY(enqueue_traverse(L, &gated));
    if (o.profile) HIP_TRY(hipEventRecord(p->ev[5], s));
    if (windows && !o.traverse_only) TRY(enqueue_emit(L, gated));
    if (o.profile) HIP_TRY(hipEventRecord(p->ev[1], s));
    if (o.traverse_only) return DH_OK;
    TRY(enqueue_vote(L));
    if (o.profile) HIP_TRY(hipEventRecord(p->ev[2], s));
    if (L.q.heads) TRY(enqueue_heads(L));
    else {
        TRY(enqueue_cluster(L));
        if (L.q.support) TRY(enqueue_support(L));
    }
    if (o.profile) { HIP_TRY(hipEventRecord(p->ev[3], s)); p->ev_valid = true; }
    return DH_OK;
}

// Largest number of frames whose hit records are resident at once (64 B x window positions x trees
// per frame: 9 MB per frame at BASELINE config 2).  Larger batches are walked in slices on the same
// stream, reusing the workspace.
static int max_resident_frames(const dh_predictor *p) { return p->knobs.max_resident; }

// The support scratch of the current workspace (Workspace::hit_win ..), allocated and zeroed on the first support call that
// needs it; a no-op after that.  Nothing a captured batch points to is touched.
static int support_reserve(dh_predictor *p) {
    Workspace &ws = p->ws;
    if (ws.sup) return DH_OK;           // (allocated last: its presence means the others are there and zeroed)
    const size_t cap = (size_t)ws.cap_frames;
    ws.sup_words = (uint32_t)((std::max(ws.geom.npatch, 1) + 31) / 32);
    TRY(ws.hit_win.alloc(cap * ws.hits_cap));
    TRY(ws.sup_acc.alloc(cap));
    TRY(ws.sup_bits.alloc(cap * ws.sup_words));
    TRY(ws.sup.alloc(cap));
    if (hipMemsetAsync(ws.sup_acc.get(), 0, cap * sizeof(SupAcc), p->own_stream) != hipSuccess ||
        hipMemsetAsync(ws.sup_bits.get(), 0, cap * ws.sup_words * sizeof(uint32_t), p->own_stream) != hipSuccess ||
        hipStreamSynchronize(p->own_stream) != hipSuccess) {
        ws.sup.reset();
        return fail(DH_EHIP, "zero-fill of the support scratch");
    }
    return DH_OK;
}

// The heads scratch of the current workspace (Workspace::hd_*, and the support scratch it shares: k_emit's hit windows), allocated
// and zeroed on the first heads call that needs it; a no-op after that.  Nothing a captured batch points to is touched.
static int heads_reserve(dh_predictor *p) {
    TRY(support_reserve(p));
    Workspace &ws = p->ws;
    if (ws.hd_n) return DH_OK;          // (allocated last: its presence means the others are there and zeroed)
    const size_t cap = (size_t)ws.cap_frames, ch = cap * DH_MAX_HEADS;
    TRY(ws.hd_pick.alloc(ch));
    TRY(ws.hd_nseed.alloc(cap));
    TRY(ws.hd_mom.alloc(ch));
    TRY(ws.hd_pose.alloc(ch));
    TRY(ws.hd_acc.alloc(ch));
    TRY(ws.hd_bits.alloc(ch * ws.sup_words));
    TRY(ws.hd_sup.alloc(ch));
    TRY(ws.hd_mask.alloc(cap * ws.hits_cap));
    TRY(ws.hd_rgrid.alloc(ch * DH_GRID3));
    TRY(ws.hd_out.alloc(ch));
    if (hipMemsetAsync(ws.hd_mom.get(), 0, ch * sizeof(HdMom), p->own_stream) != hipSuccess ||
        hipMemsetAsync(ws.hd_acc.get(), 0, ch * sizeof(SupAcc), p->own_stream) != hipSuccess ||
        hipMemsetAsync(ws.hd_bits.get(), 0, ch * ws.sup_words * sizeof(uint32_t), p->own_stream) != hipSuccess ||
        hipMemsetAsync(ws.hd_rgrid.get(), 0, ch * DH_GRID3 * sizeof(uint32_t), p->own_stream) != hipSuccess ||
        hipStreamSynchronize(p->own_stream) != hipSuccess)
        return fail(DH_EHIP, "zero-fill of the heads scratch");
    TRY(ws.hd_n.alloc(cap));
    return DH_OK;
}

// Everything a request's kernels touch, for `frames` frames of its geometry: the workspace, then the support scratch or the heads
// scratch when r asks for support records or heads.
static int reserve_req(dh_predictor *p, const BatchReq &r, int frames) {
    TRY(reserve(p, frames, r.w, r.h));
    if (r.support) TRY(support_reserve(p));
    if (r.heads) TRY(heads_reserve(p));
    return DH_OK;
}

// ------------------------------------------------------------------ checking a request
// shared checks of the camera calls: n frames against the table, the table on the predictor's device
static int cameras_check(const dh_predictor *p, const dh_cameras *c, int n, const char *fn) {
    if (c->device != p->device) return fail(DH_EINVAL, "%s: camera table on device %d, predictor on device %d", fn, c->device, p->device);
    if (n > c->n) return fail(DH_EINVAL, "%s: %d frames, the camera table has %d cameras", fn, n, c->n);
    return DH_OK;
}

// The checks of a request made by entry point fn, on the host before anything is launched.  An input with several faults
// reports the first of them in this order:
//   1. a radius (support, heads) above 2^31 - 1: a negative int passed
//   2. max_heads (heads) outside 1 .. DH_MAX_HEADS
//   3. NULL support records (support)
//   4. any other NULL: the predictor, the input (`input`: the frames or the payloads), K or the camera table, the poses or
//      the heads and their counts
//   5. n < 0
//   6. the camera table: on the predictor's device, a camera for every frame
//   7. n == 0: nothing to run, DH_OK (run returns before selecting the device)
static int check_req(const dh_predictor *p, const BatchReq &r, bool input, const char *fn) {
    if (r.kind != POSES && r.radius > 0x7fffffffu) return fail(DH_EINVAL, "%s: radius %u (a negative int?); expected 0 .. 2^31 - 1", fn, r.radius);
    if (r.kind == HEADS && (r.max_heads < 1 || r.max_heads > DH_MAX_HEADS))
        return fail(DH_EINVAL, "%s: max_heads %d outside 1 .. %d", fn, r.max_heads, DH_MAX_HEADS);
    if (r.kind == SUPPORT && !r.support) return fail(DH_EINVAL, "%s: NULL support", fn);
    if (!p || !input || (!r.K && !r.cams.c) || (r.kind == HEADS ? !r.heads || !r.n_heads : !r.out)) return fail(DH_EINVAL, "%s: NULL argument", fn);
    if (r.n < 0) return fail(DH_EINVAL, "negative batch size");
    if (r.cams.c) TRY(cameras_check(p, r.cams.c, r.n, fn));
    return DH_OK;
}

// Every prediction entry point: its request checked (check_req), then driver() on the predictor's device.
template <typename F>
static int run(dh_predictor *p, const BatchReq &r, bool input, const char *fn, F driver) {
    TRY(check_req(p, r, input, fn));
    if (r.n == 0) return DH_OK;
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    return driver();
}

// ------------------------------------------------------------------ the batch drivers
// The device batch every prediction runs (request checked, device selected): r's arrays are on the device, its kernels go to
// stream s.  Frames beyond the resident limit run in slices; the slices and forked sub-batches each take their part of r.
static int batch_device(dh_predictor *p, const BatchReq &r, hipStream_t s) {
    const int n = r.n, slice = p->debug ? n : std::min(n, max_resident_frames(p));   // the taps index the whole batch
    TRY(reserve_req(p, r, slice));
    for (int f0 = 0; f0 < n; f0 += slice) {
        BatchReq sl = r.at(f0);
        sl.n = std::min(slice, n - f0);
        const int m = sl.n;
        p->ws.list_chunks = 0;
        // Forked sub-batches: two halves of the slice on two streams let the latency-bound tail kernels of one half run
        // beside the head kernels of the other.  Measured on MI355X: it pays once each half still has >= 256 frames
        // (512 frames per call: 479 k -> 533 k frames/s with 2 chunks, 483 k with 4; 256 frames per call: no gain),
        // so that is the automatic choice; DH_CHUNKS forces a count.
        int chunks = p->chunks > 0 ? p->chunks : (m >= 512 ? 2 : 1);
        if (p->profiling || p->debug || p->capturing || m < 2 * DH_MIN_CHUNK_FRAMES) chunks = 1;
        chunks = std::min(chunks, m / DH_MIN_CHUNK_FRAMES);
        // The per-batch counters: one kernel sequence on the uniform path has them cleared by its first kernel (k_boxsum: every
        // wave of its grid takes a share; the tile flags carry tags and need no fill) -- one dispatch less per batch, 4.7 us of a
        // single frame's 95.  Forked sub-batches, the general path and frames smaller than the patch keep the fill.
        const Workspace &ws = p->ws;
        const bool fold = chunks <= 1 && ws.geom.uniform && ws.geom.npatch > 0 && ws.lay.zero_words < 0xffffffffull && !p->knobs.no_zero_fold;
        if (!fold) {
            // (inside a captured graph the zero-fill is a kernel node: see k_zero)
            if (p->capturing) HIP_TRY(dh_launch_zero(ws.counters.get(), (ws.lay.zero_words * sizeof(uint32_t) + 15) & ~(size_t)15, s));
            else HIP_TRY(hipMemsetAsync(ws.counters.get(), 0, ws.lay.zero_words * sizeof(uint32_t), s));
        }
        if (chunks <= 1) {
            EnqueueOpts o;
            o.profile = p->profiling; o.zero_fold = fold;
            TRY(enqueue_range(p, sl, 0, m, s, o));
        } else {
            HIP_TRY(hipEventRecord(p->ev_fork, s));
            for (int c = 0; c < chunks; ++c) {
                const int c0 = (int)((long long)m * c / chunks), c1 = (int)((long long)m * (c + 1) / chunks);
                hipStream_t cs = c == 0 ? s : p->aux_stream[c - 1];
                if (c > 0) HIP_TRY(hipStreamWaitEvent(cs, p->ev_fork, 0));
                EnqueueOpts o;
                o.chunk = c;
                TRY(enqueue_range(p, sl, c0, c1 - c0, cs, o));
                if (c > 0) {
                    HIP_TRY(hipEventRecord(p->ev_join[c - 1], cs));
                    HIP_TRY(hipStreamWaitEvent(s, p->ev_join[c - 1], 0));
                }
            }
        }
    }
    p->last_n = std::min(n, slice);   // the taps describe the last resident slice
    p->last_frames = r.frames;
    p->ws.dbg_valid = p->debug && !r.heads;   // (a heads batch runs no k_cluster of its own: the guess / mean-shift taps are not its)
    return DH_OK;
}

// n frames of w x h in ws.frames
static int ensure_frame_staging(dh_predictor *p, int n, int w, int h) {
    const size_t px = (size_t)n * w * h;
    if (px <= p->ws.frames.cap()) return DH_OK;
    HIP_TRY(hipStreamSynchronize(p->own_stream));
    HIP_TRY(hipStreamSynchronize(p->copy_stream));
    return p->ws.frames.alloc(px);
}
static int stage_frames(dh_predictor *p, const uint16_t *frames, int n, int w, int h) {
    TRY(ensure_frame_staging(p, n, w, h));
    HIP_TRY(hipMemcpyAsync(p->ws.frames.get(), frames, (size_t)n * w * h * sizeof(uint16_t), hipMemcpyHostToDevice, p->own_stream));
    return DH_OK;
}

// The small host arrays of a slice (guesses and their mask in; poses, support records and heads out: download) cross PCIe
// through the predictor's OWN page-locked staging blocks: the caller's arrays are ordinary pageable memory a few hundred bytes
// long, typically sharing their pages with other allocations of other host threads, and handing such ranges to the runtime's
// pageable-copy path (pin the pages, DMA, unpin -- per copy, beside other threads doing the same to neighbouring bytes) is both
// slower than a pinned copy and the one place where concurrent predictors met inside the runtime.  Layout for m frames of the
// inbound block: rot guesses | mid guesses | mask.
struct SmallStage {
    double *rot; float *midp; uint8_t *mask;
};
static int small_stage(dh_predictor *p, int m, SmallStage *st) {
    const size_t need = (size_t)m * (3 * sizeof(double) + 3 * sizeof(float) + 1) + 64;
    TRY(p->pin_small.grow(need));      // (only between slices: both streams are idle)
    st->rot = (double *)p->pin_small.get();
    st->midp = (float *)(st->rot + (size_t)m * 3);
    st->mask = (uint8_t *)(st->midp + (size_t)m * 3);
    return DH_OK;
}
// count elements of the workspace's src -> the outbound staging block on s, wait, -> the caller's dst
template <typename T>
static int download(dh_predictor *p, T *dst, const T *src, size_t count, hipStream_t s) {
    TRY(p->pin_out.grow(count * sizeof(T)));
    HIP_TRY(hipMemcpyAsync(p->pin_out.get(), src, count * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(dst, p->pin_out.get(), count * sizeof(T));
    return DH_OK;
}

// Per-slice setup of the host entry points for slice sl (host arrays): the workspace, the output scratch sl asks for and the frame
// staging for its sl.n frames of sl.w x sl.h, and its guesses through the pinned staging block into the workspace on own_stream.
// *d is sl on those device buffers; its frames (ws.frames) are the caller's to fill.
static int slice_setup(dh_predictor *p, const BatchReq &sl, BatchReq *d) {
    const int m = sl.n;
    TRY(reserve_req(p, sl, m));
    TRY(ensure_frame_staging(p, m, sl.w, sl.h));
    SmallStage st;
    TRY(small_stage(p, m, &st));
    const Workspace &ws = p->ws;
    hipStream_t s = p->own_stream;
    *d = sl;
    d->frames = ws.frames.get();
    d->out = sl.out ? ws.poses.get() : nullptr;
    d->support = sl.support ? ws.sup.get() : nullptr;
    d->heads = sl.heads ? ws.hd_out.get() : nullptr;
    d->n_heads = sl.heads ? ws.hd_n.get() : nullptr;
    if (sl.midp) {
        memcpy(st.midp, sl.midp, (size_t)m * 3 * sizeof(float));
        HIP_TRY(hipMemcpyAsync(ws.midp.get(), st.midp, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, s));
        d->midp = ws.midp.get();
    }
    if (sl.rot) {
        memcpy(st.rot, sl.rot, (size_t)m * 3 * sizeof(double));
        HIP_TRY(hipMemcpyAsync(ws.rot.get(), st.rot, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        d->rot = ws.rot.get();
    }
    if (sl.mask) {
        memcpy(st.mask, sl.mask, (size_t)m);
        HIP_TRY(hipMemcpyAsync(ws.mask.get(), st.mask, (size_t)m, hipMemcpyHostToDevice, s));
        d->mask = ws.mask.get();
    }
    return DH_OK;
}
// Chunk [c0, c0 + cm) of a staged slice d (slice_setup) on stream s.
static int predict_staged(dh_predictor *p, const BatchReq &d, int c0, int cm, hipStream_t s) {
    BatchReq c = d.at(c0);
    c.n = cm;
    return batch_device(p, c, s);
}
// The slice loop of the host entry points: enqueue(f0, sl) stages slice sl = r.at(f0) of the request (slice_setup) and enqueues
// its prediction on own_stream; then each output r asks for -- poses, support records, heads and their counts -- comes back in
// one copy.  With the taps on, the whole batch is one slice (heads keep their resident slices: their taps are not kept).
template <typename F>
static int host_slices(dh_predictor *p, const BatchReq &r, F enqueue) {
    const int n = r.n, slice = p->debug && !r.heads ? n : std::min(n, max_resident_frames(p));
    const Workspace &ws = p->ws;
    hipStream_t s = p->own_stream;
    for (int f0 = 0; f0 < n; f0 += slice) {
        BatchReq sl = r.at(f0);
        sl.n = std::min(slice, n - f0);
        int rc = enqueue(f0, sl);
        if (rc == DH_OK && sl.out) rc = download(p, sl.out, ws.poses.get(), sl.n, s);
        if (rc == DH_OK && sl.support) rc = download(p, sl.support, ws.sup.get(), sl.n, s);
        if (rc == DH_OK && sl.heads) rc = download(p, sl.heads, ws.hd_out.get(), (size_t)sl.n * sl.max_heads, s);
        if (rc == DH_OK && sl.heads) rc = download(p, sl.n_heads, ws.hd_n.get(), sl.n, s);
        if (rc) return rc;
    }
    return DH_OK;
}

// Host batch of frames.  The frames cross PCIe in chunks on copy_stream while the kernels of the previous chunk run on
// own_stream (the path is PCIe-bound: 614 KB per frame in, 40 bytes out), so a batch takes about its upload time plus
// the kernels of the last chunk.  A heads batch uploads each slice in one copy.
static int batch_host(dh_predictor *p, const BatchReq &r) {
    hipStream_t s = p->own_stream, cs = p->copy_stream;
    const size_t fpx = (size_t)r.w * r.h;
    return host_slices(p, r, [&](int, const BatchReq &sl) -> int {
        BatchReq d;
        TRY(slice_setup(p, sl, &d));
        const int m = sl.n;
        // the parity taps describe ONE device batch: with them on, the slice is a single chunk
        int cstart[DH_STAGE_EVENTS + 1];
        const int nchunks = dh_chunk_plan_(m, p->knobs.stage_chunk, p->debug || sl.heads, cstart);
        if (nchunks == 1) {
            // latency path (single frames, small batches): one copy on the compute stream itself
            HIP_TRY(hipMemcpyAsync(p->ws.frames.get(), sl.frames, (size_t)m * fpx * sizeof(uint16_t), hipMemcpyHostToDevice, s));
            int rc = predict_staged(p, d, 0, m, s);
            if (rc) { (void)hipStreamSynchronize(s); return rc; }
        } else {
            // Chunk k + 1 is uploaded on copy_stream while the kernels of chunk k run on own_stream.  From page-locked host
            // memory (dh_host_alloc, or any buffer the caller registered with HIP) the copies are true asynchronous DMA and
            // the whole batch takes its PCIe time; from pageable memory each copy is issued synchronously (the runtime pins,
            // copies, unpins), which still overlaps the kernels but not the next chunk's preparation.
            // (Measured and rejected: three host threads issuing the pageable chunk copies on three streams -- 60-82 k frames/s,
            // erratic, against 80 k from this one thread: the pinning of the pages serialises in the driver.)
            HIP_TRY(hipStreamWaitEvent(cs, p->ev_slice, 0));          // the previous slice's kernels have read the staging buffer
            for (int k = 0; k < nchunks; ++k) {
                const int c0 = cstart[k], cm = cstart[k + 1] - c0;
                HIP_TRY(hipMemcpyAsync(p->ws.frames.get() + (size_t)c0 * fpx, sl.frames + (size_t)c0 * fpx, (size_t)cm * fpx * sizeof(uint16_t), hipMemcpyHostToDevice, cs));
                HIP_TRY(hipEventRecord(p->ev_stage[k], cs));
                HIP_TRY(hipStreamWaitEvent(s, p->ev_stage[k], 0));
                int rc = predict_staged(p, d, c0, cm, s);
                if (rc) { (void)hipStreamSynchronize(cs); (void)hipStreamSynchronize(s); return rc; }
            }
        }
        HIP_TRY(hipEventRecord(p->ev_slice, s));
        return DH_OK;
    });
}

static int predict_batch_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                                 const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                                 dh_pose *out, void *stream_) {
    const BatchReq r{frames, n, w, h, K, {}, midp_guess, rot_guess, guess_mask, out};
    return run(p, r, frames != nullptr, "dh_predict_batch_device", [&] { return batch_device(p, r, (hipStream_t)stream_); });
}
static int predict_batch_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                          const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out) {
    const BatchReq r{frames, n, w, h, K, {}, midp_guess, rot_guess, guess_mask, out};
    return run(p, r, frames != nullptr, "dh_predict_batch", [&] { return batch_host(p, r); });
}

// Page-locked host memory for frame buffers: uploads from it are asynchronous DMA at PCIe speed.
static int host_alloc_(size_t bytes, void **out) {
    if (!out) return fail(DH_EINVAL, "dh_host_alloc: NULL argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) { *out = nullptr; return fail(DH_ENOMEM, "hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    return DH_OK;
}
static int host_free_(void *ptr) {
    if (ptr && hipHostFree(ptr) != hipSuccess) return fail(DH_EHIP, "hipHostFree");
    return DH_OK;
}

// ------------------------------------------------------------------ run-length coded input (BIWI `.bin`, biwi.rs:81-103)
// Validates every payload (dh_rle_plan_), packs blob + run table into pinned memory (dh_rle_pack_) and sizes the device
// buffers.  Nothing has been launched when this fails.
static_assert(sizeof(DhRun) == sizeof(uint2), "run table entries are uint2 on the device");
static int rle_prepare(dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, RlePlan &plan) {
    int rc = dh_rle_plan_(bufs, lens, n, p->knobs.host_threads, plan);
    if (rc) return rc;
    const size_t blob_bytes = plan.blob_off[n];
    TRY(p->pin_begin.grow((size_t)n + 1));
    TRY(p->pin_blob.grow(blob_bytes));
    TRY(p->pin_runs.grow(std::max<size_t>(plan.nruns, 1)));
    TRY(p->dev_blob.grow(blob_bytes));
    TRY(p->dev_runs.grow(std::max<size_t>(plan.nruns, 1)));
    TRY(p->dev_begin.grow((size_t)n + 1));
    memcpy(p->pin_begin.get(), plan.run_begin.data(), ((size_t)n + 1) * sizeof(uint32_t));
    dh_rle_pack_(bufs, lens, n, p->knobs.host_threads, plan, p->pin_blob.get(), (DhRun *)p->pin_runs.get());
    return DH_OK;
}

// Uploads chunk [c0, c0 + cm) of the prepared batch on the copy stream and enqueues its decode into `frames_dev`
// (frame c0 first) on stream s.
static int rle_upload_decode(dh_predictor *p, const std::vector<size_t> &blob_off, int c0, int cm, int ci, uint32_t W, uint32_t H,
                             uint16_t *frames_dev, hipStream_t s) {
    hipStream_t cs = p->copy_stream;
    const size_t b0 = blob_off[c0], b1 = blob_off[c0 + cm];
    const uint32_t r0 = p->pin_begin.get()[c0], r1 = p->pin_begin.get()[c0 + cm];
    HIP_TRY(hipMemcpyAsync(p->dev_blob.get() + b0, p->pin_blob.get() + b0, b1 - b0, hipMemcpyHostToDevice, cs));
    if (r1 > r0) HIP_TRY(hipMemcpyAsync(p->dev_runs.get() + r0, p->pin_runs.get() + r0, (size_t)(r1 - r0) * sizeof(uint2), hipMemcpyHostToDevice, cs));
    hipEvent_t ev = p->ev_stage[ci % DH_STAGE_EVENTS];
    HIP_TRY(hipEventRecord(ev, cs));
    HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    HIP_TRY(hipMemsetAsync(frames_dev, 0, (size_t)cm * W * H * sizeof(uint16_t), s));          // the empty runs (biwi.rs:90-93)
    RleArgs ra{};
    ra.blob = (const uint16_t *)p->dev_blob.get(); ra.runs = p->dev_runs.get(); ra.run_begin = p->dev_begin.get() + c0;
    // the run table addresses pixels of the whole batch: frame c0 of the chunk is pixel c0 * W * H there
    ra.frames = frames_dev - (size_t)c0 * W * H; ra.n_frames = cm;
    const uint32_t per_frame = (r1 - r0 + (uint32_t)cm - 1) / (uint32_t)cm;
    ra.blocks_per_frame = (int)std::max(1u, std::min(64u, (per_frame + 15) / 16));
    HIP_TRY(dh_launch_rle_decode(ra, s));
    return DH_OK;
}

static int biwi_decode_depth_device_(dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, uint16_t *frames_dev,
                                           size_t cap_px, uint32_t *w, uint32_t *h) {
    if (!p || !bufs || !lens || !w || !h) return fail(DH_EINVAL, "dh_biwi_decode_depth_device: NULL argument");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipStreamSynchronize(p->own_stream));             // the pinned staging buffers are free
    HIP_TRY(hipStreamSynchronize(p->copy_stream));
    RlePlan plan;
    int rc = rle_prepare(p, bufs, lens, n, plan);
    if (rc) return rc;
    const std::vector<size_t> &blob_off = plan.blob_off;
    const uint32_t W = plan.W, H = plan.H;
    *w = W; *h = H;
    if (!frames_dev) return DH_OK;                            // size query (validates as well)
    if (cap_px < (size_t)n * W * H) return fail(DH_EINVAL, "output holds %zu pixels, the batch has %zu", cap_px, (size_t)n * W * H);
    HIP_TRY(hipMemcpyAsync(p->dev_begin.get(), p->pin_begin.get(), ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p->own_stream));
    const int chunk = std::min(n, p->knobs.stage_chunk * 2);
    int ci = 0;
    for (int c0 = 0; c0 < n; c0 += chunk, ++ci) {
        const int cm = std::min(chunk, n - c0);
        rc = rle_upload_decode(p, blob_off, c0, cm, ci, W, H, frames_dev + (size_t)c0 * W * H, p->own_stream);
        if (rc) { (void)hipStreamSynchronize(p->copy_stream); (void)hipStreamSynchronize(p->own_stream); return rc; }
    }
    HIP_TRY(hipStreamSynchronize(p->own_stream));
    return DH_OK;
}

// The host batch of payloads: per resident slice the payloads are validated and packed, then decoded chunk by chunk into the
// frame staging, each chunk predicted as it lands.  The frame size is the slice's decoded one.
static int rle_host(dh_predictor *p, const BatchReq &r, const uint8_t *const *bufs, const size_t *lens) {
    hipStream_t s = p->own_stream;
    return host_slices(p, r, [&](int f0, BatchReq sl) -> int {
        HIP_TRY(hipStreamSynchronize(s));                         // pinned staging and device blob of the previous slice are free
        HIP_TRY(hipStreamSynchronize(p->copy_stream));
        const int m = sl.n;
        RlePlan plan;
        TRY(rle_prepare(p, bufs + f0, lens + f0, m, plan));       // validates: nothing launched on failure
        const uint32_t W = plan.W, H = plan.H;
        sl.w = (int)W; sl.h = (int)H;
        BatchReq d;
        TRY(slice_setup(p, sl, &d));
        HIP_TRY(hipMemcpyAsync(p->dev_begin.get(), p->pin_begin.get(), ((size_t)m + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        const int chunk = p->debug ? m : std::min(m, p->knobs.stage_chunk * 2);   // compressed chunks are small: twice the raw chunk
        int ci = 0;
        for (int c0 = 0; c0 < m; c0 += chunk, ++ci) {
            const int cm = std::min(chunk, m - c0);
            int rc = rle_upload_decode(p, plan.blob_off, c0, cm, ci, W, H, p->ws.frames.get() + (size_t)c0 * W * H, s);
            if (rc == DH_OK) rc = predict_staged(p, d, c0, cm, s);
            if (rc) { (void)hipStreamSynchronize(p->copy_stream); (void)hipStreamSynchronize(s); return rc; }
        }
        return DH_OK;
    });
}
static int predict_batch_rle_(dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, const float K[9],
                              const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out) {
    const BatchReq r{nullptr, n, 0, 0, K, {}, midp_guess, rot_guess, guess_mask, out};     // (frames and their size: rle_host)
    return run(p, r, bufs && lens, "dh_predict_batch_rle", [&] { return rle_host(p, r, bufs, lens); });
}

// ------------------------------------------------------------------ hipGraph capture of one batch
// For launch-bound use (small frames / single frames, BASELINE config 5): the zero-fill and the kernel
// launches (k_boxsum ... k_cluster) of one dh_predict_batch_device call are captured once and replayed with one host call.
static int graph_destroy_(dh_predictor *p) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    drop_graph(p);
    p->graph_stale = false;
    return DH_OK;
}

// Captures driver() -- one device batch of r's size on own_stream -- into the predictor's graph slot, replacing what it held: no
// taps or profiling, every allocation r asks for (reserve_req) before the capture starts, refused by dh_graph_launch once the
// workspace is reallocated.
template <typename F>
static int capture(dh_predictor *p, const BatchReq &r, F driver) {
    if (p->debug || p->profiling) return fail(DH_ESTATE, "taps / profiling cannot be captured");
    TRY(reserve_req(p, r, std::min(r.n, max_resident_frames(p))));
    drop_graph(p);
    p->graph_stale = false;
    HIP_TRY(hipStreamSynchronize(p->own_stream));
    HIP_TRY(hipStreamBeginCapture(p->own_stream, hipStreamCaptureModeThreadLocal));
    p->capturing = true;
    const int rc = driver();
    p->capturing = false;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(p->own_stream, &g);
    if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(DH_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    p->graph = g;
    HIP_TRY(hipGraphInstantiate(&p->graph_exec, p->graph, nullptr, nullptr, 0));
    return DH_OK;
}
static int graph_capture_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                          const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out) {
    if (n == 0) return fail(DH_EINVAL, "dh_graph_capture: batch size must be positive");
    const BatchReq r{frames, n, w, h, K, {}, midp_guess, rot_guess, guess_mask, out};
    return run(p, r, frames != nullptr, "dh_graph_capture", [&] { return capture(p, r, [&] { return batch_device(p, r, p->own_stream); }); });
}

static int graph_launch_(dh_predictor *p, void *stream) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    if (p->graph_stale) return fail(DH_ESTATE, "the captured batch is stale: the workspace was reallocated after dh_graph_capture (larger batch, other frame size or debug taps); capture again");
    if (!p->graph_exec) return fail(DH_ESTATE, "no captured batch (dh_graph_capture)");
    DeviceGuard guard(p->device);      // (stream 0: the null stream of the predictor's device, where the graph was captured)
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipGraphLaunch(p->graph_exec, (hipStream_t)stream));
    return DH_OK;
}

// ------------------------------------------------------------------ camera batches and live tracking
static int cameras_create_(const float *K, int n, int device, dh_cameras **out) {
    if (!K || !out) return fail(DH_EINVAL, "dh_cameras_create: NULL argument");
    *out = nullptr;
    if (n <= 0) return fail(DH_EINVAL, "dh_cameras_create: n = %d, expected at least one camera", n);
    std::unique_ptr<dh_cameras> c(new dh_cameras);
    c->device = device; c->n = n;
    c->host.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        DhCam &r = c->host[(size_t)i];
        memset(&r, 0, sizeof r);
        memcpy(r.k, K + (size_t)i * 9, sizeof r.k);
        dh_mat3_inv_f32_(r.k, r.kinv);      // IntrinsicMatrix::inv (types.rs:436-441), as every single-K batch
        r.pin = r.k[1] == 0.0f && r.k[3] == 0.0f && r.k[6] == 0.0f && r.k[7] == 0.0f && r.k[8] == 1.0f ? 1u : 0u;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    TRY(c->dev.alloc((size_t)n));
    HIP_TRY(hipMemcpy(c->dev.get(), c->host.data(), (size_t)n * sizeof(DhCam), hipMemcpyHostToDevice));
    *out = c.release();
    return DH_OK;
}
static int cameras_destroy_(dh_cameras *c) {
    if (!c) return DH_OK;
    DeviceGuard guard(c->device);      // (the buffer is freed on its device)
    delete c;
    return DH_OK;
}
static int predict_batch_cameras_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                         const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out, void *stream) {
    const BatchReq r{frames, n, w, h, nullptr, {c, 0}, midp_guess, rot_guess, guess_mask, out};
    return run(p, r, frames != nullptr, "dh_predict_batch_cameras_device", [&] { return batch_device(p, r, (hipStream_t)stream); });
}
static int predict_batch_cameras_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                  const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out) {
    const BatchReq r{frames, n, w, h, nullptr, {c, 0}, midp_guess, rot_guess, guess_mask, out};
    return run(p, r, frames != nullptr, "dh_predict_batch_cameras", [&] { return batch_host(p, r); });
}

// The host steps of tracker t: each resident slice of cameras [f0, f0 + m) stages its frames and its present bytes (into
// t->present), then enqueue(d, present) runs the step on own_stream, d being the slice on device buffers and present the staged
// bytes of the whole table or NULL.  after(f0, m) then copies back what the tracker reports beyond host_slices' own outputs.
template <typename E, typename A>
static int track_slices(dh_predictor *p, TrackerCore *t, const BatchReq &r, const uint8_t *present, E enqueue, A after) {
    hipStream_t s = p->own_stream;
    return host_slices(p, r, [&](int f0, const BatchReq &sl) -> int {
        BatchReq d;
        TRY(slice_setup(p, sl, &d));
        const int m = sl.n;
        HIP_TRY(hipMemcpyAsync(p->ws.frames.get(), sl.frames, (size_t)m * sl.w * sl.h * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        if (present) {
            SmallStage st;
            TRY(small_stage(p, m, &st));       // (the slice's guess-mask staging: a tracker step takes no host guesses)
            memcpy(st.mask, present + f0, (size_t)m);
            HIP_TRY(hipMemcpyAsync(t->present.get() + f0, st.mask, (size_t)m, hipMemcpyHostToDevice, s));
        }
        int rc = enqueue(d, present ? t->present.get() : nullptr);
        if (rc) { (void)hipStreamSynchronize(s); return rc; }
        HIP_TRY(hipEventRecord(p->ev_slice, s));
        return after(f0, m);
    });
}

// A tracker's state is exactly the guess arrays of a camera batch (midp_guess, rot_guess, guess_mask): a step predicts with them
// and k_track then rewrites them from the step's poses (dh_track.h: live_prediction.rs:79-101).
struct dh_tracker : TrackerCore {
    uint32_t flags = 0;
    Buf<float> midp;         // [n][3]
    Buf<double> rot;         // [n][3]
    Buf<uint8_t> mask;       // [n] bit0 midpoint guess, bit1 rotation guess
    Buf<uint8_t> has_rot;    // [n]
    // live_prediction.rs:63-64: latest_midp = [0, 0, 0], latest_rot = None
    int clear(size_t c0, size_t m, hipStream_t s) {
        HIP_TRY(hipMemsetAsync(midp.get() + c0 * 3, 0, m * 3 * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(rot.get() + c0 * 3, 0, m * 3 * sizeof(double), s));
        HIP_TRY(hipMemsetAsync(mask.get() + c0, 0, m, s));
        HIP_TRY(hipMemsetAsync(has_rot.get() + c0, 0, m, s));
        return DH_OK;
    }
};
static int tracker_create_(const dh_cameras *c, uint32_t flags, dh_tracker **out) {
    if (!c || !out) return fail(DH_EINVAL, "dh_tracker_create: NULL argument");
    *out = nullptr;
    if (flags & ~(DH_TRACK_PREV_GUESS | DH_TRACK_SLUGGISH)) return fail(DH_EINVAL, "dh_tracker_create: unknown flags 0x%x", flags);
    return create_tracker(c, out, [&](dh_tracker &t, size_t n) -> int {
        t.flags = flags;
        TRY(t.midp.alloc(n * 3));
        TRY(t.rot.alloc(n * 3));
        TRY(t.mask.alloc(n));
        return t.has_rot.alloc(n);
    });
}
static int tracker_destroy_(dh_tracker *t) { return destroy_tracker(t); }
static int tracker_reset_(dh_tracker *t, int camera, void *stream) { return reset_tracker(t, camera, stream, "dh_tracker_reset"); }
// A step's request: every camera of the tracker (a NULL tracker leaves the camera table NULL: check_req refuses it), poses into
// `out`; track_enqueue supplies the guesses.
static BatchReq track_req(const dh_tracker *t, const uint16_t *frames, int w, int h, dh_pose *out) {
    BatchReq r{frames, t ? t->n : 0, w, h, nullptr, {t ? t->cams : nullptr, 0}};
    r.out = out;
    return r;
}
// Cameras [c0, c0 + r.n) of a step (r on device buffers, c0 = r.cams.c0): their batch with the tracker's guesses, then k_track
// over their poses, both on stream s.  present is the array of the whole camera table (nullable).  k_track reads no support.
static int track_enqueue(dh_predictor *p, dh_tracker *t, BatchReq r, const uint8_t *present, hipStream_t s) {
    const size_t c0 = (size_t)r.cams.c0;
    r.midp = t->midp.get() + c0 * 3; r.rot = t->rot.get() + c0 * 3; r.mask = t->mask.get() + c0;
    TRY(batch_device(p, r, s));
    TrackArgs a{};
    a.poses = r.out; a.present = off(present, c0); a.n = r.n; a.flags = t->flags;
    a.midp = t->midp.get() + c0 * 3; a.rot = t->rot.get() + c0 * 3; a.mask = t->mask.get() + c0; a.has_rot = t->has_rot.get() + c0;
    { Range rg(p->profiling, "dh:track"); HIP_TRY(dh_launch_track(a, s)); }
    return DH_OK;
}
// The host steps: k_track after each slice's batch, nothing copied back beyond the poses (and support records).
static int track_host(dh_predictor *p, dh_tracker *t, const BatchReq &r, const uint8_t *present) {
    return track_slices(p, t, r, present, [&](const BatchReq &d, const uint8_t *pr) { return track_enqueue(p, t, d, pr, p->own_stream); },
                        [](int, int) { return DH_OK; });
}
static int tracker_step_device_(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out,
                                void *stream) {
    const BatchReq r = track_req(t, frames, w, h, out);
    return run(p, r, frames != nullptr, "dh_tracker_step_device", [&] { return track_enqueue(p, t, r, present, (hipStream_t)stream); });
}
static int tracker_step_(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out) {
    const BatchReq r = track_req(t, frames, w, h, out);
    return run(p, r, frames != nullptr, "dh_tracker_step", [&] { return track_host(p, t, r, present); });
}
static int tracker_state_(dh_tracker *t, float *midp, double *rot, uint8_t *flags) {
    return read_tracker(t, "dh_tracker_state", [&](size_t n) -> int {
        if (midp) HIP_TRY(hipMemcpy(midp, t->midp.get(), n * 3 * sizeof(float), hipMemcpyDeviceToHost));
        if (rot) HIP_TRY(hipMemcpy(rot, t->rot.get(), n * 3 * sizeof(double), hipMemcpyDeviceToHost));
        if (flags) {
            std::vector<uint8_t> hr(n);
            HIP_TRY(hipMemcpy(flags, t->mask.get(), n, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(hr.data(), t->has_rot.get(), n, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) flags[i] = (uint8_t)(flags[i] | (hr[i] ? 4u : 0u));
        }
        return DH_OK;
    });
}
// One device step captured into the predictor's graph slot (capture).
static int tracker_capture_(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out) {
    const BatchReq r = track_req(t, frames, w, h, out);
    return run(p, r, frames != nullptr, "dh_tracker_capture", [&] { return capture(p, r, [&] { return track_enqueue(p, t, r, present, p->own_stream); }); });
}

// ------------------------------------------------------------------ vote support
// The *_support twins of the batch, camera and tracker calls: the same request with k_emit's SUP instance and k_support
// appended, one dh_support per frame.
static int predict_batch_support_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess,
                                  const double *rot_guess, const uint8_t *guess_mask, uint32_t radius, dh_pose *out, dh_support *support) {
    const BatchReq r{frames, n, w, h, K, {}, midp_guess, rot_guess, guess_mask, out, SUPPORT, radius, support};
    return run(p, r, frames != nullptr, "dh_predict_batch_support", [&] { return batch_host(p, r); });
}
static int predict_batch_support_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                                         const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius,
                                         dh_pose *out, dh_support *support, void *stream) {
    const BatchReq r{frames, n, w, h, K, {}, midp_guess, rot_guess, guess_mask, out, SUPPORT, radius, support};
    return run(p, r, frames != nullptr, "dh_predict_batch_support_device", [&] { return batch_device(p, r, (hipStream_t)stream); });
}
static int predict_batch_cameras_support_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                          const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius,
                                          dh_pose *out, dh_support *support) {
    const BatchReq r{frames, n, w, h, nullptr, {c, 0}, midp_guess, rot_guess, guess_mask, out, SUPPORT, radius, support};
    return run(p, r, frames != nullptr, "dh_predict_batch_cameras_support", [&] { return batch_host(p, r); });
}
static int predict_batch_cameras_support_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                                 const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                                                 uint32_t radius, dh_pose *out, dh_support *support, void *stream) {
    const BatchReq r{frames, n, w, h, nullptr, {c, 0}, midp_guess, rot_guess, guess_mask, out, SUPPORT, radius, support};
    return run(p, r, frames != nullptr, "dh_predict_batch_cameras_support_device", [&] { return batch_device(p, r, (hipStream_t)stream); });
}
static int tracker_step_support_(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                 uint32_t radius, dh_pose *out, dh_support *support) {
    BatchReq r = track_req(t, frames, w, h, out);
    r.kind = SUPPORT; r.radius = radius; r.support = support;
    return run(p, r, frames != nullptr, "dh_tracker_step_support", [&] { return track_host(p, t, r, present); });
}
static int tracker_step_support_device_(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                        uint32_t radius, dh_pose *out, dh_support *support, void *stream) {
    BatchReq r = track_req(t, frames, w, h, out);
    r.kind = SUPPORT; r.radius = radius; r.support = support;
    return run(p, r, frames != nullptr, "dh_tracker_step_support_device", [&] { return track_enqueue(p, t, r, present, (hipStream_t)stream); });
}

// ------------------------------------------------------------------ several heads per frame
// n_heads [n] and heads [n][max_heads] in place of the poses.
static int predict_heads_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads, uint32_t radius,
                          uint32_t *n_heads, dh_head *heads) {
    BatchReq r{frames, n, w, h, K};
    r.kind = HEADS; r.radius = radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = max_heads;
    return run(p, r, frames != nullptr, "dh_predict_heads", [&] { return batch_host(p, r); });
}
static int predict_heads_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads,
                                 uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream) {
    BatchReq r{frames, n, w, h, K};
    r.kind = HEADS; r.radius = radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = max_heads;
    return run(p, r, frames != nullptr, "dh_predict_heads_device", [&] { return batch_device(p, r, (hipStream_t)stream); });
}
static int predict_heads_cameras_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads,
                                  uint32_t radius, uint32_t *n_heads, dh_head *heads) {
    BatchReq r{frames, n, w, h, nullptr, {c, 0}};
    r.kind = HEADS; r.radius = radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = max_heads;
    return run(p, r, frames != nullptr, "dh_predict_heads_cameras", [&] { return batch_host(p, r); });
}
static int predict_heads_cameras_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads,
                                         uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream) {
    BatchReq r{frames, n, w, h, nullptr, {c, 0}};
    r.kind = HEADS; r.radius = radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = max_heads;
    return run(p, r, frames != nullptr, "dh_predict_heads_cameras_device", [&] { return batch_device(p, r, (hipStream_t)stream); });
}

// ------------------------------------------------------------------ several heads per camera with identities
// A multi-head tracker's state: DH_MAX_TRACKS track records and the next id per camera.  A step is a heads camera batch followed
// by k_track_heads (dh_track_heads.h) over its heads.
struct dh_multi_tracker : TrackerCore {
    dh_multi_track_params prm{};
    Buf<dh_head_track> tracks;   // [n][DH_MAX_TRACKS]
    Buf<uint32_t> next_id;       // [n]
    Buf<uint32_t> ids;           // [n][max_heads] host steps: the ids before their copy back
    // tracks zeroed, next ids 1
    int clear(size_t c0, size_t m, hipStream_t s) {
        HIP_TRY(hipMemsetAsync(tracks.get() + c0 * DH_MAX_TRACKS, 0, m * DH_MAX_TRACKS * sizeof(dh_head_track), s));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(next_id.get() + c0), 1, m, s));
        return DH_OK;
    }
};
static int multi_params_check(const dh_multi_track_params *prm, const char *fn) {
    if (prm->max_heads < 1 || prm->max_heads > DH_MAX_HEADS)
        return fail(DH_EINVAL, "%s: max_heads %d outside 1 .. %d", fn, prm->max_heads, DH_MAX_HEADS);
    if (prm->radius > 0x7fffffffu) return fail(DH_EINVAL, "%s: radius %u (a negative int?); expected 0 .. 2^31 - 1", fn, prm->radius);
    if (prm->gate > 0x7fffffffu) return fail(DH_EINVAL, "%s: gate %u (a negative int?); expected 0 .. 2^31 - 1", fn, prm->gate);
    return DH_OK;
}
static int multi_tracker_create_(const dh_cameras *c, const dh_multi_track_params *prm, dh_multi_tracker **out) {
    if (!prm || !out) return fail(DH_EINVAL, "dh_multi_tracker_create: NULL argument");
    *out = nullptr;
    TRY(multi_params_check(prm, "dh_multi_tracker_create"));
    if (!c) return fail(DH_EINVAL, "dh_multi_tracker_create: NULL camera table");
    return create_tracker(c, out, [&](dh_multi_tracker &t, size_t n) -> int {
        t.prm = *prm;
        TRY(t.tracks.alloc(n * DH_MAX_TRACKS));
        TRY(t.next_id.alloc(n));
        return t.ids.alloc(n * (size_t)prm->max_heads);
    });
}
static int multi_tracker_destroy_(dh_multi_tracker *t) { return destroy_tracker(t); }
static int multi_tracker_reset_(dh_multi_tracker *t, int camera, void *stream) { return reset_tracker(t, camera, stream, "dh_multi_tracker_reset"); }
// A step's request: a heads camera batch of every camera of the tracker with its max_heads and radius.
static BatchReq multi_track_req(const dh_multi_tracker *t, const uint16_t *frames, int w, int h, uint32_t *n_heads, dh_head *heads) {
    BatchReq r{frames, t->n, w, h, nullptr, {t->cams, 0}};
    r.kind = HEADS; r.radius = t->prm.radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = t->prm.max_heads;
    return r;
}
// Cameras [c0, c0 + r.n) of a step (r on device buffers, c0 = r.cams.c0): their heads batch, then k_track_heads over their heads,
// both on stream s.  present, ids and tracks are the arrays of the whole camera table (present and tracks nullable).
static int multi_track_enqueue(dh_predictor *p, dh_multi_tracker *t, const BatchReq &r, const uint8_t *present, uint32_t *ids,
                               dh_head_track *tracks, hipStream_t s) {
    const size_t c0 = (size_t)r.cams.c0;
    TRY(batch_device(p, r, s));
    TrackHeadsArgs a{};
    a.heads = r.heads; a.n_heads = r.n_heads; a.present = off(present, c0);
    a.state = t->tracks.get() + c0 * DH_MAX_TRACKS; a.next_id = t->next_id.get() + c0;
    a.ids = ids + c0 * (size_t)r.max_heads; a.snapshot = off(tracks, c0 * DH_MAX_TRACKS);
    a.n = r.n; a.max_heads = r.max_heads; a.gate = t->prm.gate; a.max_misses = t->prm.max_misses;
    { Range rg(p->profiling, "dh:track_heads"); HIP_TRY(dh_launch_track_heads(a, s)); }
    return DH_OK;
}
static int multi_tracker_step_device_(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                      uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks, void *stream) {
    if (!t || !ids) return fail(DH_EINVAL, "dh_multi_tracker_step_device: NULL argument");
    const BatchReq r = multi_track_req(t, frames, w, h, n_heads, heads);
    return run(p, r, frames != nullptr, "dh_multi_tracker_step_device",
               [&] { return multi_track_enqueue(p, t, r, present, ids, tracks, (hipStream_t)stream); });
}
static int multi_tracker_step_(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                               uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks) {
    if (!t || !ids) return fail(DH_EINVAL, "dh_multi_tracker_step: NULL argument");
    const BatchReq r = multi_track_req(t, frames, w, h, n_heads, heads);
    const size_t mh = (size_t)r.max_heads;
    return run(p, r, frames != nullptr, "dh_multi_tracker_step", [&] {
        hipStream_t s = p->own_stream;
        auto enqueue = [&](const BatchReq &d, const uint8_t *pr) { return multi_track_enqueue(p, t, d, pr, t->ids.get(), nullptr, s); };
        // the ids and track records of cameras [f0, f0 + m), after their kernels and before host_slices' copies of their heads
        auto after = [&](int f0, int m) -> int {
            TRY(download(p, ids + (size_t)f0 * mh, t->ids.get() + (size_t)f0 * mh, (size_t)m * mh, s));
            if (tracks) TRY(download(p, tracks + (size_t)f0 * DH_MAX_TRACKS, t->tracks.get() + (size_t)f0 * DH_MAX_TRACKS, (size_t)m * DH_MAX_TRACKS, s));
            return DH_OK;
        };
        return track_slices(p, t, r, present, enqueue, after);
    });
}
static int multi_tracker_state_(dh_multi_tracker *t, dh_head_track *tracks, uint32_t *next_id) {
    return read_tracker(t, "dh_multi_tracker_state", [&](size_t n) -> int {
        if (tracks) HIP_TRY(hipMemcpy(tracks, t->tracks.get(), n * DH_MAX_TRACKS * sizeof(dh_head_track), hipMemcpyDeviceToHost));
        if (next_id) HIP_TRY(hipMemcpy(next_id, t->next_id.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
// One device step captured into the predictor's graph slot (capture).
static int multi_tracker_capture_(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                  uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks) {
    if (!t || !ids) return fail(DH_EINVAL, "dh_multi_tracker_capture: NULL argument");
    const BatchReq r = multi_track_req(t, frames, w, h, n_heads, heads);
    return run(p, r, frames != nullptr, "dh_multi_tracker_capture",
               [&] { return capture(p, r, [&] { return multi_track_enqueue(p, t, r, present, ids, tracks, p->own_stream); }); });
}

// ------------------------------------------------------------------ camera rigs
static int rig_create_(const dh_cameras *c, const float *R, const float *t, const int32_t *rig_begin, int n_rigs, dh_rig **out) {
    if (!out) return fail(DH_EINVAL, "dh_rig_create: NULL argument");
    *out = nullptr;
    if (!c || !R || !t || !rig_begin) return fail(DH_EINVAL, "dh_rig_create: NULL argument");
    if (n_rigs < 1) return fail(DH_EINVAL, "dh_rig_create: n_rigs = %d, expected at least one rig", n_rigs);
    if (rig_begin[0] != 0 || rig_begin[n_rigs] != c->n)
        return fail(DH_EINVAL, "dh_rig_create: the rigs cover cameras %d .. %d, the camera table has 0 .. %d", rig_begin[0], rig_begin[n_rigs], c->n);
    for (int g = 0; g < n_rigs; ++g) {
        const int64_t m = (int64_t)rig_begin[g + 1] - rig_begin[g];
        if (m < 1 || m > DH_RIG_MAX_CAMERAS)
            return fail(DH_EINVAL, "dh_rig_create: rig %d has %lld cameras, expected 1 .. %d in ascending ranges", g, (long long)m, DH_RIG_MAX_CAMERAS);
    }
    std::vector<RigCam> host((size_t)c->n);
    for (int i = 0; i < c->n; ++i) {
        memcpy(host[(size_t)i].R, R + (size_t)i * 9, sizeof host[0].R);
        memcpy(host[(size_t)i].t, t + (size_t)i * 3, sizeof host[0].t);
        for (int q = 0; q < 12; ++q)
            if (!std::isfinite(q < 9 ? host[(size_t)i].R[q] : host[(size_t)i].t[q - 9]))
                return fail(DH_EINVAL, "dh_rig_create: camera %d has a non-finite entry in %s", i, q < 9 ? "R" : "t");
    }
    DeviceGuard guard(c->device);
    if (!guard.ok) return DH_EHIP;
    std::unique_ptr<dh_rig> r(new dh_rig);
    r->cams = c; r->n_rigs = n_rigs;
    for (int g = 0; g < n_rigs; ++g) r->largest = std::max(r->largest, (int)(rig_begin[g + 1] - rig_begin[g]));
    TRY(r->dev.alloc((size_t)c->n));
    TRY(r->rig_begin.alloc((size_t)n_rigs + 1));
    HIP_TRY(hipMemcpy(r->dev.get(), host.data(), host.size() * sizeof(RigCam), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(r->rig_begin.get(), rig_begin, ((size_t)n_rigs + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = r.release();
    return DH_OK;
}
static int rig_destroy_(dh_rig *r) {
    if (!r) return DH_OK;
    DeviceGuard guard(r->cams->device);
    delete r;
    return DH_OK;
}

static int rig_tracker_create_(const dh_rig *rig, const dh_rig_track_params *prm, dh_rig_tracker **out) {
    const char *fn = "dh_rig_tracker_create";
    if (!prm || !out) return fail(DH_EINVAL, "%s: NULL argument", fn);
    *out = nullptr;
    if (prm->max_heads < 1 || prm->max_heads > DH_MAX_HEADS) return fail(DH_EINVAL, "%s: max_heads %d outside 1 .. %d", fn, prm->max_heads, DH_MAX_HEADS);
    if (prm->radius > 0x7fffffffu) return fail(DH_EINVAL, "%s: radius %u (a negative int?); expected 0 .. 2^31 - 1", fn, prm->radius);
    if (prm->fuse_gate > 0x7fffffffu) return fail(DH_EINVAL, "%s: fuse_gate %u (a negative int?); expected 0 .. 2^31 - 1", fn, prm->fuse_gate);
    if (prm->gate > 0x7fffffffu) return fail(DH_EINVAL, "%s: gate %u (a negative int?); expected 0 .. 2^31 - 1", fn, prm->gate);
    if (!rig) return fail(DH_EINVAL, "%s: NULL rig table", fn);
    const size_t ng = (size_t)rig->n_rigs, mh = (size_t)prm->max_heads;
    return create_tracker(rig->cams, out, [&](dh_rig_tracker &t, size_t n) -> int {
        t.rig = rig; t.prm = *prm;
        TRY(t.tracks.alloc(ng * DH_RIG_MAX_TRACKS));
        TRY(t.next_id.alloc(ng));
        TRY(t.heads.alloc(n * mh));
        TRY(t.n_heads.alloc(n));
        TRY(t.ids.alloc(n * mh));
        TRY(t.n_persons.alloc(ng));
        return t.persons.alloc(ng * DH_RIG_MAX_PERSONS);
    }, ng);
}
static int rig_tracker_destroy_(dh_rig_tracker *t) { return destroy_tracker(t); }
static int rig_tracker_reset_(dh_rig_tracker *t, int rig, void *stream) {
    return reset_tracker(t, rig, stream, "dh_rig_tracker_reset", t ? t->rig->n_rigs : 0, "rig");
}
// A step's request: a heads camera batch of every camera of the rig table with the tracker's max_heads and radius.
static BatchReq rig_track_req(const dh_rig_tracker *t, const uint16_t *frames, int w, int h, uint32_t *n_heads, dh_head *heads) {
    BatchReq r{frames, t->n, w, h, nullptr, {t->cams, 0}};
    r.kind = HEADS; r.radius = t->prm.radius; r.heads = heads; r.n_heads = n_heads; r.max_heads = t->prm.max_heads;
    return r;
}
// k_rig_fuse over every rig on stream s: heads, n_heads, present (nullable) and ids are device arrays of the whole camera
// table, n_persons, persons and tracks (nullable) of every rig.
static int rig_fuse_enqueue(dh_predictor *p, dh_rig_tracker *t, const dh_head *heads, const uint32_t *n_heads, const uint8_t *present,
                            uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, hipStream_t s) {
    RigFuseArgs a{};
    a.cams = t->rig->dev.get(); a.rig_begin = t->rig->rig_begin.get();
    a.heads = heads; a.n_heads = n_heads; a.present = present;
    a.state = t->tracks.get(); a.next_id = t->next_id.get();
    a.ids = ids; a.n_persons = n_persons; a.persons = persons; a.snapshot = tracks;
    a.n_rigs = t->rig->n_rigs; a.max_heads = t->prm.max_heads;
    a.fuse_gate = t->prm.fuse_gate; a.gate = t->prm.gate; a.max_misses = t->prm.max_misses;
    { Range rg(p->profiling, "dh:rig_fuse"); HIP_TRY(dh_launch_rig_fuse(a, s)); }
    return DH_OK;
}
// The device step: the heads batch of the whole table (batch_device slices it when it exceeds the resident limit; the heads stay
// in the caller's arrays), then k_rig_fuse, both on stream s.
static int rig_track_enqueue(dh_predictor *p, dh_rig_tracker *t, const BatchReq &r, const uint8_t *present, uint32_t *ids,
                             uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, hipStream_t s) {
    TRY(batch_device(p, r, s));
    return rig_fuse_enqueue(p, t, r.heads, r.n_heads, present, ids, n_persons, persons, tracks, s);
}
static int rig_args_check(const dh_predictor *p, const dh_rig_tracker *t, const void *ids, const void *n_persons, const void *persons, const char *fn) {
    if (!t || !ids || !n_persons || !persons) return fail(DH_EINVAL, "%s: NULL argument", fn);
    if (p && t->cams->device != p->device)
        return fail(DH_EINVAL, "%s: rig table on device %d, predictor on device %d", fn, t->cams->device, p->device);
    return DH_OK;
}
static int rig_tracker_step_device_(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                    uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons,
                                    dh_rig_track *tracks, void *stream) {
    TRY(rig_args_check(p, t, ids, n_persons, persons, "dh_rig_tracker_step_device"));
    const BatchReq r = rig_track_req(t, frames, w, h, n_heads, heads);
    return run(p, r, frames != nullptr, "dh_rig_tracker_step_device",
               [&] { return rig_track_enqueue(p, t, r, present, ids, n_persons, persons, tracks, (hipStream_t)stream); });
}
static int rig_tracker_step_(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                             uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons,
                             dh_rig_track *tracks) {
    TRY(rig_args_check(p, t, ids, n_persons, persons, "dh_rig_tracker_step"));
    const BatchReq r = rig_track_req(t, frames, w, h, n_heads, heads);
    const size_t mh = (size_t)r.max_heads, ng = (size_t)t->rig->n_rigs;
    return run(p, r, frames != nullptr, "dh_rig_tracker_step", [&] {
        hipStream_t s = p->own_stream;
        // a slice's heads pipeline, its heads kept in the tracker's arrays of the whole table
        auto enqueue = [&](const BatchReq &d, const uint8_t *) -> int {
            const size_t c0 = (size_t)d.cams.c0;
            TRY(batch_device(p, d, s));
            HIP_TRY(hipMemcpyAsync(t->heads.get() + c0 * mh, d.heads, (size_t)d.n * mh * sizeof(dh_head), hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(t->n_heads.get() + c0, d.n_heads, (size_t)d.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            return DH_OK;
        };
        // after the last slice: one k_rig_fuse over every rig, and its outputs back
        auto after = [&](int f0, int m) -> int {
            if (f0 + m < t->n) return DH_OK;
            TRY(rig_fuse_enqueue(p, t, t->heads.get(), t->n_heads.get(), present ? t->present.get() : nullptr, t->ids.get(),
                                 t->n_persons.get(), t->persons.get(), nullptr, s));
            TRY(download(p, ids, t->ids.get(), (size_t)t->n * mh, s));
            TRY(download(p, n_persons, t->n_persons.get(), ng, s));
            TRY(download(p, persons, t->persons.get(), ng * DH_RIG_MAX_PERSONS, s));
            if (tracks) TRY(download(p, tracks, t->tracks.get(), ng * DH_RIG_MAX_TRACKS, s));
            return DH_OK;
        };
        return track_slices(p, t, r, present, enqueue, after);
    });
}
static int rig_tracker_state_(dh_rig_tracker *t, dh_rig_track *tracks, uint32_t *next_id) {
    return read_tracker(t, "dh_rig_tracker_state", [&](size_t) -> int {
        const size_t ng = (size_t)t->rig->n_rigs;
        if (tracks) HIP_TRY(hipMemcpy(tracks, t->tracks.get(), ng * DH_RIG_MAX_TRACKS * sizeof(dh_rig_track), hipMemcpyDeviceToHost));
        if (next_id) HIP_TRY(hipMemcpy(next_id, t->next_id.get(), ng * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
// One device step captured into the predictor's graph slot (capture): the tracker's own buffers exist since its creation, so
// the capture allocates nothing beyond what reserve_req covers.
static int rig_tracker_capture_(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons,
                                dh_rig_track *tracks) {
    TRY(rig_args_check(p, t, ids, n_persons, persons, "dh_rig_tracker_capture"));
    const BatchReq r = rig_track_req(t, frames, w, h, n_heads, heads);
    return run(p, r, frames != nullptr, "dh_rig_tracker_capture",
               [&] { return capture(p, r, [&] { return rig_track_enqueue(p, t, r, present, ids, n_persons, persons, tracks, p->own_stream); }); });
}

// ------------------------------------------------------------------ predict_mask / 2-D Hough votes
static int aux_reserve(dh_predictor *p, int n, int w, int h, size_t out_bytes) {
    TRY(reserve(p, n, w, h));
    Workspace &ws = p->ws;
    const size_t cap = ws.cap_frames, npatch = std::max(ws.geom.npatch, 1);
    if (ws.aux_cap < ws.cap_frames || !ws.aux_leaf) {
        HIP_TRY(hipDeviceSynchronize());
        ws.aux_cap = 0;
        TRY(ws.aux_leaf.alloc(cap * npatch * p->n_trees));
        TRY(ws.aux_flags.alloc(cap * npatch));
        TRY(ws.aux_u32.alloc(cap * w * h));
        ws.aux_cap = ws.cap_frames;
    }
    if (out_bytes > ws.aux_out.cap()) {
        HIP_TRY(hipDeviceSynchronize());
        TRY(ws.aux_out.alloc(out_bytes));
    }
    return DH_OK;
}

// Taps of imageproc's gaussian_kernel_f32 (dh_blur_taps_, dh_host.cpp; parity unpinned), uploaded once per sigma.
static int blur_kernel(dh_predictor *p) {
    const float sigma = p->params.gaussian_sigma;
    if (p->blur_kern && p->blur_sigma == sigma) return DH_OK;
    std::vector<float> k;
    TRY(dh_blur_taps_(sigma, k));
    HIP_TRY(hipDeviceSynchronize());
    TRY(p->blur_kern.alloc(k.size()));
    HIP_TRY(hipMemcpy(p->blur_kern.get(), k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice));
    p->blur_klen = (int)k.size(); p->blur_sigma = sigma;
    return DH_OK;
}

enum : unsigned { AUX_MASK = 1, AUX_VOTES = 2, AUX_BLUR = 4, AUX_POSES = 8 };   // what a call produces (poses: from the blurred votes)

// One resident slice of frames: the mask (AUX_MASK) or the vote image into `img`, the 2-D poses into `poses2d`.
static int aux_run(dh_predictor *p, unsigned req, const uint16_t *frames, int n, int w, int h, const float K[9], void *img,
                   dh_pose *poses2d, hipStream_t s) {
    const Workspace &ws = p->ws;
    const Geom &g = ws.geom;
    float kinv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (K) dh_mat3_inv_f32_(K, kinv);
    HIP_TRY(hipMemsetAsync(ws.hit_count(0), 0, (ws.lay.pos_grid - ws.lay.hit_count) * sizeof(uint32_t), s));   // hit counters only
    HIP_TRY(hipMemsetAsync(ws.tile_flags(0), 0, (ws.lay.leaf_hits - ws.lay.tile_flags) * sizeof(uint32_t), s));   // tile flags, window counts
    HIP_TRY(hipMemsetAsync(ws.aux_flags.get(), 0, (size_t)n * std::max(g.npatch, 1), s));
    EnqueueOpts o;
    o.leaf_out = ws.aux_leaf.get(); o.flags_out = ws.aux_flags.get(); o.traverse_only = true;
    TRY(enqueue_range(p, BatchReq{frames, n, w, h, K ? K : kid}, 0, n, s, o));
    AuxArgs a{};
    a.frames = frames; a.n_frames = n; a.w = w; a.h = h;
    a.step = (int)p->params.stepwidth; a.sw = (int)p->params.subimage_width; a.sh = (int)p->params.subimage_height;
    a.lw = a.sw / 2; a.lh = a.sh / 2; a.nx = g.nx; a.ny = g.ny;
    memcpy(a.k, K ? K : kid, sizeof a.k); memcpy(a.kinv, kinv, sizeof a.kinv);
    a.f = p->dev; a.leaf = ws.aux_leaf.get(); a.flags = ws.aux_flags.get();
    if (req & AUX_MASK) {
        HIP_TRY(hipMemsetAsync(img, 0, (size_t)n * w * h, s));          // ImageBuffer::new zero-fills (prediction.rs:852)
        a.mask = (uint8_t *)img;
        HIP_TRY(dh_launch_mask(a, s));
    }
    if (req & AUX_VOTES) {
        uint16_t *hough = (uint16_t *)img;
        HIP_TRY(hipMemsetAsync(ws.aux_u32.get(), 0, (size_t)n * w * h * sizeof(uint32_t), s));
        a.hough32 = ws.aux_u32.get();
        HIP_TRY(dh_launch_hough2d(a, hough, s));
        // gaussian_blur_f32 (prediction.rs:844): horizontal pass into the (now free) 32-bit scratch, vertical pass back
        if (req & AUX_BLUR) HIP_TRY(dh_launch_blur_u16(hough, (uint16_t *)ws.aux_u32.get(), hough, n, w, h, p->blur_kern.get(), p->blur_klen, s));
        if (req & AUX_POSES) HIP_TRY(dh_launch_argmax2d(hough, frames, n, w, h, kinv, poses2d, s));
    }
    p->last_n = 0;   // the pose taps do not refer to this run
    p->ws.list_chunks = 0;
    return DH_OK;
}

// The mask / 2-D Hough calls: `out` holds n masks (u8 per pixel), n vote images (u16 per pixel) or n poses.  The device twins
// run on stream s from and into the caller's buffers.  The host twins stage each slice's frames into ws_frames, run it on
// own_stream into the scratch output (poses: ws_poses), copy that back and wait for it before the next slice.
static int aux_call(dh_predictor *p, const char *fn, unsigned req, const uint16_t *frames, int n, int w, int h, const float K[9],
                    void *out, bool host, hipStream_t s = nullptr) {
    if (!p || !frames || (!K && !(req & AUX_MASK)) || !out) return fail(DH_EINVAL, "%s: NULL argument", fn);
    if (n <= 0) return n == 0 ? DH_OK : fail(DH_EINVAL, "negative batch size");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    int rc = req & AUX_BLUR ? blur_kernel(p) : DH_OK;
    if (rc) return rc;
    if (host) s = p->own_stream;
    const bool poses = req & AUX_POSES;
    const size_t px = (size_t)w * h, opx = req & AUX_MASK ? 1 : sizeof(uint16_t);    // output bytes per pixel
    const int slice = std::min(n, max_resident_frames(p));
    for (int f0 = 0; f0 < n; f0 += slice) {
        const int m = std::min(slice, n - f0);
        const size_t ob = (size_t)m * px * opx;
        uint8_t *dst = poses ? nullptr : (uint8_t *)out + f0 * px * opx;     // the caller's images of the slice
        rc = aux_reserve(p, m, w, h, host || poses ? ob : 0);    // (host twins and poses: the image goes to the scratch output)
        if (rc == DH_OK && host) rc = stage_frames(p, frames + f0 * px, m, w, h);
        if (rc == DH_OK)
            rc = aux_run(p, req, host ? p->ws.frames.get() : frames + f0 * px, m, w, h, K, host || poses ? p->ws.aux_out.get() : dst,
                         !poses ? nullptr : host ? p->ws.poses.get() : (dh_pose *)out + f0, s);
        if (rc == DH_OK && host && poses) rc = download(p, (dh_pose *)out + f0, p->ws.poses.get(), m, s);
        if (rc) return rc;
        if (host && !poses) {
            HIP_TRY(hipMemcpyAsync(dst, p->ws.aux_out.get(), ob, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return DH_OK;
}

static int predict_mask_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask, void *stream) {
    return aux_call(p, "dh_predict_mask_device", AUX_MASK, frames, n, w, h, nullptr, mask, false, (hipStream_t)stream);
}
static int hough_image_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out, void *stream) {
    return aux_call(p, "dh_hough_image_device", AUX_VOTES, frames, n, w, h, K, out, false, (hipStream_t)stream);
}
// HoughPrediction::build_hough_image in full (prediction.rs:760-845) and predict_parameter_from2dhough (:343-367).
static int build_hough_image_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out, void *stream) {
    return aux_call(p, "dh_build_hough_image_device", AUX_VOTES | AUX_BLUR, frames, n, w, h, K, out, false, (hipStream_t)stream);
}
static int predict_from2dhough_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], dh_pose *out, void *stream) {
    return aux_call(p, "dh_predict_from2dhough_device", AUX_VOTES | AUX_BLUR | AUX_POSES, frames, n, w, h, K, out, false, (hipStream_t)stream);
}
static int predict_mask_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask) {
    return aux_call(p, "dh_predict_mask", AUX_MASK, frames, n, w, h, nullptr, mask, true);
}
static int hough_image_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out) {
    return aux_call(p, "dh_hough_image", AUX_VOTES, frames, n, w, h, K, out, true);
}
static int build_hough_image_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out) {
    return aux_call(p, "dh_build_hough_image", AUX_VOTES | AUX_BLUR, frames, n, w, h, K, out, true);
}
static int predict_from2dhough_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], dh_pose *out) {
    return aux_call(p, "dh_predict_from2dhough", AUX_VOTES | AUX_BLUR | AUX_POSES, frames, n, w, h, K, out, true);
}

// ------------------------------------------------------------------ profiling
static int set_profiling_(dh_predictor *p, int on) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    p->profiling = on != 0;
    p->ev_valid = false;
    return DH_OK;
}
static int get_timing_(dh_predictor *p, dh_timing *out) {
    if (!p || !out) return fail(DH_EINVAL, "NULL argument");
    if (!p->ev_valid) return fail(DH_ESTATE, "no profiled batch yet (dh_set_profiling + a batch)");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipEventSynchronize(p->ev[3]));
    HIP_TRY(hipEventElapsedTime(&out->boxsum_ms, p->ev[0], p->ev[4]));
    HIP_TRY(hipEventElapsedTime(&out->traverse_ms, p->ev[4], p->ev[5]));
    HIP_TRY(hipEventElapsedTime(&out->emit_ms, p->ev[5], p->ev[1]));
    HIP_TRY(hipEventElapsedTime(&out->vote_ms, p->ev[1], p->ev[2]));
    HIP_TRY(hipEventElapsedTime(&out->cluster_ms, p->ev[2], p->ev[3]));
    HIP_TRY(hipEventElapsedTime(&out->total_ms, p->ev[0], p->ev[3]));
    out->n_frames = (uint32_t)p->last_n;

    return DH_OK;
}

// ------------------------------------------------------------------ parity taps
static int debug_enable_(dh_predictor *p, int on) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    p->debug = on != 0;
    if (!p->debug) p->ws.dbg_valid = false;
    return DH_OK;
}
// Runs a tap's body on the predictor's device once the last batch is complete (dbg: a batch that ran with the taps on).
template <typename F>
static int with_taps(dh_predictor *p, bool dbg, F body) {
    if (!p) return fail(DH_EINVAL, "NULL predictor");
    if (p->last_n == 0) return fail(DH_ESTATE, "no batch has run on this predictor");
    DeviceGuard guard(p->device);
    if (!guard.ok) return DH_EHIP;
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(DH_EHIP, "sync: %s", hipGetErrorString(e));
    if (dbg && !p->ws.dbg_valid) return fail(DH_ESTATE, "debug taps were not enabled for the last batch");
    return body();
}
static int debug_leaf_indices_(dh_predictor *p, int32_t *out, size_t cap) {
    return with_taps(p, true, [&]() -> int {
        size_t n = (size_t)p->last_n * p->ws.geom.npatch * p->n_trees;
        if (!out || cap < n) return fail(DH_EINVAL, "buffer too small: need %zu elements", n);
        if (n) HIP_TRY(hipMemcpy(out, p->ws.dbg_leaf.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_patch_flags_(dh_predictor *p, uint8_t *out, size_t cap) {
    return with_taps(p, true, [&]() -> int {
        size_t n = (size_t)p->last_n * p->ws.geom.npatch;
        if (!out || cap < n) return fail(DH_EINVAL, "buffer too small: need %zu elements", n);
        if (n) HIP_TRY(hipMemcpy(out, p->ws.dbg_flags.get(), n, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_grids_(dh_predictor *p, uint32_t *pos_grid, uint32_t *rot_grid) {
    return with_taps(p, false, [&]() -> int {
        const Workspace &ws = p->ws;       // (frames [0, last_n) of each grid)
        if (pos_grid) HIP_TRY(hipMemcpy(pos_grid, ws.pos_grid(0), (ws.pos_grid(p->last_n) - ws.pos_grid(0)) * 4, hipMemcpyDeviceToHost));
        if (rot_grid) HIP_TRY(hipMemcpy(rot_grid, ws.rot_grid(0), (ws.rot_grid(p->last_n) - ws.rot_grid(0)) * 4, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_hit_counts_(dh_predictor *p, uint32_t *out) {
    return with_taps(p, false, [&]() -> int {
        if (!out) return fail(DH_EINVAL, "NULL output");
        HIP_TRY(hipMemcpy(out, p->ws.hit_count(0), (size_t)p->last_n * 4, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
// The windows of every frame of the last batch that passed the probability gate (prediction.rs:582-584).  A batch whose tiles gated
// their own windows counted them (win_total: the lengths of its lists); for any other the frames' lists, still in the workspace, are
// gated once more here.
static int debug_window_totals_(dh_predictor *p, uint32_t *out) {
    return with_taps(p, false, [&]() -> int {
        if (!out) return fail(DH_EINVAL, "NULL output");
        const Workspace &ws = p->ws;
        const Geom &g = ws.geom;
        const size_t bytes = (size_t)p->last_n * 4;
        if (g.npatch <= 0) { memset(out, 0, bytes); return DH_OK; }
        if (ws.last_gated) { HIP_TRY(hipMemcpy(out, ws.win_total(0), bytes, hipMemcpyDeviceToHost)); return DH_OK; }
        Buf<uint32_t> tot;
        TRY(tot.alloc(p->last_n));
        HIP_TRY(hipMemset(tot.get(), 0, bytes));
        EmitArgs ea{};
        ea.n_frames = p->last_n; ea.px = g.px; ea.py = g.py; ea.tiles = g.tiles_x * g.tiles_y; ea.f = p->dev;
        set_windows(ea, ws, 0, p->n_trees);
        HIP_TRY(dh_launch_window_totals(ea, tot.get(), nullptr));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, tot.get(), bytes, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_geometry_(dh_predictor *p, int32_t out[10]) {
    if (!p || !out) return fail(DH_EINVAL, "NULL argument");
    if (p->ws.cap_frames == 0) return fail(DH_ESTATE, "no workspace yet (dh_predictor_reserve or a batch)");
    const Geom &g = p->ws.geom;
    const bool walk_tab = g.uniform && p->absorb_ok;
    const bool tile_gate = dh_tile_gate_(g, p->ws.cap_frames, p->absorb_ok, p->n_trees, p->debug, p->knobs);
    const int32_t v[10] = {(g.uniform ? 1 : 0) | (walk_tab ? 1 << 8 : 0) | (tile_gate ? 1 << 9 : 0) | (walk_tab ? g.top_levels << 16 : 0), g.px, g.py, g.tiles_x, g.tiles_y, g.swz_log2, g.swz_q, g.ss_row, p->f_rw, p->f_rh};
    memcpy(out, v, sizeof v);
    return DH_OK;
}
// Like the other taps this describes the last resident slice of the last batch (batch_device starts every slice with list_chunks = 0;
// a replayed graph rewrites the lists of the batch it captured; the mask / 2-D Hough calls run without lists and clear last_n).
// The tile lists of that slice: shifts[f] = {sx, sy} of frame f's tile grid in windows (zeros where no frame chooses: TileShifts),
// counts[x] = flagged tiles in the list of the frames = x mod 8 (summed over forked sub-batches, each of which counts from its own first frame).
static int debug_tile_shifts_(dh_predictor *p, int32_t *shifts, uint32_t counts[8]) {
    return with_taps(p, false, [&]() -> int {
        const Workspace &ws = p->ws;
        if (!shifts || !counts) return fail(DH_EINVAL, "NULL output");
        if (ws.list_chunks == 0) return fail(DH_ESTATE, "the last batch ran without tile lists");
        std::vector<uint32_t> sh((size_t)p->last_n, 0u);
        if (ws.tile_shift) HIP_TRY(hipMemcpy(sh.data(), ws.tile_shift.get(), sh.size() * 4, hipMemcpyDeviceToHost));
        for (int f = 0; f < p->last_n; ++f) { shifts[2 * f] = (int32_t)(sh[f] & 0xffffu); shifts[2 * f + 1] = (int32_t)(sh[f] >> 16); }
        for (int x = 0; x < 8; ++x) counts[x] = 0;
        for (int c = 0; c < ws.list_chunks; ++c) {
            uint32_t cc[8];
            HIP_TRY(hipMemcpy(cc, ws.list_ptr(c) + 16 * ws.tile_list_stride, sizeof cc, hipMemcpyDeviceToHost));
            for (int x = 0; x < 8; ++x) counts[x] += cc[x];
        }
        return DH_OK;
    });
}
static int debug_guesses_(dh_predictor *p, int32_t *out) {
    return with_taps(p, true, [&]() -> int {
        if (!out) return fail(DH_EINVAL, "NULL output");
        HIP_TRY(hipMemcpy(out, p->ws.dbg_guess.get(), (size_t)p->last_n * 6 * 4, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_meanshift_(dh_predictor *p, int which, int32_t *trace, uint32_t *steps) {
    return with_taps(p, true, [&]() -> int {
        if (which < 0 || which > 1) return fail(DH_EINVAL, "which must be 0 or 1");
        size_t per = (size_t)(p->params.meanshift_iterations + 1) * 3;
        // device layout is [2][last batch n][...]: the kernel indexed with n_frames = last_n
        if (trace) HIP_TRY(hipMemcpy(trace, p->ws.dbg_trace.get() + (size_t)which * p->last_n * per, (size_t)p->last_n * per * 4, hipMemcpyDeviceToHost));
        if (steps) HIP_TRY(hipMemcpy(steps, p->ws.dbg_steps.get() + (size_t)which * p->last_n, (size_t)p->last_n * 4, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}
static int debug_votes_(dh_predictor *p, int frame, int which, int32_t *out, size_t cap, size_t *count) {
    return with_taps(p, false, [&]() -> int {
        if (frame < 0 || frame >= p->last_n || which < 0 || which > 1 || !count) return fail(DH_EINVAL, "bad frame / which / count");
        // k_emit writes the rotation records only without the leaf histogram or with the taps on
        Workspace &ws = p->ws;
        if (which == 1 && ws.lay.leaves && !ws.dbg_valid) return fail(DH_ESTATE, "rotation votes need dh_debug_enable(1) before the batch");
        if (cap > 0xffffffffull) cap = 0xffffffffull;
        if (!ws.dbg_vcount) TRY(ws.dbg_vcount.alloc(1));
        if (cap * 4 > ws.dbg_votes.cap()) TRY(ws.dbg_votes.alloc(cap * 4));
        HIP_TRY(hipMemset(ws.dbg_vcount.get(), 0, 4));
        VotesDumpArgs a{};
        a.frame = frame; a.which = which; a.f = p->dev; set_hits(a, ws, 0);
        a.out = ws.dbg_votes.get(); a.cap = (uint32_t)cap; a.count = ws.dbg_vcount.get();
        HIP_TRY(dh_launch_votes_dump(a, nullptr));
        HIP_TRY(hipDeviceSynchronize());
        uint32_t c = 0;
        HIP_TRY(hipMemcpy(&c, ws.dbg_vcount.get(), 4, hipMemcpyDeviceToHost));
        *count = c;
        size_t ncopy = std::min<size_t>(c, cap);
        if (ncopy && out) HIP_TRY(hipMemcpy(out, ws.dbg_votes.get(), ncopy * 16, hipMemcpyDeviceToHost));
        return DH_OK;
    });
}

// ------------------------------------------------------------------ what the fit trackers' unit calls (dh_runtime_track.h)
// A fit tracker's whole step (dh_api_fit_track.hip) runs the prediction or the rig step inside its own entry point's guard, so
// it calls these bodies, not the public entry points over them.
int dh_predict_batch_cameras_support_device_(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                             const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                                             uint32_t radius, dh_pose *out, dh_support *support, void *stream) {
    return predict_batch_cameras_support_device_(p, frames, n, w, h, c, midp_guess, rot_guess, guess_mask, radius, out, support, stream);
}
int dh_rig_tracker_step_device_(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                uint32_t *n_heads, dh_head *heads, uint32_t *ids, uint32_t *n_persons, dh_rig_person *persons,
                                dh_rig_track *tracks, void *stream) {
    return rig_tracker_step_device_(p, t, frames, w, h, present, n_heads, heads, ids, n_persons, persons, tracks, stream);
}
int dh_predictor_device_(const dh_predictor *p) { return p->device; }

// ------------------------------------------------------------------ the C ABI (DH_API: dh_runtime.h)
DH_API(forest_create, (const dh_forest_desc *d, dh_forest **out), (d, out))
DH_API(forest_destroy, (dh_forest *f), (f))
DH_API(forest_info, (const dh_forest *f, uint32_t *n_trees, uint32_t *n_nodes, uint32_t *n_leaves, uint32_t *max_depth), (f, n_trees, n_nodes, n_leaves, max_depth))
DH_API(patch_grid, (const dh_params *p, int w, int h, int *nx, int *ny), (p, w, h, nx, ny))
DH_API(predictor_destroy, (dh_predictor *p), (p))
DH_API(predictor_create, (const dh_forest *f, const dh_params *prm, int device, dh_predictor **out), (f, prm, device, out))
DH_API(predictor_update_sigma, (dh_predictor *p, float val), (p, val))
DH_API(predictor_sigma, (const dh_predictor *p, float *out), (p, out))
DH_API(predictor_reserve, (dh_predictor *p, int n, int w, int h), (p, n, w, h))
DH_API(predictor_set_forking, (dh_predictor *p, int chunks), (p, chunks))
DH_API(predict_batch_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out, void *stream_), (p, frames, n, w, h, K, midp_guess, rot_guess, guess_mask, out, stream_))
DH_API(predict_batch, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out), (p, frames, n, w, h, K, midp_guess, rot_guess, guess_mask, out))
DH_API(host_alloc, (size_t bytes, void **out), (bytes, out))
DH_API(host_free, (void *ptr), (ptr))
DH_API(biwi_decode_depth_device, (dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, uint16_t *frames_dev, size_t cap_px, uint32_t *w, uint32_t *h), (p, bufs, lens, n, frames_dev, cap_px, w, h))
DH_API(predict_batch_rle, (dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out), (p, bufs, lens, n, K, midp_guess, rot_guess, guess_mask, out))
DH_API(graph_destroy, (dh_predictor *p), (p))
DH_API(graph_capture, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out), (p, frames, n, w, h, K, midp_guess, rot_guess, guess_mask, out))
DH_API(graph_launch, (dh_predictor *p, void *stream), (p, stream))
DH_API(predict_mask_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask, void *stream), (p, frames, n, w, h, mask, stream))
DH_API(hough_image_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out, void *stream), (p, frames, n, w, h, K, out, stream))
DH_API(predict_mask, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask), (p, frames, n, w, h, mask))
DH_API(hough_image, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out), (p, frames, n, w, h, K, out))
DH_API(build_hough_image_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out, void *stream), (p, frames, n, w, h, K, out, stream))
DH_API(predict_from2dhough_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], dh_pose *out, void *stream), (p, frames, n, w, h, K, out, stream))
DH_API(build_hough_image, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out), (p, frames, n, w, h, K, out))
DH_API(predict_from2dhough, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], dh_pose *out), (p, frames, n, w, h, K, out))
DH_API(set_profiling, (dh_predictor *p, int on), (p, on))
DH_API(get_timing, (dh_predictor *p, dh_timing *out), (p, out))
DH_API(debug_enable, (dh_predictor *p, int on), (p, on))
DH_API(debug_leaf_indices, (dh_predictor *p, int32_t *out, size_t cap), (p, out, cap))
DH_API(debug_patch_flags, (dh_predictor *p, uint8_t *out, size_t cap), (p, out, cap))
DH_API(debug_grids, (dh_predictor *p, uint32_t *pos_grid, uint32_t *rot_grid), (p, pos_grid, rot_grid))
DH_API(debug_hit_counts, (dh_predictor *p, uint32_t *out), (p, out))
DH_API(debug_geometry, (dh_predictor *p, int32_t out[10]), (p, out))
DH_API(debug_window_totals, (dh_predictor *p, uint32_t *out), (p, out))
DH_API(debug_tile_shifts, (dh_predictor *p, int32_t *shifts, uint32_t counts[8]), (p, shifts, counts))
DH_API(debug_guesses, (dh_predictor *p, int32_t *out), (p, out))
DH_API(debug_meanshift, (dh_predictor *p, int which, int32_t *trace, uint32_t *steps), (p, which, trace, steps))
DH_API(debug_votes, (dh_predictor *p, int frame, int which, int32_t *out, size_t cap, size_t *count), (p, frame, which, out, cap, count))
DH_API(cameras_create, (const float *K, int n, int device, dh_cameras **out), (K, n, device, out))
DH_API(cameras_destroy, (dh_cameras *c), (c))
DH_API(predict_batch_cameras, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out), (p, frames, n, w, h, c, midp_guess, rot_guess, guess_mask, out))
DH_API(predict_batch_cameras_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out, void *stream), (p, frames, n, w, h, c, midp_guess, rot_guess, guess_mask, out, stream))
DH_API(tracker_create, (const dh_cameras *c, uint32_t flags, dh_tracker **out), (c, flags, out))
DH_API(tracker_destroy, (dh_tracker *t), (t))
DH_API(tracker_reset, (dh_tracker *t, int camera, void *stream), (t, camera, stream))
DH_API(tracker_step, (dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out), (p, t, frames, w, h, present, out))
DH_API(tracker_step_device, (dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out, void *stream), (p, t, frames, w, h, present, out, stream))
DH_API(tracker_state, (dh_tracker *t, float *midp, double *rot, uint8_t *flags), (t, midp, rot, flags))
DH_API(tracker_capture, (dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out), (p, t, frames, w, h, present, out))
DH_API(predict_batch_support, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius, dh_pose *out, dh_support *support), (p, frames, n, w, h, K, midp_guess, rot_guess, guess_mask, radius, out, support))
DH_API(predict_batch_support_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius, dh_pose *out, dh_support *support, void *stream), (p, frames, n, w, h, K, midp_guess, rot_guess, guess_mask, radius, out, support, stream))
DH_API(predict_batch_cameras_support, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius, dh_pose *out, dh_support *support), (p, frames, n, w, h, c, midp_guess, rot_guess, guess_mask, radius, out, support))
DH_API(predict_batch_cameras_support_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius, dh_pose *out, dh_support *support, void *stream), (p, frames, n, w, h, c, midp_guess, rot_guess, guess_mask, radius, out, support, stream))
DH_API(tracker_step_support, (dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, dh_pose *out, dh_support *support), (p, t, frames, w, h, present, radius, out, support))
DH_API(tracker_step_support_device, (dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius, dh_pose *out, dh_support *support, void *stream), (p, t, frames, w, h, present, radius, out, support, stream))
DH_API(predict_heads, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads, uint32_t radius, uint32_t *n_heads, dh_head *heads), (p, frames, n, w, h, K, max_heads, radius, n_heads, heads))
DH_API(predict_heads_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads, uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream), (p, frames, n, w, h, K, max_heads, radius, n_heads, heads, stream))
DH_API(predict_heads_cameras, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads, uint32_t radius, uint32_t *n_heads, dh_head *heads), (p, frames, n, w, h, c, max_heads, radius, n_heads, heads))
DH_API(predict_heads_cameras_device, (dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads, uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream), (p, frames, n, w, h, c, max_heads, radius, n_heads, heads, stream))
DH_API(multi_tracker_create, (const dh_cameras *c, const dh_multi_track_params *prm, dh_multi_tracker **out), (c, prm, out))
DH_API(multi_tracker_destroy, (dh_multi_tracker *t), (t))
DH_API(multi_tracker_reset, (dh_multi_tracker *t, int camera, void *stream), (t, camera, stream))
DH_API(multi_tracker_step, (dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks), (p, t, frames, w, h, present, n_heads, heads, ids, tracks))
DH_API(multi_tracker_step_device, (dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks, void *stream), (p, t, frames, w, h, present, n_heads, heads, ids, tracks, stream))
DH_API(multi_tracker_state, (dh_multi_tracker *t, dh_head_track *tracks, uint32_t *next_id), (t, tracks, next_id))
DH_API(multi_tracker_capture, (dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks), (p, t, frames, w, h, present, n_heads, heads, ids, tracks))
DH_API(rig_create, (const dh_cameras *c, const float *R, const float *t, const int32_t *rig_begin, int n_rigs, dh_rig **out), (c, R, t, rig_begin, n_rigs, out))
DH_API(rig_destroy, (dh_rig *r), (r))
DH_API(rig_tracker_create, (const dh_rig *r, const dh_rig_track_params *prm, dh_rig_tracker **out), (r, prm, out))
DH_API(rig_tracker_destroy, (dh_rig_tracker *t), (t))
DH_API(rig_tracker_reset, (dh_rig_tracker *t, int rig, void *stream), (t, rig, stream))
DH_API(rig_tracker_step, (dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks), (p, t, frames, w, h, present, n_heads, heads, rig_ids, n_persons, persons, tracks))
DH_API(rig_tracker_step_device, (dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, void *stream), (p, t, frames, w, h, present, n_heads, heads, rig_ids, n_persons, persons, tracks, stream))
DH_API(rig_tracker_state, (dh_rig_tracker *t, dh_rig_track *tracks, uint32_t *next_id), (t, tracks, next_id))
DH_API(rig_tracker_capture, (dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks), (p, t, frames, w, h, present, n_heads, heads, rig_ids, n_persons, persons, tracks))
