// dh_api_render.hip -- meshes and the renderer of posed meshes (kernels: k_render.hip).
#include "dh_runtime.h"
#include "dh_render.h"

// ------------------------------------------------------------------ rendering posed meshes
// A mesh: vertices and index triples on one device, immutable.
struct dh_mesh {
    int device = 0;
    uint32_t nv = 0, nt = 0;
    float bbox[6] = {0, 0, 0, 0, 0, 0};
    Buf<float> verts;
    Buf<uint32_t> tris;
};
static int mesh_create_(const float *verts, uint32_t nv, const uint32_t *tris, uint32_t nt, int device, dh_mesh **out) {
    if (!out) return fail(DH_EINVAL, "dh_mesh_create: NULL argument");
    *out = nullptr;
    if (!verts || !tris) return fail(DH_EINVAL, "dh_mesh_create: NULL argument");
    if (nv == 0 || nt == 0) return fail(DH_EINVAL, "dh_mesh_create: %u vertices and %u triangles, expected at least one of each", nv, nt);
    if (nt > 0x7fffffffu / 3 || nv > 0x7fffffffu / 3) return fail(DH_EINVAL, "dh_mesh_create: mesh too large");
    std::unique_ptr<dh_mesh> m(new dh_mesh);
    m->device = device; m->nv = nv; m->nt = nt;
    for (int q = 0; q < 3; ++q) { m->bbox[q] = INFINITY; m->bbox[3 + q] = -INFINITY; }
    for (size_t i = 0; i < (size_t)nv * 3; ++i) {
        if (!std::isfinite(verts[i])) return fail(DH_EINVAL, "dh_mesh_create: vertex %zu is not finite", i / 3);
        m->bbox[i % 3] = std::min(m->bbox[i % 3], verts[i]);
        m->bbox[3 + i % 3] = std::max(m->bbox[3 + i % 3], verts[i]);
    }
    for (size_t i = 0; i < (size_t)nt * 3; ++i)
        if (tris[i] >= nv) return fail(DH_EINVAL, "dh_mesh_create: triangle %zu names vertex %u of %u", i / 3, tris[i], nv);
    DeviceGuard guard(device);
    if (!guard.ok) return DH_EHIP;
    TRY(m->verts.alloc((size_t)nv * 3));
    TRY(m->tris.alloc((size_t)nt * 3));
    HIP_TRY(hipMemcpy(m->verts.get(), verts, (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->tris.get(), tris, (size_t)nt * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
    *out = m.release();
    return DH_OK;
}
static int mesh_destroy_(dh_mesh *m) {
    if (!m) return DH_OK;
    DeviceGuard guard(m->device);
    delete m;
    return DH_OK;
}
static int mesh_info_(const dh_mesh *m, uint32_t *nv, uint32_t *nt, float bbox[6]) {
    if (!m) return fail(DH_EINVAL, "dh_mesh_info: NULL mesh");
    if (nv) *nv = m->nv;
    if (nt) *nt = m->nt;
    if (bbox) memcpy(bbox, m->bbox, sizeof m->bbox);
    return DH_OK;
}

// A renderer: the call's tables, the triangle records, the tile counters and lists, and the device frames of the host calls.
// Everything grows on demand and is kept between calls.
struct dh_renderer {
    int device = 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool profiling = false, timed = false;
    Buf<unsigned long long, PINNED> total_h; // [2]
    Buf<unsigned long long> total;           // [2]
    Buf<RenderTri> tri;
    Buf<uint32_t> tile_cnt, tile_cur, list;
    Buf<uint16_t> frames;                    // host calls
    Buf<uint8_t> masks;
    CallTables tab;                          // tri_begin | meshes | instances (last: its stream and events go before any buffer)
    ~dh_renderer() {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    }
};
static int renderer_destroy_(dh_renderer *r) { return destroy_owner(r); }
static int renderer_create_(int device, dh_renderer **out) { return create_owner(device, out, "dh_renderer_create"); }
// (the first buffers too come with the first render)
static int renderer_init(dh_renderer *r) {
    if (r->tab.s) return DH_OK;
    TRY(r->tab.init());
    for (auto &e : r->ev) TRY(hip_step(hipEventCreate(&e), "hipEventCreate"));
    TRY(r->total.alloc(2));
    TRY(r->total_h.alloc(2));
    return DH_OK;
}
static int renderer_set_profiling_(dh_renderer *r, int on) {
    if (!r) return fail(DH_EINVAL, "dh_renderer_set_profiling: NULL renderer");
    r->profiling = on != 0;
    return DH_OK;
}
static int renderer_timing_(dh_renderer *r, float ms[4]) {
    if (!r || !ms) return fail(DH_EINVAL, "dh_renderer_timing: NULL argument");
    if (!r->timed) return fail(DH_ESTATE, "dh_renderer_timing: no render has run with profiling on");
    DeviceGuard guard(r->device);
    if (!guard.ok) return DH_EHIP;
    HIP_TRY(hipEventSynchronize(r->ev[4]));
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], r->ev[i], r->ev[i + 1]));
    return DH_OK;
}

// One render call.  dev_out: frames / masks are device pointers and `stream` the caller's; else host pointers.
struct RenderReq {
    const dh_mesh *const *meshes; uint32_t n_meshes;
    const dh_render_instance *inst; uint32_t n_inst;
    int n, w, h;
    const float *K; const dh_cameras *cams; bool use_cams;
    const dh_render_params *prm;
    uint16_t *frames; uint8_t *masks;
};
static int render_run(dh_renderer *r, const RenderReq &q, bool dev_out, hipStream_t stream, const char *who) {
    // ---- refusals: all of them before anything is allocated or launched
    if (!r) return fail(DH_EINVAL, "%s: NULL renderer", who);
    if (!q.frames) return fail(DH_EINVAL, "%s: NULL frames", who);
    TRY(check_frames(q.n, q.w, q.h, q.K, q.cams, q.use_cams, r->device, "renderer", who));
    if (q.n_inst && !q.inst) return fail(DH_EINVAL, "%s: NULL instances", who);
    if (q.n_inst && !q.meshes) return fail(DH_EINVAL, "%s: NULL meshes", who);
    if (q.n_inst > 0x7fffffffu) return fail(DH_EINVAL, "%s: too many instances", who);
    uint32_t noise = 0;
    unsigned long long hole_thr = 0, seed = 0;
    if (q.prm) {
        const double p = q.prm->hole_probability;
        if (!(p >= 0.0 && p <= 1.0)) return fail(DH_EINVAL, "%s: hole_probability %g outside [0, 1]", who, p);
        if (q.prm->noise_amplitude > 65535u) return fail(DH_EINVAL, "%s: noise_amplitude %u above 65535", who, q.prm->noise_amplitude);
        noise = q.prm->noise_amplitude; seed = q.prm->seed;
        hole_thr = (unsigned long long)floor(p * 9007199254740992.0);
    }
    for (uint32_t i = 0; i < q.n_inst; ++i) {
        if (q.inst[i].frame >= (uint32_t)q.n) return fail(DH_EINVAL, "%s: instance %u names frame %u of %d", who, i, q.inst[i].frame, q.n);
        if (q.inst[i].mesh >= q.n_meshes) return fail(DH_EINVAL, "%s: instance %u names mesh %u of %u", who, i, q.inst[i].mesh, q.n_meshes);
    }
    for (uint32_t i = 0; i < q.n_meshes && q.n_inst; ++i) {
        if (!q.meshes[i]) return fail(DH_EINVAL, "%s: mesh %u is NULL", who, i);
        if (q.meshes[i]->device != r->device) return fail(DH_EINVAL, "%s: mesh %u lives on device %d, the renderer on %d", who, i, q.meshes[i]->device, r->device);
    }
    uint64_t n_tri = 0;
    uint32_t max_nt = 0;
    for (uint32_t i = 0; i < q.n_inst; ++i) {
        n_tri += q.meshes[q.inst[i].mesh]->nt;
        max_nt = std::max(max_nt, q.meshes[q.inst[i].mesh]->nt);
    }
    if (n_tri > 0x7fffffffull) return fail(DH_ESIZE, "%s: %llu triangles in one call (limit 2^31 - 1)", who, (unsigned long long)n_tri);

    DeviceGuard guard(r->device);
    if (!guard.ok) return DH_EHIP;
    TRY(renderer_init(r));
    hipStream_t s = dev_out ? stream : r->tab.s;
    RenderArgs a;
    memset(&a, 0, sizeof a);
    a.n = q.n; a.w = q.w; a.h = q.h;
    a.tiles_x = (q.w + DH_RT_W - 1) / DH_RT_W; a.tiles_y = (q.h + DH_RT_H - 1) / DH_RT_H;
    const size_t n_tiles = (size_t)q.n * a.tiles_x * a.tiles_y, n_px = (size_t)q.n * q.w * q.h;
    if (n_tiles > 0x7fffffffull) return fail(DH_ESIZE, "%s: %zu screen tiles in one call (limit 2^31 - 1)", who, n_tiles);
    a.n_inst = q.n_inst; a.max_nt = max_nt; a.n_tri = (uint32_t)n_tri;
    if (q.use_cams) a.cams = q.cams->dev.get();
    else memcpy(a.k, q.K, sizeof a.k);
    a.noise = noise; a.hole_thr = hole_thr; a.seed = seed;
    // ---- the call's tables: one staging buffer, one upload
    const size_t o_mesh = (((size_t)q.n_inst + 1) * sizeof(uint32_t) + 15) & ~(size_t)15;
    const size_t o_inst = o_mesh + (((size_t)q.n_meshes * sizeof(RenderMesh) + 15) & ~(size_t)15);
    const size_t bytes = o_inst + (size_t)q.n_inst * sizeof(dh_render_instance);
    TRY(r->tab.reserve(bytes));
    {
        uint32_t *tb = (uint32_t *)r->tab.stage.get();
        RenderMesh *mm = (RenderMesh *)(r->tab.stage.get() + o_mesh);
        uint32_t acc = 0;
        for (uint32_t i = 0; i < q.n_inst; ++i) { tb[i] = acc; acc += q.meshes[q.inst[i].mesh]->nt; }
        tb[q.n_inst] = acc;
        for (uint32_t i = 0; i < q.n_meshes && q.n_inst; ++i) mm[i] = RenderMesh{q.meshes[i]->verts.get(), q.meshes[i]->tris.get(), q.meshes[i]->nv, q.meshes[i]->nt};
        if (q.n_inst) memcpy(r->tab.stage.get() + o_inst, q.inst, (size_t)q.n_inst * sizeof(dh_render_instance));
    }
    a.tri_begin = (const uint32_t *)r->tab.dev.get();
    a.meshes = (const RenderMesh *)(r->tab.dev.get() + o_mesh);
    a.inst = (const dh_render_instance *)(r->tab.dev.get() + o_inst);
    // ---- renderer-owned memory (growing waits for whatever still uses the old)
    if (r->tri.cap() < n_tri || r->tile_cnt.cap() < n_tiles) HIP_TRY(hipDeviceSynchronize());
    TRY(r->tri.grow((size_t)n_tri));
    if (r->tile_cnt.cap() < n_tiles) { TRY(r->tile_cnt.grow(n_tiles)); TRY(r->tile_cur.alloc(r->tile_cnt.cap())); }
    if (!dev_out) {
        if (r->frames.cap() < n_px) { HIP_TRY(hipDeviceSynchronize()); TRY(r->frames.grow(n_px)); TRY(r->masks.alloc(r->frames.cap())); }
        a.frames = r->frames.get(); a.masks = q.masks ? r->masks.get() : nullptr;
    } else { a.frames = q.frames; a.masks = q.masks; }
    a.vec = q.w % 8 == 0 && (uintptr_t)a.frames % 16 == 0 && (uintptr_t)a.masks % 8 == 0 ? 1 : 0;
    a.tri = r->tri.get(); a.tile_cnt = r->tile_cnt.get(); a.tile_cur = r->tile_cur.get(); a.total = r->total.get();
    const bool prof = r->profiling;
    Range range(prof, "dh:render");
    TRY(r->tab.upload(bytes, s));                       // (waits for a call on another stream that still uses the records and lists)
    HIP_TRY(hipMemsetAsync(a.tile_cnt, 0, n_tiles * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(a.total, 0, 2 * sizeof(unsigned long long), s));
    if (prof) HIP_TRY(hipEventRecord(r->ev[0], s));
    TRY(hip_step(dh_launch_render_setup(a, s), "k_render_setup"));
    if (prof) HIP_TRY(hipEventRecord(r->ev[1], s));
    // the size of the tile lists: the one point where the host waits
    HIP_TRY(hipMemcpyAsync(r->total_h.get(), a.total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const unsigned long long refs = r->total_h.get()[0];
    if (refs > 0xffffffffull) return fail(DH_ESIZE, "%s: the tile lists need %llu entries (limit 2^32 - 1)", who, refs);
    TRY(r->list.grow((size_t)refs));
    a.list = r->list.get(); a.list_cap = r->list.cap();
    TRY(hip_step(dh_launch_render_offsets(a, s), "k_render_offsets"));
    if (prof) HIP_TRY(hipEventRecord(r->ev[2], s));
    TRY(hip_step(dh_launch_render_fill(a, s), "k_render_fill"));
    if (prof) HIP_TRY(hipEventRecord(r->ev[3], s));
    TRY(hip_step(dh_launch_render_resolve(a, s), "k_render_resolve"));
    if (prof) { HIP_TRY(hipEventRecord(r->ev[4], s)); r->timed = true; }
    TRY(r->tab.done(s));
    if (!dev_out) {
        HIP_TRY(hipMemcpyAsync(q.frames, a.frames, n_px * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
        if (q.masks) HIP_TRY(hipMemcpyAsync(q.masks, a.masks, n_px, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return DH_OK;
}
static int render_depth_(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances,
                         int n, int w, int h, const float K[9], const dh_render_params *params, uint16_t *frames, uint8_t *masks) {
    return render_run(r, RenderReq{meshes, n_meshes, instances, n_instances, n, w, h, K, nullptr, false, params, frames, masks}, false, nullptr, "dh_render_depth");
}
static int render_depth_cameras_(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances,
                                 int n, int w, int h, const dh_cameras *c, const dh_render_params *params, uint16_t *frames, uint8_t *masks) {
    return render_run(r, RenderReq{meshes, n_meshes, instances, n_instances, n, w, h, nullptr, c, true, params, frames, masks}, false, nullptr, "dh_render_depth_cameras");
}
static int render_depth_device_(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances,
                                int n, int w, int h, const float K[9], const dh_render_params *params, uint16_t *frames, uint8_t *masks, void *stream) {
    return render_run(r, RenderReq{meshes, n_meshes, instances, n_instances, n, w, h, K, nullptr, false, params, frames, masks}, true, (hipStream_t)stream, "dh_render_depth_device");
}
static int render_depth_cameras_device_(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances,
                                        int n, int w, int h, const dh_cameras *c, const dh_render_params *params, uint16_t *frames, uint8_t *masks, void *stream) {
    return render_run(r, RenderReq{meshes, n_meshes, instances, n_instances, n, w, h, nullptr, c, true, params, frames, masks}, true, (hipStream_t)stream, "dh_render_depth_cameras_device");
}

// ------------------------------------------------------------------ the C ABI (DH_API: dh_runtime.h)
DH_API(mesh_create, (const float *verts, uint32_t nv, const uint32_t *tris, uint32_t nt, int device, dh_mesh **out), (verts, nv, tris, nt, device, out))
DH_API(mesh_destroy, (dh_mesh *m), (m))
DH_API(mesh_info, (const dh_mesh *m, uint32_t *nv, uint32_t *nt, float bbox[6]), (m, nv, nt, bbox))
DH_API(renderer_create, (int device, dh_renderer **out), (device, out))
DH_API(renderer_destroy, (dh_renderer *r), (r))
DH_API(renderer_set_profiling, (dh_renderer *r, int on), (r, on))
DH_API(renderer_timing, (dh_renderer *r, float ms[4]), (r, ms))
DH_API(render_depth, (dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances, int n, int w, int h, const float K[9], const dh_render_params *params, uint16_t *frames, uint8_t *masks), (r, meshes, n_meshes, instances, n_instances, n, w, h, K, params, frames, masks))
DH_API(render_depth_cameras, (dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances, int n, int w, int h, const dh_cameras *c, const dh_render_params *params, uint16_t *frames, uint8_t *masks), (r, meshes, n_meshes, instances, n_instances, n, w, h, c, params, frames, masks))
DH_API(render_depth_device, (dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances, int n, int w, int h, const float K[9], const dh_render_params *params, uint16_t *frames, uint8_t *masks, void *stream), (r, meshes, n_meshes, instances, n_instances, n, w, h, K, params, frames, masks, stream))
DH_API(render_depth_cameras_device, (dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances, uint32_t n_instances, int n, int w, int h, const dh_cameras *c, const dh_render_params *params, uint16_t *frames, uint8_t *masks, void *stream), (r, meshes, n_meshes, instances, n_instances, n, w, h, c, params, frames, masks, stream))
