// dh_render.h -- the renderer's kernel argument block, record layouts and launchers (k_render.hip), shared with the host
// runtime (dh_api_render.hip).  Not part of the ABI.  The rule the kernels implement is stated in include/depthhead_hip.h (section
// "rendering posed meshes") and DESIGN.md section 17.
#pragma once
#include "dh_internal.h"

static_assert(sizeof(dh_render_instance) == 64, "dh_render_instance: 64 bytes, no padding");
static_assert(sizeof(dh_render_params) == 40, "dh_render_params: 40 bytes");

// a screen tile: one workgroup of k_render_resolve, its keys in LDS (4 KB); a tile row is 128 bytes of depth
#define DH_RT_W 64
#define DH_RT_H 16
#define DH_RENDER_GUARD 1048576     // 2^20: snapped coordinates beyond it drop the triangle

// One mesh of a render call (device pointers of a dh_mesh).
struct RenderMesh {
    const float *verts;       // [nv][3]
    const uint32_t *tris;     // [nt][3]
    uint32_t nv, nt;
};

// One triangle after setup: snapped vertices (1/16 pixel, area > 0 after the swap of vertices 1 and 2), camera-space depths.
struct __attribute__((aligned(16))) RenderTri {
    int32_t x0, y0, x1, y1;
    int32_t x2, y2;
    float z0, z1;
    float z2;
    uint32_t frame;
    uint32_t low;             // key bit 0: 0 head, 1 not a head
    uint32_t valid;           // 0: dropped, or no pixel centre of the frame inside its bounding box
};
static_assert(sizeof(RenderTri) == 48, "RenderTri is three 16-byte rows");

struct RenderArgs {
    // the call
    const RenderMesh *meshes;
    const dh_render_instance *inst;
    const uint32_t *tri_begin;    // [n_inst + 1] first triangle record of each instance
    uint32_t n_inst, max_nt;      // max_nt: the most triangles any instance's mesh has
    uint32_t n_tri;               // tri_begin[n_inst]
    int n, w, h, tiles_x, tiles_y;
    float k[9];                   // the one K of the batch (cams == NULL)
    const DhCam *cams;            // nullable [n]: frame f sees cams[f].k
    // renderer-owned
    RenderTri *tri;               // [tri_begin[n_inst]]
    uint32_t *tile_cnt;           // [n * tiles]: triangles whose bounding box touches the tile (zeroed per call)
    uint32_t *tile_cur;           // [n * tiles]: k_render_offsets: first list slot; after k_render_fill: one past the last
    unsigned long long *total;    // [2]: sum of tile_cnt (setup), list slots handed out (offsets); zeroed per call
    uint32_t *list;               // [list_cap] triangle record indices, tile after tile
    unsigned long long list_cap;
    // outputs
    uint16_t *frames;             // [n][h][w]
    uint8_t *masks;               // nullable
    int vec;                      // 1: w % 8 == 0 and both outputs 16 / 8 byte aligned: 8 pixels per lane and store
    // sensor model
    uint32_t noise;               // a
    unsigned long long hole_thr;  // floor(p * 2^53)
    unsigned long long seed;
};

hipError_t dh_launch_render_setup(const RenderArgs &a, hipStream_t s);      // records, tile counts, total[0]
hipError_t dh_launch_render_offsets(const RenderArgs &a, hipStream_t s);    // tile_cur
hipError_t dh_launch_render_fill(const RenderArgs &a, hipStream_t s);       // list
hipError_t dh_launch_render_resolve(const RenderArgs &a, hipStream_t s);    // frames, masks
