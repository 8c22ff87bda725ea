/*
 * depthhead_hip.h -- C ABI of libdepthhead_hip.so: the MI355X (gfx950) implementation of
 * depthhead's Hough-forest head-pose inference path.
 *
 * The reference (Entscheider/depthhead, pure Rust) has no FFI or plugin interface; its public
 * seam for this path is
 *     HoughPrediction::predict_parameter_parallel(&self, img: Arc<DepthImage>,
 *         intrinsic: &IntrinsicMatrix, midp_guess: Option<[f32;3]>, rot_guess: Option<[f64;3]>)
 *         -> PredictionResult                                   (src/hough/prediction.rs:397-409)
 * and its serial twin predict_parameter (:376-388).  This library sits where
 * predict_parameter_generic (:421-493) sits, with a FRAME BATCH as the unit of work, so a Rust
 * `extern "C"` shim can keep the method signature unchanged.
 *
 * Plain C: pointers and sizes only.  Every entry point returns an int status (0 = DH_OK,
 * negative = error) and never throws or aborts across the boundary; dh_last_error() gives the
 * message of the calling thread's last failure.
 *
 * Threading (mirrors `HoughPrediction: !Sync`, prediction.rs:253 / types.rs:405): a dh_forest is
 * immutable and may be shared; a dh_predictor is NOT thread-safe -- one per host thread / GPU
 * stream.  Distinct predictors may run concurrently.
 */
#ifndef DEPTHHEAD_HIP_H
#define DEPTHHEAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_VERSION 100 /* 0.1.0 */

/* ---- status codes ---- */
#define DH_OK 0
#define DH_EINVAL (-1)  /* NULL / out-of-range argument                                    */
#define DH_EFOREST (-2) /* forest violates an invariant the reference would panic on        */
#define DH_EHIP (-3)    /* HIP runtime error (message has the hipError string)              */
#define DH_ENOMEM (-4)  /* host or device allocation failed                                 */
#define DH_ESIZE (-5)   /* geometry unsupported: frame smaller than the patch, etc.         */
#define DH_ESTATE (-6)  /* call not valid in this state (e.g. debug tap without a batch)    */

/* ---- compile-time constants of the reference (src/hough/prediction.rs:270-286, :314, :584) ---- */
#define DH_ZSCALEFACTOR 1
#define DH_GUESS_GRID_PARTS 20
#define DH_ROT_GRID_PARTS 120
#define DH_MAX_VARIANCE_ROT 400.0
#define DH_MAX_VARIANCE_OFFSET 5200.0f
#define DH_MEANSHIFT_KERNEL_SIZE 20
#define DH_PROB_GATE 0.7

/* One split node.  Replaces houghforest.rs:63-68 `NodeParam{r1: Rect, r2: Rect, threshold: f64}`
 * plus the child links stamm keeps.  r = {x0, y0, x1, y1}: Rect.topleft / Rect.bottomright
 * (src/types.rs:33-37), relative to the patch.  child >= 0 is a node index, child < 0 is the leaf
 * ~child.  child_one is taken when avg(r1) - avg(r2) > threshold (Binar::One,
 * houghforest.rs:185-193), child_zero otherwise. */
typedef struct dh_node {
    uint16_t r1[4];
    uint16_t r2[4];
    double   threshold;
    int32_t  child_zero;
    int32_t  child_one;
} dh_node; /* 32 bytes */

/* Host-side description of a forest; dh_forest_create copies everything.  Replaces the serde
 * model `RandomForest<LeafParam, HoughTreeFunctions>` (prediction.rs:33-34) with
 * `LeafParam{prob: f64, offsets: Vec<Vec3<f32>>, rotations: Vec<Vec3<f64>>}` (houghforest.rs:73-78)
 * in CSR form. */
typedef struct dh_forest_desc {
    uint32_t        n_trees;
    const int32_t  *roots;      /* [n_trees] node index, or ~leaf for a single-leaf tree */
    uint32_t        n_nodes;
    const dh_node  *nodes;      /* [n_nodes] */
    uint32_t        n_leaves;
    const double   *leaf_prob;  /* [n_leaves] */
    const uint32_t *off_begin;  /* [n_leaves + 1] into offsets   */
    const uint32_t *rot_begin;  /* [n_leaves + 1] into rotations */
    const float    *offsets;    /* [off_begin[n_leaves] * 3] mm      */
    const double   *rotations;  /* [rot_begin[n_leaves] * 3] degrees */
} dh_forest_desc;

/* The serialised scalars of `HoughPrediction` (prediction.rs:239-256). */
typedef struct dh_params {
    uint32_t stepwidth;
    uint32_t subimage_width;
    uint32_t subimage_height;
    float    gaussian_sigma;        /* used as the VARIANCE of the kernel, prediction.rs:314 */
    uint32_t meanshift_iterations;
} dh_params;

/* `PredictionResult` (prediction.rs:259-267).  bounding_box is always Rect(0,0,0,0) there
 * (:491) and is not carried here: the *_support calls report it in a dh_support record.  36 payload
 * bytes; `reserved` fills the natural padding and is 0. */
typedef struct dh_pose {
    float    mid_point[3]; /* mm, camera space, integer-valued          */
    uint32_t reserved;
    double   rotation[3];  /* radians, multiples of 3.14159/60          */
} dh_pose; /* 40 bytes */

typedef struct dh_forest dh_forest;       /* opaque, immutable */
typedef struct dh_predictor dh_predictor; /* opaque, one per thread/stream */

/* Average duration of each kernel over the last batch, when profiling is on. */
typedef struct dh_timing {
    float traverse_ms; /* tile build + background gate + tree walks (excludes boxsum_ms, emit_ms) */
    float vote_ms;     /* coarse 20x20 / 20^3 guess grids                    */
    float cluster_ms;  /* initial guesses + both mean shifts                 */
    float total_ms;    /* first kernel start -> last kernel end              */
    uint32_t n_frames;
    float boxsum_ms;   /* rectangle-sum images or pixel flags, and the list of flagged tiles */
    float emit_ms;     /* probability gate + hit records                     */
    uint32_t reserved;
} dh_timing;

const char *dh_last_error(void);
int dh_version(void);

/* Validate and copy a forest.  Rejected with DH_EFOREST where the reference would panic or read
 * out of bounds: child/root index out of range, a node reachable twice (cycle / DAG), a rectangle
 * with x1 < x0 or y1 < y0 (u32 underflow, types.rs:47-52), non-monotone CSR arrays, a leaf with
 * prob > 0 and no offset (division by zero, prediction.rs:594) or no rotation (unwrap of None,
 * :600), a rotation whose bin leaves [0,120) after the single wrap (index out of bounds, :636). */
int dh_forest_create(const dh_forest_desc *desc, dh_forest **out);
int dh_forest_destroy(dh_forest *f);
int dh_forest_info(const dh_forest *f, uint32_t *n_trees, uint32_t *n_nodes, uint32_t *n_leaves,
                   uint32_t *max_depth);

/* Upload the forest to `device`, precompute the per-leaf vote tables on the GPU and build the
 * mean-shift kernel table (get_or_build_kernel, prediction.rs:310-317).  Rejects (DH_EFOREST) a
 * split rectangle that leaves the patch and (DH_ESIZE) a patch whose pixel sum can exceed 2^32.
 * One window's summed-area table must also fit the 160 KB LDS of a CU: the first batch / reserve call
 * refuses (DH_ESIZE) patches beyond about 195 x 195 (the reference's only trainer uses 80 x 80). */
int dh_predictor_create(const dh_forest *f, const dh_params *p, int device, dh_predictor **out);
int dh_predictor_destroy(dh_predictor *p);
/* HoughPrediction::update_sigma / sigma (prediction.rs:320-331): no-op for val <= 0 or unchanged. */
int dh_predictor_update_sigma(dh_predictor *p, float val);
int dh_predictor_sigma(const dh_predictor *p, float *out);

/* predict_parameter_parallel over n frames held in HOST memory (row-major u16, index y*w+x,
 * types.rs:10).  K: row-major 3x3 intrinsic (types.rs:405).  midp_guess (n*3 f32) / rot_guess
 * (n*3 f64, radians) are the Option<> arguments: NULL = None for every frame; guess_mask (n bytes,
 * may be NULL = all present) selects per frame: bit0 = midp_guess is Some, bit1 = rot_guess is
 * Some.  Synchronous: copies in, runs, copies out.  The upload is pipelined: frames cross PCIe in chunks while the
 * kernels of the previous chunk run (without dh_debug_enable the parity taps then describe the LAST chunk only). */
int dh_predict_batch(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                     const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                     dh_pose *out);

/* Page-locked host memory for frame buffers (a camera driver or file reader writes frames there): dh_predict_batch
 * then uploads by asynchronous DMA at PCIe speed, chunk k + 1 while the kernels of chunk k run.  Pageable buffers work
 * too, more slowly (the runtime pins and unpins the pages of every copy). */
int dh_host_alloc(size_t bytes, void **out);
int dh_host_free(void *ptr);

/* The same batch handed over as BIWI run-length coded depth payloads -- the bytes of the `.bin` files that
 * db_reader::biwi::read_depth (src/db_reader/biwi.rs:81-103) parses: bufs[i] / lens[i] = payload of frame i; every
 * frame must decode to the same w x h.  The host only walks the run headers (with the checks of dh_biwi_decode_depth:
 * a truncated payload or a run that overruns the image gives DH_EINVAL BEFORE anything is launched); payloads and
 * the run table cross PCIe instead of the 2-byte pixels (a BIWI frame is ~80 % background), the depth images are
 * rebuilt on the device, byte for byte what dh_biwi_decode_depth yields, and predicted.  Synchronous. */
int dh_predict_batch_rle(dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n, const float K[9],
                         const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out);
/* The decode step alone: n payloads -> DEVICE frames [n][h][w] u16 (frames_dev == NULL: validate and return
 * *w, *h only).  Synchronous (returns when the frames are in place). */
int dh_biwi_decode_depth_device(dh_predictor *p, const uint8_t *const *bufs, const size_t *lens, int n,
                                uint16_t *frames_dev, size_t cap_px, uint32_t *w, uint32_t *h);

/* Same with DEVICE pointers (frames, guesses, mask, out all device-resident) on `stream`
 * (a hipStream_t; NULL = default stream).  Asynchronous: returns after enqueueing; buffers must
 * stay valid until the stream reaches this point.  Performs no allocation and no host
 * synchronisation once the workspace for (n, w, h) exists, so it can be captured in a hipGraph
 * (call dh_predictor_reserve first). */
int dh_predict_batch_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h,
                            const float K[9], const float *midp_guess, const double *rot_guess,
                            const uint8_t *guess_mask, dh_pose *out, void *stream);

/* ---- sibling consumers of the tree walk (same kernel, different epilogue) ----
 * HoughPrediction::predict_mask (prediction.rs:850-905): per window the mean leaf probability,
 * as u8 = (prob * 255) painted into a stepwidth x stepwidth block; mask is n*h*w bytes. */
int dh_predict_mask(dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask);
int dh_predict_mask_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, uint8_t *mask,
                           void *stream);
/* The VOTING stage of HoughPrediction::build_hough_image (prediction.rs:760-840): every leaf with
 * prob >= 0.95 casts (255 * prob) / n_offsets at the projected vote pixel, u16 wrapping.  out is
 * n*h*w u16, the image the reference then passes to imageproc::filter::gaussian_blur_f32 (:844):
 * dh_build_hough_image below adds that blur, dh_predict_from2dhough the argmax of :343-367. */
int dh_hough_image(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                   uint16_t *out);
int dh_hough_image_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                          uint16_t *out, void *stream);

/* HoughPrediction::build_hough_image IN FULL (prediction.rs:760-845): the votes above passed through
 * imageproc::filter::gaussian_blur_f32(_, gaussian_sigma) (:844) -- a separable Gaussian with taps at 0..ceil(2 sigma),
 * f32 accumulation in tap order, each pass clamped and truncated to u16, image borders replicated.  imageproc 0.12.0
 * (Cargo.lock:555) is an external crate whose source is not vendored: PARITY UNPINNED, the blur restates the crate's
 * published algorithm (see oracle/dh_oracle.c orc_gaussian_blur_u16).  Needs gaussian_sigma > 0 (the crate asserts). */
int dh_build_hough_image(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], uint16_t *out);
int dh_build_hough_image_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                                uint16_t *out, void *stream);
/* HoughPrediction::predict_parameter_from2dhough (prediction.rs:343-367): argmax of that image -- `max_by_key`
 * keeps the LAST of equal maxima -- lifted to 3-D with the frame's depth at that pixel (img_to_space_coord);
 * rotation is always (0, 0, 0) there (:363). */
int dh_predict_from2dhough(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], dh_pose *out);
int dh_predict_from2dhough_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                                  dh_pose *out, void *stream);

/* hipGraph path for launch-bound use (single frames, small frames): capture ONE
 * dh_predict_batch_device call -- device pointers, sizes and K are baked in -- then replay it with one
 * host call per batch; new inputs are written into the same buffers between replays. */
int dh_graph_capture(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                     const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out);
int dh_graph_launch(dh_predictor *p, void *stream);
int dh_graph_destroy(dh_predictor *p);

/* Allocate the workspace for batches of up to n frames of w x h. */
int dh_predictor_reserve(dh_predictor *p, int n, int w, int h);

/* Forked sub-batches inside one device call.  A call of >= 512 frames on an otherwise idle GPU runs faster as two halves on two
 * streams (the latency-bound tail kernels of one half beside the head kernels of the other); a caller that keeps several
 * predictors in flight already has that overlap and loses to the fork's event plumbing (MI355X, 512 frames per call, four
 * predictors: 669 k frames/s forked, 713 k whole).  chunks: 0 = automatic (two halves from 512 frames on; the default, or
 * DH_CHUNKS), 1 = never fork, 2 .. 8 = that many.  No counterpart in the reference (rayon decides there). */
int dh_predictor_set_forking(dh_predictor *p, int chunks);

/* Number of sliding-window positions for a frame size (prediction.rs:535-548, 684-686). */
int dh_patch_grid(const dh_params *p, int w, int h, int *nx, int *ny);

/* ---- several cameras in one batch; live head tracking (examples/live_prediction.rs) ----
 * A dh_cameras table holds n intrinsic matrices on one device.  It is immutable once created and may be shared by predictors
 * of that device.  In a camera batch, frame i is seen by camera i of the table: its inverse is the same dh_mat3_inv_f32 a
 * single-K batch computes, so a table of n copies of K predicts exactly what dh_predict_batch(K) does. */
typedef struct dh_cameras dh_cameras;
int dh_cameras_create(const float *K /* [n][9] row-major */, int n, int device, dh_cameras **out);
int dh_cameras_destroy(dh_cameras *c);
/* frame i uses camera i; n <= the table's count; guesses / poses as dh_predict_batch(_device).  DH_EINVAL: the table lives
 * on another device than the predictor, more frames than cameras, NULL arguments. */
int dh_predict_batch_cameras(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                             const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out);
int dh_predict_batch_cameras_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                    const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, dh_pose *out,
                                    void *stream);

/* A tracker feeds each camera's pose back as that camera's next guess, on the device (live_prediction.rs:79-101):
 *   DH_TRACK_PREV_GUESS  the stored midpoint is the next midpoint guess when its z > 500 mm, the stored rotation the next
 *                        rotation guess once there is one (--prevguess; without it every step predicts without guesses);
 *   DH_TRACK_SLUGGISH    the stored midpoint moves only when the new one is within an L1 distance of 100 mm of it, or when
 *                        its z < 500 mm (--sluggish).
 * The state -- midpoint [n][3] f32, rotation [n][3] f64, guess mask [n] u8 -- lives on the tracker's device and is what the
 * next step's kernels read as their guesses.  A step predicts one frame per camera (frames [n_cams][h][w]) and then updates
 * the cameras whose `present` byte is non-zero (all of them when present is NULL); absent cameras are predicted with their
 * current guesses and keep their state.  One tracker's steps must be stream-ordered: a step reads the state the previous
 * one wrote.  After dh_predictor_reserve(p, n_cams, w, h) the device step allocates nothing and does not synchronise. */
#define DH_TRACK_PREV_GUESS 1u
#define DH_TRACK_SLUGGISH 2u
typedef struct dh_tracker dh_tracker;
int dh_tracker_create(const dh_cameras *c, uint32_t flags, dh_tracker **out);   /* the table must outlive the tracker */
int dh_tracker_destroy(dh_tracker *t);
/* the reference's initial state, [0,0,0], no rotation, mask 0, for one camera or all (camera = -1); stream-ordered */
int dh_tracker_reset(dh_tracker *t, int camera, void *stream);
int dh_tracker_step(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out);
int dh_tracker_step_device(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                           dh_pose *out, void *stream);
/* synchronous copy-out, each pointer nullable: midp [n][3], rot [n][3], flags [n] = guess mask | 4 once a rotation is stored */
int dh_tracker_state(dh_tracker *t, float *midp, double *rot, uint8_t *flags);
/* capture one dh_tracker_step_device (device pointers) into the predictor's graph slot; replay with dh_graph_launch.  Each
 * replay is one step.  Like a captured batch it is refused (DH_ESTATE) once the workspace has been reallocated. */
int dh_tracker_capture(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, dh_pose *out);

/* ---- vote support of each pose: head bounding box and confidence ----
 * Not in the reference, which computes none of it.  For frame f with final midpoint cell m = (int)mid_point and a radius r
 * (cells = mm), the frame's POSITION VOTES are exactly the votes the reference adds to its midpoint accumulator
 * (prediction.rs:590-667): windows past the 0.7 gate, leaves with prob > 0 whose offsets pass the covariance gate, every
 * offset o with p3 - o not negative in z, in cell c = (int)(p3 - o).  A vote SUPPORTS the pose when max_k |c_k - m_k| <= r
 * (evaluated in 64 bits).  Per frame:
 *   x, y, width, height  the Rect (types.rs:33-61) spanned by the CENTRE pixels (prediction.rs:544-552) of the windows with at
 *                        least one supporting vote: x = min cx, width = max cx - min cx + 1.  All 0 when nothing supports,
 *                        i.e. the reference's Rect(0,0,0,0).  The union of those windows' patch rectangles is this box
 *                        grown by subimage_width / 2 and subimage_height / 2 on every side.
 *   windows              distinct windows with at least one supporting vote
 *   hits                 (window, tree) pairs with at least one supporting vote
 *   mass                 sum of valtoadd over the supporting votes (exact, 64 bits)
 *   total_mass           the same sum over all position votes of the frame; mass / total_mass is the pose's confidence
 * Integer throughout: the record is bit-identical run to run.  The poses of these calls are byte-identical to those of the
 * plain calls.  `support` has one record per frame (host memory for the host calls, device memory for the _device calls).
 * radius: at most 2^31 - 1 (DH_EINVAL otherwise, e.g. a negative int passed).  The first support call of a workspace
 * allocates its scratch (4 bytes per (window, tree) pair and frame); after that the _device calls allocate nothing and do
 * not synchronise.  The plain entry points are unaffected: they launch exactly the kernels they launch without it. */
#define DH_SUPPORT_RADIUS 30   /* chosen by measurement: DESIGN.md section 13 */
typedef struct dh_support {
    uint32_t x, y, width, height;   /* Rect of the supporting windows' centre pixels */
    uint32_t windows;
    uint32_t hits;
    uint64_t mass;                  /* (byte offset 24: the record has no padding) */
    uint64_t total_mass;
} dh_support; /* 40 bytes */
int dh_predict_batch_support(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                             const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius,
                             dh_pose *out, dh_support *support);
int dh_predict_batch_support_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9],
                                    const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius,
                                    dh_pose *out, dh_support *support, void *stream);
int dh_predict_batch_cameras_support(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                     const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask, uint32_t radius,
                                     dh_pose *out, dh_support *support);
int dh_predict_batch_cameras_support_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                            const float *midp_guess, const double *rot_guess, const uint8_t *guess_mask,
                                            uint32_t radius, dh_pose *out, dh_support *support, void *stream);
/* one record per camera, absent ones included; the tracker's state is updated exactly as by dh_tracker_step(_device) */
int dh_tracker_step_support(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                            uint32_t radius, dh_pose *out, dh_support *support);
int dh_tracker_step_support_device(dh_predictor *p, dh_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                   uint32_t radius, dh_pose *out, dh_support *support, void *stream);

/* ---- several heads per frame ----
 * Not in the reference, which returns one pose per frame: PARITY UNPINNED, the definition below is this library's.  For frame f,
 * max_heads in 1 .. DH_MAX_HEADS and a radius r as in the support calls:
 *   1. the position votes are those of section 13; each vote (value v, cell c) also adds to one cell g of the 20 x 20 guess
 *      grid, the cell the reference's projection and clamp give it (prediction.rs:660-676);
 *   2. seed cells: the 400 grid cells in the order (count descending, index ascending); a cell with count > 0 is picked when it
 *      lies more than DH_HEADS_SUPPRESS cells (Chebyshev, on the grid) from every cell picked before; at most max_heads picks.
 *      The first pick is the reference's own guess cell (prediction.rs:694-704);
 *   3. seed k = floor(sum v * c / sum v) per axis over the votes of pick k (exact: 128-bit sums);
 *   4. the position mean shift of the plain call from each seed, over the frame's whole position accumulator: mid_k;
 *   5. head k's dh_support record for m = mid_k and radius r;
 *   6. its rotation: the plain call's rotation rule (coarse-grid argmax, mean shift) over the rotation votes of the hits
 *      (window, tree) that support head k only.  At r = 2^31 - 1 every hit supports every head: each rotation is the plain one;
 *   7. heads with mass 0 are dropped; walking the rest in seed order, a head whose mid_point lies within
 *      DH_MEANSHIFT_KERNEL_SIZE cells (Chebyshev) of a head kept before is dropped; the survivors ordered by mass descending,
 *      ties by seed order.  n_heads[f] of them fill heads[f][0 .. n_heads[f]); slots up to max_heads - 1 are zero.
 * Integer or the plain call's f32 / f64 rules throughout: bit-identical run to run.  heads is [n][max_heads] (host memory for the
 * host calls, device memory for the _device calls), n_heads [n].  DH_EINVAL before anything is launched: max_heads 0 or above
 * DH_MAX_HEADS, a radius above 2^31 - 1, NULL arguments, a camera table of another device.  The first heads call of a workspace
 * allocates its scratch; after that the _device calls allocate nothing and do not synchronise.  No guesses: heads start from
 * their seeds. */
#define DH_MAX_HEADS 4
#define DH_HEADS_SUPPRESS 2    /* guess-grid cells */
typedef struct dh_head {
    dh_pose pose;
    dh_support support;
} dh_head; /* 80 bytes */
int dh_predict_heads(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads, uint32_t radius,
                     uint32_t *n_heads, dh_head *heads);
int dh_predict_heads_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const float K[9], int max_heads,
                            uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream);
int dh_predict_heads_cameras(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads,
                             uint32_t radius, uint32_t *n_heads, dh_head *heads);
int dh_predict_heads_cameras_device(dh_predictor *p, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, int max_heads,
                                    uint32_t radius, uint32_t *n_heads, dh_head *heads, void *stream);

/* ---- several heads per camera with persistent identities ----
 * Not in the reference: PARITY UNPINNED, the definition below is this library's.  A multi-head tracker keeps, per camera,
 * DH_MAX_TRACKS track slots and next_id (1 when created or reset).  A step runs the heads calls above (max_heads and radius of
 * the params) on one frame per camera and then, for each camera whose `present` byte is non-zero (all when present is NULL),
 * with n = n_heads[c] and its heads:
 *   1. the cell of every live track's (id != 0) head.pose.mid_point and of every head's mid_point: (int32_t) per axis as the
 *      support calls convert it (NaN -> 0, saturating), widened to 64 bits;
 *   2. d(t, j): the Chebyshev distance of the two cells, in 64 bits;
 *   3. pairs with d <= gate are taken greedily in the order (d ascending, head j ascending, slot t ascending); a pair is
 *      accepted when neither its track nor its head is taken yet;
 *   4. a matched track takes the whole 80-byte head; hits and age + 1, misses = 0; ids[c][j] = its id;
 *   5. an unmatched live track: age + 1, misses + 1; when misses > max_misses its slot is zeroed (freed);
 *   6. unmatched heads in ascending j each take the lowest free slot: id = next_id, age = hits = 1, misses = 0, the head;
 *      next_id + 1, wrapping from UINT32_MAX to 1 (0 is never an id); ids[c][j] = id.  With no free slot ids[c][j] = 0;
 *   7. ids[c][j] = 0 for j >= n.
 * age, hits and misses saturate at UINT32_MAX.  An absent camera keeps its state and gets ids of zeros; its heads are computed
 * and written all the same.  Integer only: bit-identical run to run.  Ids are unique per camera until 2^32 - 1 births have
 * happened since the last reset.  Defaults (choices, not measurements): gate 100 cells = mm admits 3 m/s at 30 Hz and is five
 * times the 20-cell merge distance of the heads calls; 3 misses coast for 100 ms at 30 Hz.
 * heads and ids are [n_cams][max_heads], n_heads [n_cams], tracks (nullable: the records of every camera after the step)
 * [n_cams][DH_MAX_TRACKS]; host memory for the host calls, device memory for the _device and capture calls.  DH_EINVAL before
 * anything is launched: NULL arguments, max_heads outside 1 .. DH_MAX_HEADS, radius or gate above 2^31 - 1, a camera out of
 * range in reset, a camera table of another device.  One tracker's steps must be stream-ordered.  After
 * dh_predictor_reserve(p, n_cams, w, h) and one heads call of that workspace the device step allocates nothing and does not
 * synchronise; the capture call does both itself before it captures, and is refused (DH_ESTATE) like the other captures once
 * the workspace has been reallocated. */
#define DH_MAX_TRACKS 8
#define DH_TRACK_GATE 100
#define DH_TRACK_MAX_MISSES 3
typedef struct dh_head_track {
    uint32_t id;          /* 0 = free slot */
    uint32_t age;         /* present steps since birth, saturating */
    uint32_t hits;        /* steps matched (birth counts), saturating */
    uint32_t misses;      /* consecutive present steps without a match */
    dh_head head;         /* last matched head */
} dh_head_track;          /* 96 bytes */
typedef struct dh_multi_track_params {
    int32_t max_heads;    /* 1 .. DH_MAX_HEADS, passed to the heads pipeline */
    uint32_t radius;      /* support radius of the heads pipeline, 0 .. 2^31 - 1 */
    uint32_t gate;        /* cells (= mm), 0 .. 2^31 - 1; default DH_TRACK_GATE */
    uint32_t max_misses;  /* default DH_TRACK_MAX_MISSES */
} dh_multi_track_params;  /* 16 bytes */
typedef struct dh_multi_tracker dh_multi_tracker;
int dh_multi_tracker_create(const dh_cameras *c, const dh_multi_track_params *prm, dh_multi_tracker **out);   /* the table must outlive it */
int dh_multi_tracker_destroy(dh_multi_tracker *t);
/* the created state (every slot free, next_id 1) for one camera or all (camera = -1); stream-ordered */
int dh_multi_tracker_reset(dh_multi_tracker *t, int camera, void *stream);
int dh_multi_tracker_step(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                          uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks);
int dh_multi_tracker_step_device(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                 uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks, void *stream);
/* synchronous copy-out, each pointer nullable: tracks [n_cams][DH_MAX_TRACKS], next_id [n_cams] */
int dh_multi_tracker_state(dh_multi_tracker *t, dh_head_track *tracks, uint32_t *next_id);
/* capture one dh_multi_tracker_step_device (device pointers) into the predictor's graph slot; each dh_graph_launch is one step */
int dh_multi_tracker_capture(dh_predictor *p, dh_multi_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                             uint32_t *n_heads, dh_head *heads, uint32_t *ids, dh_head_track *tracks);

/* ---- camera rigs: heads fused across cameras into tracks with rig-wide identities ----
 * Not in the reference (one pose from one Kinect): PARITY UNPINNED, the definition below is this library's, and its constants
 * are choices.  A RIG is a group of cameras that look at one space and share one world frame.  A rig table gives every camera c
 * of a camera table its extrinsics: the camera-space point m is the world point R_c * m + t_c (R row-major, t in mm).  R is
 * NOT required to be orthonormal: the library only applies it, it never inverts it.  Rig g owns the cameras
 * rig_begin[g] .. rig_begin[g + 1] - 1; the ranges are ascending, cover 0 .. n exactly, and each holds 1 .. DH_RIG_MAX_CAMERAS
 * cameras (the views of a person are a 64-bit mask).  The table is immutable, lives on the camera table's device, and the camera
 * table must outlive it.  dh_rig_create answers DH_EINVAL before anything is allocated for: NULL arguments, n_rigs < 1, ranges
 * that are not ascending or do not cover the table, an empty or too large rig, a non-finite entry of R or t.
 *
 * A rig tracker keeps, per rig, DH_RIG_MAX_TRACKS track slots and next_id (1 when created or reset).  A step runs the heads calls
 * of section 14 (max_heads and radius of the params) on one frame per camera, exactly as dh_predict_heads_cameras(_device), and
 * then, per rig, over the heads (c, j), j < min(n_heads[c], max_heads), of its PRESENT cameras (present[c] != 0; all when present
 * is NULL):
 *   0. world midpoint of head k with camera-space mid_point m: w_q = ((R[q][0] * m_0 + R[q][1] * m_1) + R[q][2] * m_2) + t_q in
 *      f32, every product and sum rounded on its own, in exactly that order.  Its world cell: (int32_t) per axis as the support
 *      calls convert (NaN -> 0, saturating), widened to 64 bits.  All distances are Chebyshev distances of cells in 64 bits;
 *   1. ORDER the heads by (support.mass descending, camera c ascending, j ascending);
 *   2. FUSE: walking the heads in that order, a head joins the first person (in order of creation) whose ANCHOR cell is within
 *      fuse_gate (d <= fuse_gate) and that has no member from the same camera yet; otherwise it founds a new person, and its cell
 *      is that person's anchor; when DH_RIG_MAX_PERSONS persons exist already it stays unassigned.  (Two heads of one camera
 *      were told apart by section 14's merge rule and are never the same person.)
 *   3. PERSON RECORD: cell = floor(sum of the members' world cells / members) per axis (exact in 64 bits, floor toward minus
 *      infinity); views = bit (c - rig_begin[g]) for every member camera c; n_views; mass = the members' support.mass summed,
 *      saturating at UINT64_MAX; best_cam / best_head = the anchor's (c, j), c being the index in the camera table (its heaviest
 *      view: heads[c][j] carries the rotation in that camera's frame); world = the anchor's f32 world midpoint;
 *   4. MATCH the persons against the rig's track slots as section 15 matches heads against a camera's: d(t, i) between the cell
 *      of live track t's person record and person i's cell; pairs with d <= gate taken greedily in the order (d, person i, slot t)
 *      ascending; a matched track takes the whole person record, hits and age + 1, misses = 0; an unmatched live track age + 1,
 *      misses + 1, zeroed (freed) when misses > max_misses; unmatched persons in ascending i each take the lowest free slot with
 *      id = next_id, age = hits = 1, misses = 0 (next_id + 1, wrapping from UINT32_MAX to 1: 0 is never an id), or get id 0 when
 *      no slot is free.  age, hits, misses saturate at UINT32_MAX.  A person record's id is its track's id, in the persons output
 *      and in the track record alike;
 *   5. OUTPUTS: rig_ids[c][j] = the id of the person head (c, j) belongs to; 0 for unassigned heads, for j >= n, and for every
 *      head of an absent camera.  n_persons[g], persons[g][DH_RIG_MAX_PERSONS] (unused records zero) and, when asked, the
 *      snapshot tracks[g][DH_RIG_MAX_TRACKS] after the step.  n_heads and heads are written for every camera, absent ones
 *      included, byte-identical to dh_predict_heads_cameras(_device) on the same frames;
 *   6. a rig with NO present camera in a step keeps its whole state (no ageing; n_persons 0, ids 0); a rig with present cameras
 *      but no head ages its tracks.  An absent camera contributes nothing.
 * Integer apart from step 0's three products and three sums: bit-identical run to run, and to the sequential statement of the
 * rule in depthhead_amd/csrc/dh_rig.h.  Defaults (choices): DH_RIG_FUSE_GATE 100 cells = mm -- the section 14 quality runs
 * place a detected head within about 90 mm of the truth, so two views of one head can lie that far apart; gate DH_TRACK_GATE and max_misses
 * DH_TRACK_MAX_MISSES as section 15.  DESIGN.md section 16 measures them on two parallel views of two-head scenes (ids held,
 * fused cell within 54 mm of the truth); it does not measure the gate against two different people closer than 100 mm.
 * heads and rig_ids are [n_cams][max_heads], n_heads [n_cams], n_persons [n_rigs], persons [n_rigs][DH_RIG_MAX_PERSONS], tracks
 * (nullable) [n_rigs][DH_RIG_MAX_TRACKS]; host memory for the host calls, device memory for the _device and capture calls.
 * DH_EINVAL before anything is launched: NULL arguments, max_heads outside 1 .. DH_MAX_HEADS, radius, fuse_gate or gate above
 * 2^31 - 1, a rig out of range in reset, a rig table of another device than the predictor.  One tracker's steps must be
 * stream-ordered.  After dh_predictor_reserve(p, n_cams, w, h) and one heads call of that workspace the device step allocates
 * nothing and does not synchronise; the capture call does both itself before it captures.  The host step runs the heads
 * pipeline in resident slices of cameras and fuses once, after the last slice, over the heads of the whole table: a rig is
 * never cut in two. */
#define DH_RIG_MAX_CAMERAS 64
#define DH_RIG_MAX_PERSONS 16
#define DH_RIG_MAX_TRACKS 16
#define DH_RIG_FUSE_GATE 100
typedef struct dh_rig_person {
    uint64_t views;       /* bit k: camera rig_begin[g] + k sees this person */
    uint64_t mass;        /* the members' support.mass summed, saturating */
    int32_t cell[3];      /* floor of the mean of the members' world cells */
    uint32_t n_views;
    float world[3];       /* the anchor's world midpoint */
    uint32_t id;          /* the person's track id; 0: no free slot */
    uint32_t best_cam;    /* the anchor: camera (index in the camera table) and head of its heaviest view */
    uint32_t best_head;
} dh_rig_person;          /* 56 bytes, no padding */
typedef struct dh_rig_track {
    uint32_t id;          /* 0 = free slot */
    uint32_t age;         /* steps of the rig (with a present camera) since birth, saturating */
    uint32_t hits;        /* steps matched (birth counts), saturating */
    uint32_t misses;      /* consecutive steps without a match */
    dh_rig_person person; /* last matched person */
} dh_rig_track;           /* 72 bytes, no padding */
typedef struct dh_rig_track_params {
    int32_t max_heads;    /* 1 .. DH_MAX_HEADS, passed to the heads pipeline */
    uint32_t radius;      /* support radius of the heads pipeline, 0 .. 2^31 - 1 */
    uint32_t fuse_gate;   /* cells (= mm), 0 .. 2^31 - 1; default DH_RIG_FUSE_GATE */
    uint32_t gate;        /* cells (= mm), 0 .. 2^31 - 1; default DH_TRACK_GATE */
    uint32_t max_misses;  /* default DH_TRACK_MAX_MISSES */
} dh_rig_track_params;    /* 20 bytes */
typedef struct dh_rig dh_rig;
typedef struct dh_rig_tracker dh_rig_tracker;
int dh_rig_create(const dh_cameras *c, const float *R /* [n][9] row-major */, const float *t /* [n][3] mm */,
                  const int32_t *rig_begin /* [n_rigs + 1] */, int n_rigs, dh_rig **out);
int dh_rig_destroy(dh_rig *r);
int dh_rig_tracker_create(const dh_rig *r, const dh_rig_track_params *prm, dh_rig_tracker **out);   /* the rig table must outlive it */
int dh_rig_tracker_destroy(dh_rig_tracker *t);
/* the created state (every slot free, next_id 1) for one rig or all (rig = -1); stream-ordered */
int dh_rig_tracker_reset(dh_rig_tracker *t, int rig, void *stream);
int dh_rig_tracker_step(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                        uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons,
                        dh_rig_track *tracks);
int dh_rig_tracker_step_device(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                               uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons,
                               dh_rig_track *tracks, void *stream);
/* synchronous copy-out, each pointer nullable: tracks [n_rigs][DH_RIG_MAX_TRACKS], next_id [n_rigs] */
int dh_rig_tracker_state(dh_rig_tracker *t, dh_rig_track *tracks, uint32_t *next_id);
/* capture one dh_rig_tracker_step_device (device pointers) into the predictor's graph slot; each dh_graph_launch is one step */
int dh_rig_tracker_capture(dh_predictor *p, dh_rig_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                           uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons,
                           dh_rig_track *tracks);

/* ---- rendering posed meshes to depth frames and head masks ----
 * The reference draws its head model for display only (utils/src/headwin.rs); a renderer that produces the depth frame and head
 * mask a Kinect would have recorded is not in it: PARITY UNPINNED, the definition below is this library's.  A batch is n frames of
 * w x h and a list of instances; instance i draws mesh `mesh` into frame `frame` with vertex v carried to
 *     p[j] = ((R[j][0] * sv0 + R[j][1] * sv1) + R[j][2] * sv2) + t[j],  sv = v * scale                       (f32, no contraction)
 * and projected by the frame's intrinsic matrix as space_to_img_coord does (r = K p in the reference's mat-vec order, x = r0 / r2,
 * y = r1 / r2), snapped to 1/16 pixel: s = floorf(x * 16.0f + 0.5f).  A triangle is dropped whole (never clipped) when a vertex
 * has p.z < 1.0f, a snapped coordinate is not finite or lies outside +-2^20, or its area is zero; both windings are drawn.  A pixel
 * is covered when its centre (16 x + 8, 16 y + 8) lies inside the triangle by int64 edge functions with a top-left fill rule
 * (triangles sharing an edge cover every pixel along it exactly once).  Depth at a covered pixel, in f64 from the edge values e_i
 * and iz_i = 1.0 / (double)p_i.z:  z = (double)(e0 + e1 + e2) / ((e0 * iz0 + e1 * iz1) + e2 * iz2),  d = (uint32)(z + 0.5) clamped to
 * [1, 65535].  Every pixel keeps the smallest key (d << 1) | (head ? 0 : 1) over all triangles of its frame's instances (order-free;
 * a head wins a depth tie): frames = d of that key or 0 where nothing was drawn, masks = 1 where the key is a head's, else 0.
 * Sensor model, per pixel index k = (frame * h + y) * w + x with u(c) = the splitmix64 output number c (from 0) of the stream seeded
 * with `seed`: a foreground pixel becomes clamp(d + (int)(u(2k) % (2a + 1)) - a, 1, 65535) with a = noise_amplitude, and then 0 (a
 * hole) when (u(2k + 1) >> 11) < floor(hole_probability * 2^53).  Holes leave the mask as it is.  a = 0 and probability 0: no change.
 * Bit-identical run to run and to tests/render_ref.py.
 * A dh_mesh is immutable and lives on one device; a dh_renderer owns the triangle records, tile lists and (for the host calls)
 * the output staging of one device, all growing on demand, and is NOT thread-safe.  instances, meshes, K and params are host
 * memory in every call.  DH_EINVAL before anything is launched, with the outputs untouched: NULL renderer / frames (masks may be
 * NULL: no mask is written), an instance naming a frame >= n or a mesh >= n_meshes, a mesh of another device, n < 1 or above
 * 65535, w or h outside 1 .. DH_RENDER_MAX_SIZE, hole_probability outside [0, 1] (NaN included), noise_amplitude above 65535, a
 * camera table of another device or whose length is not n.  The host calls are synchronous.  The _device calls take device
 * output pointers and enqueue on `stream` (NULL = default stream); they wait on the host once, for the size of the tile lists,
 * and their output is ordered before whatever is enqueued on that stream next (the _device prediction, tracker and rig calls). */
#define DH_RENDER_HEAD 1u          /* dh_render_instance.flags bit 0: the instance is a head (mask 1, wins depth ties) */
#define DH_RENDER_MAX_SIZE 16384   /* largest frame width or height */
typedef struct dh_render_instance {
    uint32_t frame;    /* 0 .. n - 1 */
    uint32_t mesh;     /* index into the call's mesh list */
    float    R[9];     /* row-major */
    float    t[3];     /* mm */
    float    scale;
    uint32_t flags;    /* DH_RENDER_HEAD */
} dh_render_instance;  /* 64 bytes, no padding */
typedef struct dh_render_params {
    uint32_t noise_amplitude;   /* a: integer noise in [-a, a]; 0 = none */
    uint32_t reserved0;
    double   hole_probability;  /* in [0, 1]; 0 = none */
    uint64_t seed;
    uint64_t reserved[2];       /* 0 */
} dh_render_params;    /* 40 bytes */
typedef struct dh_mesh dh_mesh;
typedef struct dh_renderer dh_renderer;
/* Copies nv vertices (x, y, z triples, mm) and nt triangles (index triples) to `device`.  DH_EINVAL: NULL arguments, nv or nt 0,
 * an index >= nv, a non-finite vertex. */
int dh_mesh_create(const float *verts, uint32_t nv, const uint32_t *tris, uint32_t nt, int device, dh_mesh **out);
int dh_mesh_destroy(dh_mesh *m);
/* each pointer nullable; bbox = min x, y, z then max x, y, z */
int dh_mesh_info(const dh_mesh *m, uint32_t *nv, uint32_t *nt, float bbox[6]);
int dh_renderer_create(int device, dh_renderer **out);
int dh_renderer_destroy(dh_renderer *r);
/* params NULL: no sensor model.  frames [n][h][w] u16, masks [n][h][w] u8 or NULL. */
int dh_render_depth(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances,
                    uint32_t n_instances, int n, int w, int h, const float K[9], const dh_render_params *params, uint16_t *frames,
                    uint8_t *masks);
/* frame i is seen through camera i of the table, which must hold exactly n cameras */
int dh_render_depth_cameras(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances,
                            uint32_t n_instances, int n, int w, int h, const dh_cameras *c, const dh_render_params *params,
                            uint16_t *frames, uint8_t *masks);
int dh_render_depth_device(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes, const dh_render_instance *instances,
                           uint32_t n_instances, int n, int w, int h, const float K[9], const dh_render_params *params,
                           uint16_t *frames, uint8_t *masks, void *stream);
int dh_render_depth_cameras_device(dh_renderer *r, const dh_mesh *const *meshes, uint32_t n_meshes,
                                   const dh_render_instance *instances, uint32_t n_instances, int n, int w, int h, const dh_cameras *c,
                                   const dh_render_params *params, uint16_t *frames, uint8_t *masks, void *stream);
/* device time of the last render's kernels in ms (setup, offsets, fill, resolve), measured with events when `on` was set by
 * dh_renderer_set_profiling before it; synchronises */
int dh_renderer_set_profiling(dh_renderer *r, int on);
int dh_renderer_timing(dh_renderer *r, float ms[4]);

/* ---- fitting posed models to depth frames ----
 * The step after a discriminative detector: the posed head model is fitted to the depth pixels (point-to-plane ICP with
 * projective association) from a rough pose, the forest's.  Not in the reference: PARITY UNPINNED, the definition below is this
 * library's.  The inverse of dh_render_depth*: frames and rough instances in, refined instances and one record each out.
 * A model is n points v_i (mm) with unit normals m_i.  An instance is a dh_render_instance: `mesh` is the model index, R, t and
 * scale widen to f64, `flags` is ignored.  Everything below is f64, evaluated left to right, every product, sum and quotient
 * rounded on its own (no contraction), with + - * /, compares and casts only: no library function runs on the device.
 * ONE PASS at pose (R, t) with gate g, for every point i of the model:
 *     sv = v * scale;  p[j] = ((R[j][0] * sv0 + R[j][1] * sv1) + R[j][2] * sv2) + t[j];  nrm[j] = (R[j][0] * m0 + R[j][1] * m1) + R[j][2] * m2
 *   skipped unless p.z >= 1.0;  c = (nrm0 * p0 + nrm1 * p1) + nrm2 * p2, skipped unless c < 0.0 (the point faces the camera);
 *   projected by the frame's K widened to f64 as space_to_img_coord does: r[j] = (p0 * K[j][0] + p1 * K[j][1]) + p2 * K[j][2],
 *   x = r0 / r2, y = r1 / r2, skipped unless 0.0 <= x < w and 0.0 <= y < h (NaN fails); the pixel is ((int)x, (int)y), the
 *   renderer's pixel-centre convention;  d = (double)depth there, skipped when d == 0 or unless |d - p.z| <= g;
 *     residual  r = c * (d / p.z - 1.0)      (the measured point on the model point's own ray, projected on the normal: no K^-1)
 *     q = p - t;  J = (nrm0, nrm1, nrm2, q1 * nrm2 - q2 * nrm1, q2 * nrm0 - q0 * nrm2, q0 * nrm1 - q1 * nrm0)
 *   and with S = 2^20 the int64 sums (truncating casts, so their order is free):  A_ab += (int64)((J_a * J_b) * S) for a <= b (21),
 *   b_a += (int64)((J_a * r) * S) (6),  e += (int64)((r * r) * S),  count += 1.  Magnitudes: R is held to |R R^T - I| <=
 *   DH_FIT_R_TOLERANCE per element, so |R x| <= 1.03 |x|; with |m| <= 1.01 that gives |nrm| <= 1.05, |q| <= 1.03 * 4096 and
 *   |J_a| <= 1.09 * 4096, and |r| <= 1.05 * (|p| / p.z) * g.  For a camera that sees no point further than 60 degrees off its axis
 *   (|p| <= 2 p.z: any field of view below 120 degrees) every product stays below 2^27; times 2^20, times 2^15 points: below
 *   2^62.  A K that lets points through at a wider angle is not refused, but there the sums can leave int64 and the result is
 *   unspecified (arithmetic only: nothing faults), and no longer pinned to the restatement, whose Python ints do not wrap.
 * ONE STEP from the sums of a pass: count < min_points ends the fit with DH_FIT_FEW_POINTS.  A_ab = (double)sum / S (A symmetric),
 *   b_a alike; A_aa = A_aa * (1.0 + lambda) + 1e-9; A x = b is solved on the leading n x n block (n = 3, the translation, in a coarse
 *   step, else 6) by Gaussian elimination without pivoting in index order:  for k < n: piv = A[k][k]; for i in k+1 .. n-1:
 *   f = A[i][k] / piv; A[i][j] = A[i][j] - f * A[k][j] for j in k+1 .. n-1; b[i] = b[i] - f * b[k];  then for i = n-1 .. 0:
 *   s = b[i]; s = s - A[i][j] * x[j] for j in i+1 .. n-1; x[i] = s / A[i][i].  A pivot that is not > 0.0 (NaN included) ends the fit
 *   with DH_FIT_SINGULAR and this step changes nothing.  Else t[j] = t[j] + x[j], and in a full step with a = x[3..5] / 2.0,
 *   q = (a0 * a0 + a1 * a1) + a2 * a2, s = 1.0 + q, d = 1.0 - q, u_i = 2.0 * a_i the Cayley rotation (rational: no trigonometry)
 *     C00 = (d + u0 * a0) / s   C01 = (u0 * a1 - u2) / s   C02 = (u0 * a2 + u1) / s
 *     C10 = (u1 * a0 + u2) / s   C11 = (d + u1 * a1) / s   C12 = (u1 * a2 - u0) / s
 *     C20 = (u2 * a0 - u1) / s   C21 = (u2 * a1 + u0) / s   C22 = (d + u2 * a2) / s
 *   turns the model about its own origin:  R[i][j] = (C[i][0] * R[0][j] + C[i][1] * R[1][j]) + C[i][2] * R[2][j].
 * SCHEDULE: coarse_iterations coarse steps at gate[0], then `iterations` full steps at gate[1].  A step after which every
 *   |x_a| < 1e-6 ends its phase early (a coarse one goes on to the full steps, a full one ends the fit).  One last pass at gate[1]
 *   at the final pose -- also after DH_FIT_FEW_POINTS and DH_FIT_SINGULAR -- gives the record's points (count) and sum_r2_fixed (e);
 *   steps counts the steps that were applied.  The output instance is the input's with R and t rounded to f32 once (frame, mesh,
 *   scale and flags copied through): it can be passed to dh_render_depth* as it is.  Bit-identical run to run and to tests/fit_ref.py.
 * A dh_fit_model is immutable and lives on one device; a dh_fitter owns the call's tables and (for the host calls) the frame and
 * output staging of one device, taken at the first fit and growing on demand, and is NOT thread-safe.  models, instances, K and
 * params are host memory in every call; params NULL selects dh_fit_params_default.  DH_EINVAL before anything is launched, with
 * the outputs untouched: NULL fitter / frames / out / records; n < 1 or above 65535; w or h outside 1 .. DH_RENDER_MAX_SIZE; NULL K,
 * or a NULL camera table, one of another device or one whose length is not n; instances or models NULL with n_instances > 0; an
 * instance naming a frame >= n or a model >= n_models; a NULL model or one of another device; a non-finite R, t or scale; an
 * R with an element of R R^T (in f64) further than DH_FIT_R_TOLERANCE from the identity's (what the magnitude bound above rests
 * on; a rotation rounded to f32 is within 1e-6); |scale| * (the model's largest |v|) above DH_FIT_MAX_EXTENT; coarse_iterations + iterations above 64; a gate
 * outside (0, 4096] (NaN included); lambda not >= 0 or not finite; min_points below 6; a reserved word that is not 0.
 * n_instances = 0 is no error and writes nothing.  The host calls are synchronous.  The _device calls take device frames and
 * device outputs, enqueue on `stream` (NULL = default stream) and never wait on the host for anything the device computes --
 * every pass and step of every instance runs inside one kernel launch -- and are ordered after whatever was enqueued on that stream before (a _device
 * render or prediction) and before whatever follows. */
#define DH_FIT_OK 0u
#define DH_FIT_FEW_POINTS 1u       /* a pass associated fewer than min_points points */
#define DH_FIT_SINGULAR 2u         /* a pivot of the normal equations was not > 0 */
#define DH_FIT_MAX_POINTS 32768u   /* points of a model */
#define DH_FIT_MAX_EXTENT 4096.0   /* mm: |scale| * largest |v| of an instance */
#define DH_FIT_R_TOLERANCE 0.02    /* largest |(R R^T - I)[i][j]| of an instance */
typedef struct dh_fit_params {
    uint32_t coarse_iterations;   /* 6: translation-only steps at gate[0] */
    uint32_t iterations;          /* 14: full steps at gate[1]; the two sum to at most 64 */
    double   gate[2];             /* 120, 25 (mm): each in (0, 4096] */
    double   lambda;              /* 1e-3: relative damping of the diagonal, >= 0 */
    uint32_t min_points;          /* 16, at least 6 */
    uint32_t reserved0;           /* 0 */
    uint64_t reserved[2];         /* 0 */
} dh_fit_params;       /* 56 bytes */
typedef struct dh_fit_record {
    uint32_t points;              /* points associated by the last pass */
    uint32_t steps;               /* steps applied */
    uint32_t status;              /* DH_FIT_* */
    uint32_t reserved;            /* 0 */
    int64_t  sum_r2_fixed;        /* e of the last pass: sum of (int64)(r * r * 2^20); rms = sqrt(e / 2^20 / points) */
} dh_fit_record;       /* 24 bytes */
typedef struct dh_fit_model dh_fit_model;
typedef struct dh_fitter dh_fitter;
/* Copies n points and their normals (x, y, z triples) to `device`.  DH_EINVAL: NULL arguments, n = 0 or above DH_FIT_MAX_POINTS,
 * a non-finite value, a normal whose squared length (in f64) lies outside [0.98, 1.02]. */
int dh_fit_model_create(const float *points, const float *normals, uint32_t n, int device, dh_fit_model **out);
int dh_fit_model_destroy(dh_fit_model *m);
/* each pointer nullable; radius = the largest |v| (f64) */
int dh_fit_model_info(const dh_fit_model *m, uint32_t *n, double *radius);
int dh_fit_params_default(dh_fit_params *p);
int dh_fitter_create(int device, dh_fitter **out);
int dh_fitter_destroy(dh_fitter *f);
/* frames [n][h][w] u16; out [n_instances] and records [n_instances] */
int dh_fit_depth(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *const *models,
                 uint32_t n_models, const dh_render_instance *instances, uint32_t n_instances, const dh_fit_params *params,
                 dh_render_instance *out, dh_fit_record *records);
/* frame i is seen through camera i of the table, which must hold exactly n cameras */
int dh_fit_depth_cameras(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                         const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances,
                         uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records);
int dh_fit_depth_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9],
                        const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances,
                        uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records,
                        void *stream);
int dh_fit_depth_cameras_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances,
                                uint32_t n_instances, const dh_fit_params *params, dh_render_instance *out, dh_fit_record *records,
                                void *stream);

/* ---- carrying each camera's fitted pose across steps ----
 * Detect once, follow with the model, fall back to the detector when the model loses the head: a dh_fit_tracker holds, per camera
 * of a camera table, the last fitted instance, and each step fits every present camera's model to its frame from that instance
 * (a short schedule without coarse steps) or, where there is none, from the forest's pose, and decides whether the fit is to be
 * believed.  One head per camera.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  f32 and f64
 * expressions are evaluated left to right, every operation rounded on its own; only + - * /, compares and casts run on the
 * device.  tests/fit_track_ref.py restates it; the GPU equals it byte for byte.
 * STATE of camera c (dh_fit_track_state): R[9], t[3] of the last accepted instance (f32, exactly as the fit wrote them), t_prev[3]
 *   the accepted t before that, tracked and have_prev (0 or 1), age (consecutive accepted steps) and lost (consecutive steps
 *   without an accepted fit), both saturating at 2^32 - 1.  Created and reset to all zeros.
 * ONE STEP of camera c from its depth frame, the forest's dh_pose and dh_support of that frame, and present[c] (NULL: all present):
 * 0. ABSENT (present[c] == 0): R, t and t_prev stay; lost = lost + 1; have_prev = 0; when lost > max_coast: tracked = 0, age = 0.
 *    The record: status DH_FIT_TRACK_ABSENT, instance and fit record zeros.  Nothing below runs.
 * 1. DETECTION.  valid = total_mass > 0  and  mass * conf_den >= total_mass * conf_num (the exact 96-bit products)  and
 *    windows >= min_windows.
 * 2. START.  tracked: R = the state's R; t = the state's t, or with DH_FIT_TRACK_MOTION in the tracker's flags and have_prev,
 *    t[j] = t[j] + (t[j] - t_prev[j]) in f32.  Schedule (0, iterations_tracked).
 *    Else when valid: t = mid_point; for j = 0, 1, 2:  x = rotation[j] / 3.14159 * 60.0 + 60.5 (f64);  ri_j = 0 unless x >= 0.0 (NaN
 *    too), 119 when x >= 119.0, else (int)x.  (c_j, s_j) = entry ri_j of the ANGLE TABLE: 120 pairs (cos a_i, sin a_i) of
 *    a_i = (double)(i - 60) / 60.0 * 3.14159, computed once on the host by the C library's cos and sin and returned by
 *    dh_fit_tracker_angles; no cosine or sine is evaluated anywhere else.  With, in f64 and row-major,
 *      Z = [c0, s0, 0; -s0, c0, 0; 0, 0, 1]   (Rz(-a0): the sine negated, not evaluated again)
 *      Y = [c1, 0, s1; 0, 1, 0; -s1, 0, c1]   X = [1, 0, 0; 0, c2, -s2; 0, s2, c2]
 *    first M = Y Z, then R = X M, every element of a product as (A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] with the
 *    zeros and ones taking part as 0.0 and 1.0; R is rounded to f32 once: Rx(a2) Ry(a1) Rz(-a0), the convention of
 *    render.euler_to_matrix.  Schedule (coarse_iterations, iterations) of the step's dh_fit_params.
 *    Else there is NO START: lost = lost + 1, tracked = have_prev = age = 0, R, t, t_prev stay; the record: status
 *    DH_FIT_TRACK_NONE, instance and fit record zeros; no fit work is done for the camera.
 *    The start instance: frame c, mesh 0, R, t, the tracker's scale, flags 0.
 * 3. FIT.  The rule of the section above, unchanged, on the start instance with the camera's K, the step's dh_fit_params (gates,
 *    lambda, min_points) and the start's own schedule.
 * 4. ACCEPTANCE.  Reason bits, the fit being accepted when none is set:
 *    DH_FIT_TRACK_BAD_STATUS  status != DH_FIT_OK;      DH_FIT_TRACK_BAD_POINTS  points < keep_points;
 *    DH_FIT_TRACK_BAD_RMS     sum_r2_fixed > (int64)(rms_max * rms_max * 1048576.0) * (int64)points   (the cast made once, on the host);
 *    DH_FIT_TRACK_BAD_JUMP    the detection is valid and not ((dx * dx + dy * dy) + dz * dz <= max_jump * max_jump) with
 *                             d = (double)t_fit - (double)mid_point, in f64 (a NaN rejects).
 * 5. OUTCOME.  Accepted: t_prev = t; R, t = the fitted instance's; have_prev = the old tracked; tracked = 1; age = age + 1; lost = 0;
 *    status DH_FIT_TRACK_CARRIED when the start was the carried one, else DH_FIT_TRACK_FITTED.  Not accepted: R, t, t_prev stay;
 *    tracked = have_prev = age = 0; lost = lost + 1; status DH_FIT_TRACK_REJECTED | the reason bits; the next step starts from
 *    the forest.
 * 6. OUTPUT.  One dh_fit_track_record per camera: the fitted instance when accepted, else the start instance; the fit's record;
 *    the status; age and lost after the step.
 * dh_fit_tracker_create: the camera table and the model must outlive the tracker and live on one device.  Every device buffer
 * is allocated there (the host forms' frame staging at the first host step, for its frame size): a _device step allocates nothing,
 * launches k_fit_track_seed, the per-instance-schedule instance of k_fit and k_fit_track_update on `stream` and never waits on the
 * host.  Steps of one tracker must be stream-ordered.  step_poses takes the forest's poses and support (host memory; _device:
 * device memory); step first runs dh_predict_batch_cameras_support_device without guesses on the same stream and also returns
 * its poses and support.  records [n_cams].  DH_EINVAL before anything is launched, with the outputs untouched:
 * create: NULL cameras / model / out; unknown flags; a scale that is not finite or with |scale| * (the model's largest |v|) above
 *   DH_FIT_MAX_EXTENT; a model on another device than the table; iterations_tracked above 64; rms_max or max_jump outside
 *   (0, 4096] (NaN included); conf_den 0 or conf_num > conf_den; a reserved word that is not 0.
 * step: NULL tracker / frames / poses / support / records (and predictor for the whole step); w or h outside 1 .. DH_RENDER_MAX_SIZE;
 *   the fit's own refusals of dh_fit_params; for the whole step the predictor's own refusals (a radius above 2^31 - 1, another
 *   device).  reset: NULL tracker, a camera outside -1 .. n - 1.  state, angles, params_default: NULL argument. */
#define DH_FIT_TRACK_MOTION 1u          /* flags of dh_fit_tracker_create: constant-velocity start */
#define DH_FIT_TRACK_NONE 0u            /* dh_fit_track_record.status, low byte */
#define DH_FIT_TRACK_FITTED 1u
#define DH_FIT_TRACK_CARRIED 2u
#define DH_FIT_TRACK_REJECTED 3u
#define DH_FIT_TRACK_ABSENT 4u
#define DH_FIT_TRACK_BAD_STATUS 0x100u  /* reason bits, with DH_FIT_TRACK_REJECTED */
#define DH_FIT_TRACK_BAD_POINTS 0x200u
#define DH_FIT_TRACK_BAD_RMS 0x400u
#define DH_FIT_TRACK_BAD_JUMP 0x800u
#define DH_FIT_TRACK_ANGLES 120
typedef struct dh_fit_track_params {
    uint32_t iterations_tracked;  /* 6: full steps of a carried start, at most 64 */
    uint32_t keep_points;         /* 30 */
    double   rms_max;             /* 5.0 (mm), in (0, 4096] */
    double   max_jump;            /* 150.0 (mm), in (0, 4096] */
    uint32_t conf_num, conf_den;  /* 1 / 50: DESIGN.md section 13's confidence of a detected head at the default radius */
    uint32_t min_windows;         /* 1 */
    uint32_t max_coast;           /* 3 absent steps */
    uint64_t reserved[2];         /* 0 */
} dh_fit_track_params;  /* 56 bytes */
typedef struct dh_fit_track_state {
    float    R[9], t[3], t_prev[3];
    uint32_t tracked, have_prev, age, lost;
} dh_fit_track_state;   /* 76 bytes, no padding */
typedef struct dh_fit_track_record {
    dh_render_instance instance;
    dh_fit_record      fit;
    uint32_t status;              /* DH_FIT_TRACK_*: kind in the low byte, reason bits above it */
    uint32_t age, lost;
    uint32_t reserved;            /* 0 */
} dh_fit_track_record;  /* 104 bytes, no padding */
typedef struct dh_fit_tracker dh_fit_tracker;
int dh_fit_track_params_default(dh_fit_track_params *p);
/* the angle table (no tracker needed) */
int dh_fit_tracker_angles(double out[DH_FIT_TRACK_ANGLES][2]);
/* params NULL selects dh_fit_track_params_default */
int dh_fit_tracker_create(const dh_cameras *c, const dh_fit_model *m, float scale, uint32_t flags, const dh_fit_track_params *params,
                          dh_fit_tracker **out);
int dh_fit_tracker_destroy(dh_fit_tracker *t);
/* camera, or -1 for all, back to zeros; ordered on `stream` */
int dh_fit_tracker_reset(dh_fit_tracker *t, int camera, void *stream);
/* states [n_cams]; synchronises the device */
int dh_fit_tracker_state(dh_fit_tracker *t, dh_fit_track_state *states);
int dh_fit_tracker_step_poses(dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, const dh_pose *poses,
                              const dh_support *support, const dh_fit_params *fit_params, dh_fit_track_record *records);
int dh_fit_tracker_step_poses_device(dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                     const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params,
                                     dh_fit_track_record *records, void *stream);
int dh_fit_tracker_step(dh_predictor *p, dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, uint32_t radius,
                        const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out, dh_fit_track_record *records);
int dh_fit_tracker_step_device(dh_predictor *p, dh_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                               uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out,
                               dh_fit_track_record *records, void *stream);

/* ---- adapting a model's shape to a subject ----
 * The fit above moves a rigid model; no subject has the generic head.  A dh_fit_basis adds a linear shape space to a model and one
 * SHAPE STEP solves, per subject, for the increment of the shape coefficients that brings the model onto the frames it was already
 * fitted to: one Gauss-Newton step over all fitted instances of the subject.  Not in the reference: PARITY UNPINNED, the
 * definition below is this library's.  The arithmetic conventions are the fit's: f64, evaluated left to right, every product, sum
 * and quotient rounded on its own, + - * /, compares and casts only, no library function on the device.
 * BASIS: K displacement fields, 1 <= K <= DH_SHAPE_MAX_FIELDS, each n f32 triples B_k[i] in mm, for a model of n points; immutable,
 *   on one device.  Deforming a model is the caller's step on the host: v_i + sum_k c_k B_k[i] in f64, rounded to f32 once, the
 *   normals recomputed from the deformed mesh (fit.deform, fit.vertex_normals).  The device never evaluates coefficients: it solves
 *   for an increment at the model it is given.
 * ONE SHAPE STEP takes frames, one K or a camera table, ONE model and its basis, n_instances fitted instances (what dh_fit_depth*
 *   wrote; `mesh` and `flags` are ignored), subjects[n_instances] (NULL: every instance belongs to subject 0; DH_SHAPE_SKIP: the
 *   instance takes no part) and n_subjects <= DH_SHAPE_MAX_SUBJECTS.  For every instance that takes part and every point i of the
 *   model, p, nrm, c, the five skip tests, the pixel, d and the residual r are those of ONE PASS of the section above at the
 *   instance's (R, t), scale and frame, with gate g = params.gate.  For a point that passed, per field k < K:
 *     sb = B_k[i] * scale;  w[j] = (R[j][0] * sb0 + R[j][1] * sb1) + R[j][2] * sb2;  J_k = (nrm0 * w0 + nrm1 * w1) + nrm2 * w2
 *   and, into the sums of the instance's subject, with S = 2^20 and truncating casts (so their order is free):
 *     A_kl += (int64)((J_k * J_l) * S) for k <= l,  b_k += (int64)((J_k * r) * S),  e += (int64)((r * r) * S),  count += 1;
 *   used += 1 for every instance that passed at least one point.  Magnitudes: the gate lies in (0, DH_SHAPE_MAX_GATE] and
 *   |scale| * (the basis's largest |B_k[i]|) <= DH_SHAPE_MAX_FIELD, so with the fit's |R x| <= 1.03 |x| and |nrm| <= 1.05,
 *   |J_k| <= 1.05 * 1.03 * 256 < 2^9 and, while |p| <= 2 p.z, |r| <= 1.05 * 2 * 256 < 2^10: every product stays below 2^19;
 *   times 2^20, a subject may sum 2^23 point-instances below 2^62.  A K that lets points through at a wider angle is not refused,
 *   but there the sums can leave int64 and the result is unspecified (arithmetic only: nothing faults), and no longer pinned to the
 *   restatement, whose Python ints do not wrap.
 * SOLVE, per subject: count < min_points gives DH_SHAPE_FEW_POINTS and a zero increment (a subject without an instance: points 0).
 *   Else A_kl = (double)sum / S (A symmetric), b_k alike; A_kk = A_kk * (1.0 + lambda) + 1e-9; A delta = b is solved on the K x K
 *   block by the Gaussian elimination without pivoting and the back substitution of ONE STEP of the section above (n = K), in
 *   that operation order.  A pivot that is not > 0.0 (NaN included) gives DH_SHAPE_SINGULAR and a zero increment.
 * One dh_shape_record per subject: delta[k] for k < K and zeros beyond; points = count; instances = used; status; sum_r2_fixed = e,
 *   the residual BEFORE the step (rms = sqrt(e / 2^20 / points)).  Bit-identical run to run and to tests/shape_ref.py.
 * The calls run on a dh_fitter, which owns the sums buffer and (for the host calls) the staging, taken at the first shape call
 * and growing on demand; the shape calls of one fitter must be stream-ordered with one another.  The host calls take host frames,
 * instances, subjects and records and are synchronous.  The _device calls take device frames, instances, subjects and records,
 * enqueue exactly three stream-ordered operations on `stream` (NULL = default stream) -- k_shape_clear (the subjects' sums back to zero),
 * k_shape_accumulate, k_shape_solve -- and never wait on the host: they chain after dh_fit_depth*_device.  K and params are host memory in every call;
 * params NULL selects dh_shape_params_default.
 * DH_EINVAL before anything is launched, with the outputs untouched: NULL fitter / frames / records / model / basis; n < 1 or above
 * 65535; w or h outside 1 .. DH_RENDER_MAX_SIZE; NULL K, or a NULL camera table, one of another device or one whose length is not
 * n; n_subjects outside 1 .. DH_SHAPE_MAX_SUBJECTS; a gate outside (0, DH_SHAPE_MAX_GATE] (NaN included); lambda not >= 0 or not
 * finite; min_points 0; a reserved word that is not 0; a model or basis of another device than the fitter; a basis whose n is not
 * the model's; instances NULL with n_instances > 0; n_instances above 2^23.  The host calls also refuse, per instance that takes
 * part: a frame >= n; a subject >= n_subjects that is not DH_SHAPE_SKIP; a non-finite R, t or scale; an R outside
 * DH_FIT_R_TOLERANCE; |scale| * (the model's largest |v|) above DH_FIT_MAX_EXTENT; |scale| * (the basis's largest |B_k[i]|) above
 * DH_SHAPE_MAX_FIELD; and a subject whose instances times n exceed DH_SHAPE_MAX_TERMS.  The _device calls cannot read the
 * instances: they refuse n_instances * n above DH_SHAPE_MAX_TERMS, and the device skips (as DH_SHAPE_SKIP) every instance one of
 * the per-instance refusals names, a NaN failing each test, so no input leads out of a buffer or out of the magnitude bound.
 * n_instances = 0 is no error: every record is DH_SHAPE_FEW_POINTS with points 0. */
#define DH_SHAPE_OK 0u
#define DH_SHAPE_FEW_POINTS 1u         /* the subject's instances associated fewer than min_points points */
#define DH_SHAPE_SINGULAR 2u           /* a pivot of the normal equations was not > 0 */
#define DH_SHAPE_MAX_FIELDS 8u         /* fields of a basis */
#define DH_SHAPE_MAX_SUBJECTS 256u     /* subjects of a call */
#define DH_SHAPE_SKIP 0xFFFFFFFFu      /* subjects[i]: instance i takes no part */
#define DH_SHAPE_MAX_FIELD 256.0       /* mm: |scale| * largest |B_k[i]| */
#define DH_SHAPE_MAX_GATE 256.0        /* mm */
#define DH_SHAPE_MAX_TERMS 8388608u    /* 2^23: points times instances of one subject */
typedef struct dh_shape_params {
    double   gate;                /* 25 (mm), in (0, DH_SHAPE_MAX_GATE] */
    double   lambda;              /* 1e-3: relative damping of the diagonal, >= 0 */
    uint32_t min_points;          /* 64, at least 1 */
    uint32_t reserved0;           /* 0 */
    uint64_t reserved[2];         /* 0 */
} dh_shape_params;     /* 40 bytes */
typedef struct dh_shape_record {
    double   delta[8];            /* the increment of coefficient k; 0 for k >= K and when status is not DH_SHAPE_OK */
    uint32_t points;              /* count */
    uint32_t instances;           /* used (dh_fit_shape_views*: the (instance, view) pairs that passed a point) */
    uint32_t status;              /* DH_SHAPE_* */
    uint32_t reserved;            /* 0 */
    int64_t  sum_r2_fixed;        /* e: the residual before the step */
} dh_shape_record;     /* 88 bytes, no padding */
typedef struct dh_fit_basis dh_fit_basis;
/* Copies n_fields fields of n triples each (fields[k][i][3], mm) to `device`.  DH_EINVAL: NULL arguments, n = 0 or above
 * DH_FIT_MAX_POINTS, n_fields outside 1 .. DH_SHAPE_MAX_FIELDS, a non-finite value. */
int dh_fit_basis_create(const float *fields, uint32_t n, uint32_t n_fields, int device, dh_fit_basis **out);
int dh_fit_basis_destroy(dh_fit_basis *b);
/* each pointer nullable; largest = the largest |B_k[i]| (f64) */
int dh_fit_basis_info(const dh_fit_basis *b, uint32_t *n, uint32_t *n_fields, double *largest);
int dh_shape_params_default(dh_shape_params *p);
/* frames [n][h][w] u16; instances [n_instances]; subjects [n_instances] or NULL; records [n_subjects] */
int dh_fit_shape(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model,
                 const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects,
                 uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records);
/* frame i is seen through camera i of the table, which must hold exactly n cameras */
int dh_fit_shape_cameras(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c, const dh_fit_model *model,
                         const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances,
                         const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records);
int dh_fit_shape_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_model *model,
                        const dh_fit_basis *basis, const dh_render_instance *instances, uint32_t n_instances,
                        const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params, dh_shape_record *records,
                        void *stream);
int dh_fit_shape_cameras_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                const dh_fit_model *model, const dh_fit_basis *basis, const dh_render_instance *instances,
                                uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects, const dh_shape_params *params,
                                dh_shape_record *records, void *stream);

/* ---- fitting one model to several views ----
 * The fit of section 18 sees a head through one camera; a rig exists so that cameras at different angles constrain one another.
 * Here ONE pose in the WORLD frame is fitted per instance against the frames of every camera that sees it: one normal-equation
 * system summed over all its (view, point) pairs.  Not in the reference: PARITY UNPINNED, the definition below is this library's.
 * The arithmetic conventions are the fit's: f64, evaluated left to right, every product, sum and quotient rounded on its own (no
 * contraction), + - * /, compares and casts only, no library function on the device.
 * VIEW TABLE: a dh_fit_views is bound to a dh_cameras table of n cameras (which must outlive it) and lives on that table's device,
 *   immutable.  For each camera c it holds the WORLD-TO-CAMERA transform V_c (f32[9], row-major) and u_c (f32[3], mm), widened to
 *   f64 on the device: the camera-space point of a world point x is V_c x + u_c.  This is the inverse direction of dh_rig_create's
 *   extrinsics (camera to world: x = R_c p + t_c), on purpose: the device never inverts a matrix; V_c = R_c^T, u_c = -(R_c^T t_c)
 *   is the caller's step on the host (fit.views_from_rig: in f64, rounded to f32 once).
 * INSTANCE: a dh_view_instance.  `model` is the model index; bit k of `views` means camera first_cam + k sees the instance (the
 *   layout of dh_rig_person.views with the rig's first camera); R, t are the model's pose in the WORLD frame and widen to f64 with
 *   scale; `flags` is ignored.  Frame c of the call is camera c's frame, as in dh_fit_depth_cameras.
 * ONE PASS at the world pose (R_w, t_w) with gate g.  For every set bit k of `views`, ascending, with c = first_cam + k, V = V_c,
 *   u = u_c, the COMPOSITE camera pose of the view is formed once:
 *     R_v[i][j] = (V[i][0] * R_w[0][j] + V[i][1] * R_w[1][j]) + V[i][2] * R_w[2][j]
 *     t_v[i]    = ((V[i][0] * t_w0 + V[i][1] * t_w1) + V[i][2] * t_w2) + u[i]
 *   and every point i of the model runs ONE PASS of section 18 UNCHANGED at (scale, R_v, t_v), camera c's K and frame c: sv, p,
 *   nrm, the skip tests (p.z >= 1.0, c < 0.0, the pixel inside the frame, d != 0, |d - p.z| <= g) and the residual
 *   r = c * (d / p.z - 1.0).  For a point that passed:
 *     q = p - t_v;   m = (q1 * nrm2 - q2 * nrm1,  q2 * nrm0 - q0 * nrm2,  q0 * nrm1 - q1 * nrm0)       (as the fit forms it)
 *     J = (V^T nrm, V^T m)   with   (V^T a)[j] = (V[0][j] * a0 + V[1][j] * a1) + V[2][j] * a2          (the WORLD row)
 *   and the fit's 29 int64 sums with S = 2^20 and truncating casts (so their order is free), taken over ALL (view, point) pairs
 *   of the instance:  A_ab += (int64)((J_a * J_b) * S) for a <= b,  b_a += (int64)((J_a * r) * S),  e += (int64)((r * r) * S),
 *   count += 1.  views_used is the mask of the bits k in whose view at least one point passed.
 *   For an orthonormal V, J is the derivative of the residual with respect to a translation of the model in the world frame
 *   (J_0..2) and a rotation of the model about its own origin with a world-frame axis (J_3..5): moving the model by dt in the world
 *   moves it by V dt in the camera, (V dt) . nrm = dt . (V^T nrm); turning it by w turns it by V w in the camera, (V w) . m =
 *   w . (V^T m).  With one view, V = I and u = 0, R_v = R_w, t_v = t_w and J = (nrm, m) (products with 0.0 and 1.0 are exact), so
 *   every sum and every output equals the single-view fit's bit for bit.
 *   Magnitudes: V is held to |V V^T - I| <= DH_FIT_VIEW_TOLERANCE per element and R_w to DH_FIT_R_TOLERANCE, so |R_v x| <= 1.032 |x|
 *   (the fit's 1.03 is the one constant that changes); |nrm| <= 1.05 and |J_a| <= 1.09 * 4096 hold as they stand, |r| <= 1.05 *
 *   (|p| / p.z) * g per camera.  While no camera sees a point further than 60 degrees off its axis every product stays below 2^27;
 *   times 2^20, times at most DH_FIT_MAX_POINTS (view, point) terms of an instance: below 2^62.  Outside that the words of the
 *   section above hold (unspecified, nothing faults).  The derivation stands in depthhead_amd/csrc/dh_fit.h.
 * ONE STEP and the SCHEDULE are section 18's, applied to the world pose: count (over all views) < min_points ends the fit with
 *   DH_FIT_FEW_POINTS; the damped system is solved on the leading 3 x 3 block in a coarse step (only J_0..2 matter), else 6 x 6, a
 *   pivot that is not > 0.0 ends the fit with DH_FIT_SINGULAR; t_w[j] = t_w[j] + x[j], and in a full step R_w = C R_w with the
 *   Cayley rotation C of x[3..5]; coarse_iterations coarse steps at gate[0], then `iterations` full steps at gate[1], both early
 *   exits (every |x_a| < 1e-6), and one last pass at gate[1] at the final pose -- also after DH_FIT_FEW_POINTS and
 *   DH_FIT_SINGULAR -- that gives the record's points, sum_r2_fixed and views_used; steps counts the steps that were applied.  The
 *   output instance is the input's with R and t rounded to f32 once and everything else copied through.  dh_fit_params is taken
 *   as it is.  Bit-identical run to run and to tests/view_fit_ref.py.
 * The calls run on a dh_fitter, which owns the call's tables and (for the host call) the frame and output staging and allocates
 *   nothing after the first such call of a given size.  models, instances and params are host memory in both forms; params NULL
 *   selects dh_fit_params_default.  dh_fit_depth_views takes host frames [n][h][w] (n = the table's cameras) and host outputs and
 *   is synchronous.  dh_fit_depth_views_device takes device frames and device outputs, enqueues on `stream` (NULL = default
 *   stream) the upload of the call's tables and ONE kernel launch in which every pass and step of every instance runs, and
 *   never waits on the host for anything the device computes; it chains after dh_render_depth_cameras_device.  On a stream
 *   that is being captured the kernel alone is enqueued and the runtime is asked for nothing else: the tables must be those the
 *   fitter's last call uploaded -- the same call made once before the capture, and complete -- else DH_ESTATE.  A replay fits the
 *   captured instances to the frames' current content, and is valid until the fitter's next call, which reuses the tables.
 * DH_EINVAL before anything is launched, with the outputs untouched: NULL fitter / frames / out / records; a NULL view table or
 *   one of another device than the fitter; w or h outside 1 .. DH_RENDER_MAX_SIZE; the refusals of dh_fit_params of section 18;
 *   instances or models NULL with n_instances > 0; and per instance, in this order: views == 0; a set bit naming a camera >= n; a
 *   model >= n_models; a non-finite R, t or scale; an R outside DH_FIT_R_TOLERANCE; a NULL model or one of another device; |scale| *
 *   (the model's largest |v|) above DH_FIT_MAX_EXTENT; popcount(views) * (the model's points) above DH_FIT_MAX_POINTS (8 views of a
 *   4096-point model pass).  n_instances = 0 is no error and writes nothing. */
#define DH_FIT_VIEW_TOLERANCE 0.001   /* largest |(V V^T - I)[i][j]| of a view (a rotation rounded to f32 is within 1e-6) */
typedef struct dh_view_instance {
    uint32_t first_cam;           /* the camera of bit 0 of `views` */
    uint32_t model;               /* index into the call's models */
    uint64_t views;               /* bit k: camera first_cam + k sees the instance */
    float    R[9], t[3];          /* the model's pose in the world frame (row-major R; mm) */
    float    scale;
    uint32_t flags;               /* ignored, copied through */
} dh_view_instance;    /* 72 bytes, no padding */
typedef struct dh_view_fit_record {
    uint32_t points;              /* (view, point) pairs associated by the last pass */
    uint32_t steps;               /* steps applied */
    uint32_t status;              /* DH_FIT_* */
    uint32_t reserved;            /* 0 */
    int64_t  sum_r2_fixed;        /* e of the last pass */
    uint64_t views_used;          /* bit k: the last pass associated at least one point in the view of camera first_cam + k */
} dh_view_fit_record;  /* 32 bytes, no padding */
typedef struct dh_fit_views dh_fit_views;
/* V [n][9] and u [n][3] for the n cameras of `c`, copied to c's device.  DH_EINVAL: NULL arguments, a non-finite entry, a V with
 * an element of V V^T (in f64, formed as R R^T is in section 18) further than DH_FIT_VIEW_TOLERANCE from the identity's. */
int dh_fit_views_create(const dh_cameras *c, const float *V, const float *u, dh_fit_views **out);
int dh_fit_views_destroy(dh_fit_views *v);
/* each pointer nullable: the number of cameras and the device */
int dh_fit_views_info(const dh_fit_views *v, int *n, int *device);
/* frames [n][h][w] u16 with n the view table's cameras; out [n_instances] and records [n_instances] */
int dh_fit_depth_views(dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views,
                       const dh_fit_model *const *models, uint32_t n_models, const dh_view_instance *instances,
                       uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out, dh_view_fit_record *records);
int dh_fit_depth_views_device(dh_fitter *f, const uint16_t *frames, int w, int h, const dh_fit_views *views,
                              const dh_fit_model *const *models, uint32_t n_models, const dh_view_instance *instances,
                              uint32_t n_instances, const dh_fit_params *params, dh_view_instance *out,
                              dh_view_fit_record *records, void *stream);

/* ---- adapting a model's shape across views ----
 * The shape step of section 20 knows one camera and a camera-frame pose per instance; the multi-view fit of section 21 writes ONE
 * world pose per instance and the mask of the cameras that see it.  A MULTI-VIEW SHAPE STEP takes those instances as they are and
 * sums, per subject, section 20's normal equations over every (instance, view, point): a shape coefficient is a scalar, the same
 * in every frame, so a view contributes its terms with the composite camera pose of section 21 in place of (R, t) and nothing
 * else changes.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  The arithmetic conventions are
 * the fit's: f64, evaluated left to right, every product, sum and quotient rounded on its own, + - * /, compares and casts only.
 * ONE MULTI-VIEW SHAPE STEP takes frames [n_sets][n][h][w] u16, where n is the view table's cameras and a SET is one moment of
 *   the rig: frame s * n + c is camera c at set s; a dh_fit_views table (and through it the camera table); ONE model and its
 *   basis; n_instances dh_view_instance (what dh_fit_depth_views* wrote; `model` and `flags` are ignored, as section 20 ignores
 *   `mesh`); sets[n_instances] (NULL: every instance is in set 0); subjects[n_instances] (NULL: subject 0; DH_SHAPE_SKIP: the
 *   instance takes no part); n_subjects and dh_shape_params.  For every instance that takes part and every set bit k of `views`,
 *   with c = first_cam + k, V = V_c, u = u_c:
 *     the composite (R_v, t_v) is formed once, exactly as section 21 writes it (R_v = V R_w, t_v = V t_w + u, in its element
 *     order); every point of the model runs ONE PASS of section 18 unchanged at (scale, R_v, t_v), camera c's K, frame
 *     sets[i] * n + c and gate g = params.gate; and a point that passed adds section 20's terms with R_v for R, in section 20's
 *     operation order (sb, w, J_k), into its subject's sums: A_kl, b_k, e, count, with S = 2^20 and truncating casts.
 *   used += 1 for every (instance, view) PAIR that passed at least one point: THE RECORD'S `instances` FIELD COUNTS PAIRS HERE,
 *   not instances (with one view per instance it is section 20's count).
 *   Magnitudes: with section 21's |R_v x| <= 1.032 |x|, |J_k| <= 1.05 * 1.032 * 256 < 2^9 and section 20's product bounds stand;
 *   DH_SHAPE_MAX_TERMS = 2^23 counts the (view, point) pairs of a subject.  Outside |p| <= 2 p.z the words of section 20 hold.
 * SOLVE, the statuses and dh_shape_record are section 20's, unchanged.  With one view, V = I, u = 0 and n_sets = 1 every sum and
 *   every record byte equals dh_fit_shape_cameras on the same pose.  Bit-identical run to run and to tests/shape_views_ref.py.
 * The calls run on a dh_fitter and reuse its sums buffer, so ALL shape calls of one fitter, of this section and of section 20, must
 * be stream-ordered with one another.  dh_fit_shape_views takes host frames, instances, sets, subjects and records and is
 * synchronous.  dh_fit_shape_views_device takes device frames, instances, sets, subjects and records, enqueues exactly three
 * kernels on `stream` (NULL = default stream) -- k_shape_clear, k_shape_accumulate_views (one workgroup per (instance, view) pair),
 * k_shape_solve -- allocates nothing after the fitter's first shape call and never waits on the host: it chains after
 * dh_fit_depth_views_device, whose `out` is its `instances`.  params is host memory in both; NULL selects dh_shape_params_default.
 * DH_EINVAL before anything is launched, with the outputs untouched: section 20's refusals for the fitter, frames, records, model,
 * basis, params, n_subjects, w and h and the instance count; a NULL view table or one of another device than the fitter; n_sets of
 * 0, or n_sets * n above 65535.  The host call also refuses, per instance that takes part (its subject is not DH_SHAPE_SKIP), in
 * this order: views == 0; a set bit naming a camera >= n; a set >= n_sets; a subject >= n_subjects; what section 20 refuses of R,
 * t and scale, the field limit included; and a subject whose (instance, view) pairs times the model's points exceed
 * DH_SHAPE_MAX_TERMS.  The _device call cannot read the instances: it refuses n_instances * min(64, n) * (the model's points)
 * above DH_SHAPE_MAX_TERMS, and the device skips, AS A WHOLE, every instance one of the per-instance refusals names, a NaN failing
 * each test, so no input leads out of a buffer or out of the magnitude bound.  n_instances = 0 is no error: every record is
 * DH_SHAPE_FEW_POINTS with points 0. */
/* frames [n_sets][n][h][w] u16 with n the view table's cameras; instances, sets (or NULL) and subjects (or NULL) [n_instances];
 * records [n_subjects] */
int dh_fit_shape_views(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                       const dh_fit_model *model, const dh_fit_basis *basis, const dh_view_instance *instances,
                       uint32_t n_instances, const uint32_t *sets, const uint32_t *subjects, uint32_t n_subjects,
                       const dh_shape_params *params, dh_shape_record *records);
int dh_fit_shape_views_device(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                              const dh_fit_model *model, const dh_fit_basis *basis, const dh_view_instance *instances,
                              uint32_t n_instances, const uint32_t *sets, const uint32_t *subjects, uint32_t n_subjects,
                              const dh_shape_params *params, dh_shape_record *records, void *stream);

/* ---- calibrating a view table ----
 * Every multi-view section above takes the view table on faith.  A CALIBRATION STEP reads the same residual once more with the
 * fitted world poses and the model HELD and each camera MOVED: one Gauss-Newton step per camera over all the (instance, point)
 * pairs that camera sees, for a small rigid motion of the camera.  Not in the reference: PARITY UNPINNED, the definition below is
 * this library's.  The arithmetic conventions are the fit's: f64, evaluated left to right, every product, sum and quotient
 * rounded on its own (no contraction), + - * /, compares and casts only, no library function on the device.
 * ONE CALIBRATION STEP takes frames [n_sets][n][h][w] u16 (section 23's layout: frame s * n + c is camera c at set s), a
 *   dh_fit_views table of n cameras, ONE model, n_instances dh_view_instance (what dh_fit_depth_views* wrote; `model` and `flags`
 *   are ignored), sets[n_instances] (NULL: set 0), take[n_instances] (NULL: all take part; DH_CALIB_SKIP: the instance takes no
 *   part; any other value: it does), hold[n] bytes (NULL: none; non-zero: camera c is HELD, a gauge camera that gets no update)
 *   and dh_calib_params.  It writes one dh_calib_record per CAMERA.
 * PIVOT: params.pivot is one world point o (mm).  Camera c's pivot is its image, formed as section 21 forms t_v:
 *     g_c[i] = ((V[i][0] * o0 + V[i][1] * o1) + V[i][2] * o2) + u[i]
 *   The camera is turned about g_c, not about its own origin: with o among the heads a rotation moves the model points little,
 *   so rotation and translation decouple and the lever arms stay short (Magnitudes).
 * ACCUMULATION, for every instance that takes part and every set bit k of `views` with c = first_cam + k not held: the
 *   composite (R_v, t_v) is formed exactly as section 21 writes it.  The pair takes no part unless |t_v[i] - g_c[i]| <=
 *   DH_CALIB_MAX_ARM for i = 0, 1, 2 (a NaN fails).  Every point of the model runs ONE PASS of section 18 unchanged at (scale,
 *   R_v, t_v), camera c's K, frame sets[i] * n + c and gate g = params.gate.  A point that passed adds to CAMERA c's sums the
 *   fit's full row with the pivot in place of the translation:
 *     q = p - g_c;   m = (q1 * nrm2 - q2 * nrm1,  q2 * nrm0 - q0 * nrm2,  q0 * nrm1 - q1 * nrm0)
 *     J = (nrm0, nrm1, nrm2, m0 / DH_CALIB_ARM_UNIT, m1 / DH_CALIB_ARM_UNIT, m2 / DH_CALIB_ARM_UNIT)       (64: the division is exact)
 *   A_ab += (int64)((J_a * J_b) * S) for a <= b (21),  b_a += (int64)((J_a * r) * S) (6),  e += (int64)((r * r) * S),  count += 1,
 *   with S = 2^20 and truncating casts, so their order is free.  pairs += 1 for every (instance, view) pair that passed a point.
 *   Moving the camera by (d, w) about g_c moves a camera-space point p to C (p - g_c) + g_c + d: J is the derivative of the
 *   residual with respect to d and to 64 w.
 *   Magnitudes: |q| <= |p - t_v| + |t_v - g_c| <= 1.032 * 4096 + 2048 sqrt(3) < 7775, so |J_3..5| <= 1.05 * 7775 / 64 < 128 and
 *   |J_0..2| <= 1.05; the gate lies in (0, DH_SHAPE_MAX_GATE], so |r| < 538 while |p| <= 2 p.z: J J < 2^14, J r < 2^16.1,
 *   r r < 2^18.2, every product below section 20's 2^19; times 2^20, a camera may sum DH_SHAPE_MAX_TERMS = 2^23 (instance, point)
 *   terms below 2^62.  Outside |p| <= 2 p.z the words of section 18 hold (unspecified, nothing faults).
 * SOLVE, per camera: a held camera gets DH_CALIB_HELD.  Else count < min_points gives DH_CALIB_FEW_POINTS.  Else A_ab = (double)sum
 *   / S (A symmetric), b_a alike, A_aa = A_aa * (1.0 + lambda) + 1e-9, and A x = b is solved on the 6 x 6 block by section 18's
 *   elimination and back substitution; a pivot that is not > 0.0 gives DH_CALIB_SINGULAR.  Else d = x[0..2], w[j] = x[3 + j] /
 *   DH_CALIB_ARM_UNIT, C is section 18's Cayley rotation of w (a = w / 2.0 and the nine quotients written there), and
 *     V'[i][j] = (C[i][0] * V[0][j] + C[i][1] * V[1][j]) + C[i][2] * V[2][j]
 *     s = u - g_c;   u'[i] = (((C[i][0] * s0 + C[i][1] * s1) + C[i][2] * s2) + g_c[i]) + d[i]
 *   both rounded to f32 once.  If an element of V' V'^T (of the ROUNDED V', in f64, formed as R R^T is in section 18) is further
 *   than DH_FIT_VIEW_TOLERANCE from the identity's (NaN included) the status is DH_CALIB_NOT_ORTHONORMAL, else DH_CALIB_OK.
 * RECORD: V, u = the updated entry when the status is DH_CALIB_OK, otherwise the table's own entry bit for bit; points = count;
 *   pairs; status; sum_r2_fixed = e, the residual BEFORE the step; delta = (d, w), zeros unless DH_CALIB_OK.  The view table is
 *   immutable: the caller builds the next one on the host from the records (fit.views_from_records).  Bit-identical run to run
 *   and to tests/calib_ref.py.
 * The calls run on a dh_fitter, which owns the sums ([n] rows of 32 words, taken at the first call of a given table size) and,
 * for the host call, the staging; the calibration calls of one fitter must be stream-ordered with one another and with its
 * shape calls.  dh_fit_calibrate_views takes host frames, instances, sets, take, hold and records and is synchronous.
 * dh_fit_calibrate_views_device takes device pointers for those, enqueues exactly three kernels on `stream` (NULL = default
 * stream) -- k_calib_clear, k_calib_accumulate (one workgroup per (instance, view) pair), k_calib_solve -- and never waits on
 * the host: it chains after dh_fit_depth_views_device, whose `out` is its `instances`.  params is host memory in both forms;
 * NULL selects dh_calib_params_default.
 * DH_EINVAL before anything is launched, with the outputs untouched: NULL fitter / frames / records / model; a model of another
 * device than the fitter; a NULL view table or one of another device; n_sets of 0, or n_sets * n above 65535; w or h outside
 * 1 .. DH_RENDER_MAX_SIZE; a gate outside (0, DH_SHAPE_MAX_GATE] (NaN included); lambda not >= 0 or not finite; min_points 0; a
 * non-finite pivot; a reserved word that is not 0; instances NULL with n_instances > 0; n_instances above 2^23.  The host call
 * also refuses, per instance that takes part, in this order: views == 0; a set bit naming a camera >= n; a set >= n_sets; a
 * non-finite R, t or scale; an R outside DH_FIT_R_TOLERANCE; |scale| * (the model's largest |v|) above DH_FIT_MAX_EXTENT; and a
 * camera that is not held whose pairs times the model's points exceed DH_SHAPE_MAX_TERMS (every pair of an instance that takes
 * part counts here, one beyond the arm too: only the device forms t_v).  A pair beyond DH_CALIB_MAX_ARM is SKIPPED in both
 * forms, not refused (the caller cannot know it before the fit), and is not counted in the record's `pairs`.  The _device call cannot read
 * the instances: it refuses n_instances * (the model's points) above DH_SHAPE_MAX_TERMS, and the device skips, AS A WHOLE, every
 * instance one of the per-instance refusals names, a NaN failing each test, so no input leads out of a buffer or out of the
 * magnitude bound.  n_instances = 0 is no error: every camera that is not held reports DH_CALIB_FEW_POINTS. */
#define DH_CALIB_OK 0u
#define DH_CALIB_FEW_POINTS 1u         /* the camera's pairs associated fewer than min_points points */
#define DH_CALIB_SINGULAR 2u           /* a pivot of the normal equations was not > 0 */
#define DH_CALIB_NOT_ORTHONORMAL 3u    /* the updated V, rounded to f32, is outside DH_FIT_VIEW_TOLERANCE */
#define DH_CALIB_HELD 4u               /* hold[c] was set */
#define DH_CALIB_SKIP 0xFFFFFFFFu      /* take[i]: instance i takes no part */
#define DH_CALIB_ARM_UNIT 64.0         /* mm: the unit of the rotation columns (a power of two) */
#define DH_CALIB_MAX_ARM 2048.0        /* mm: largest |t_v[i] - g_c[i]| of a pair that takes part */
typedef struct dh_calib_params {
    double   gate;                /* 25 (mm), in (0, DH_SHAPE_MAX_GATE] */
    double   lambda;              /* 1e-3: relative damping of the diagonal, >= 0 */
    double   pivot[3];            /* 0, 0, 0 (mm): the world point o the cameras are turned about */
    uint32_t min_points;          /* 64, at least 1 */
    uint32_t reserved0;           /* 0 */
    uint64_t reserved[2];         /* 0 */
} dh_calib_params;     /* 64 bytes */
typedef struct dh_calib_record {
    float    V[9], u[3];          /* the updated entry when status is DH_CALIB_OK; otherwise the table's own, bit for bit */
    uint32_t points;              /* count */
    uint32_t pairs;               /* the (instance, view) pairs that passed a point */
    uint32_t status;              /* DH_CALIB_* */
    uint32_t reserved;            /* 0 */
    int64_t  sum_r2_fixed;        /* e: the residual before the step */
    double   delta[6];            /* d (mm) and w (radians to first order); 0 unless status is DH_CALIB_OK */
} dh_calib_record;     /* 120 bytes, no padding */
int dh_calib_params_default(dh_calib_params *p);
/* frames [n_sets][n][h][w] u16 with n the view table's cameras; instances, sets (or NULL) and take (or NULL) [n_instances];
 * hold (or NULL) [n] bytes; records [n] */
int dh_fit_calibrate_views(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                           const dh_fit_model *model, const dh_view_instance *instances, uint32_t n_instances,
                           const uint32_t *sets, const uint32_t *take, const uint8_t *hold, const dh_calib_params *params,
                           dh_calib_record *records);
int dh_fit_calibrate_views_device(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                                  const dh_fit_model *model, const dh_view_instance *instances, uint32_t n_instances,
                                  const uint32_t *sets, const uint32_t *take, const uint8_t *hold, const dh_calib_params *params,
                                  dh_calib_record *records, void *stream);

/* ---- carrying each rig person's fitted world pose across steps ----
 * The composition of the three sections above: every person of every rig keeps ONE fitted pose in the WORLD frame under the
 * rig-wide id the rig tracker (section 16) gave it.  Each step refits that pose against all the views that see the person,
 * from where it was and with a short schedule (section 19's idea, section 21's fit), and falls back to the rig tracker's person
 * record -- the forest's detection -- when the model loses the head.  A dh_rig_fit_tracker is bound to a rig table, a view table
 * of the SAME camera table and one model.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  f32
 * and f64 expressions are evaluated left to right, every operation rounded on its own; only + - * /, compares and casts run on
 * the device.  tests/rig_fit_track_ref.py restates it; the GPU equals it byte for byte.
 * The view table alone gives the rotation of a detected start (V_b^T below), so the device inverts nothing.  That the persons'
 * `world` came from a rig table CONSISTENT with the view table (V_c = R_c^T, u_c = -(R_c^T t_c): fit.views_from_rig) is the
 * caller's contract; the library checks only that both tables are bound to one dh_cameras handle.
 * STATE of rig g: DH_RIG_MAX_TRACKS entries (dh_rig_fit_state): id (0 = free; a free entry is all zeros), R[9], t[3] of the last
 *   accepted fit in the world frame (f32, exactly as the fit wrote them), t_prev[3] the accepted t before that, views_used of
 *   the last accepted fit, tracked and have_prev (0 or 1), age (consecutive accepted steps) and lost (consecutive steps without
 *   an accepted fit), both saturating at 2^32 - 1.  Created and reset to all zeros.
 * ONE STEP of rig g with cameras c0 = rig_begin[g] .. rig_begin[g + 1] - 1, from one frame per camera, present (NULL: all
 * present) and the outputs of a rig tracker step -- n_heads [n_cams], heads [n_cams][max_heads], n_persons [n_rigs], persons
 * [n_rigs][DH_RIG_MAX_PERSONS].  pm = the mask of the bits k with camera c0 + k present.
 * 0. pm == 0: the whole state of the rig is kept; every record of the rig is zero but for status = DH_FIT_TRACK_ABSENT.
 *    Nothing below runs.
 * 1. BIND.  The persons i < min(n_persons[g], DH_RIG_MAX_PERSONS) are walked in ascending i.  A person whose best_cam is no
 *    camera of the table or whose best_head >= min(n_heads[best_cam], max_heads) names no head and is ignored altogether.
 *    A person with id != 0 takes the lowest entry that holds its id, unless an earlier person of this step took that entry;
 *    when no entry holds the id it takes the lowest free entry, which becomes zeros with that id.  A person with id 0, one whose
 *    id an earlier person of the step bound, and one that finds no free entry is UNBOUND: it is fitted from its detection
 *    and reported, and nothing of it is carried.  An entry with id != 0 that no person took is UNSEEN; an unseen entry that is
 *    not tracked is freed (zeroed) here and has no record.  Then the unbound persons, in ascending i, each take the lowest
 *    RECORD SLOT s whose entry is free after all this; an unbound person for which none is left is dropped.  So a slot s of the
 *    rig is an entry (seen or unseen), an unbound person, or unused.
 * 2. START of a slot.
 *    CARRIED (an entry that is tracked): R = the state's R; t = the state's t, or with DH_FIT_TRACK_MOTION in the tracker's flags
 *      and have_prev, t[j] = t[j] + (t[j] - t_prev[j]) in f32; views = (views_used | the person's views when seen) & pm; schedule
 *      (0, iterations_tracked).  When that mask is empty the entry COASTS instead: lost = lost + 1, have_prev = 0, and when
 *      lost > max_coast the entry is freed (zeroed); its record: id, status DH_FIT_TRACK_ABSENT, age and lost (as they were
 *      before the zeroing), the person index, instance and fit record zeros.  No fit work is done for it.
 *    DETECTED (a seen entry that is not tracked, or an unbound person): t = the person's world; with b = best_cam, V = V_b of the
 *      view table widened to f64 and Rh = the rotation section 19 builds from heads[b][best_head].pose.rotation -- the angle
 *      table, M = Y Z, Rh = X M, rounded to f32 as there, and widened to f64 again --
 *        R[i][j] = (V[0][i] * Rh[0][j] + V[1][i] * Rh[1][j]) + V[2][i] * Rh[2][j]        (V_b^T Rh), rounded to f32 once;
 *      views = the person's views & pm; schedule (coarse_iterations, iterations) of the step's dh_fit_params.
 *    The start is a dh_view_instance: first_cam c0, model 0, views, R, t, the tracker's scale, flags 0.
 * 3. FIT.  The rule of the section above, unchanged, on the start with the step's dh_fit_params (gates, lambda, min_points) and
 *    the start's own schedule (an empty mask included: every sum is zero then).
 * 4. ACCEPTANCE.  Section 19's reason bits on the dh_view_fit_record: DH_FIT_TRACK_BAD_STATUS  status != DH_FIT_OK;
 *    DH_FIT_TRACK_BAD_POINTS  points (over all views) < keep_points;  DH_FIT_TRACK_BAD_RMS  sum_r2_fixed > (int64)(rms_max * rms_max
 *    * 1048576.0) * (int64)points (the cast made once, on the host);  DH_FIT_TRACK_BAD_JUMP  the slot is seen and not ((dx * dx + dy *
 *    dy) + dz * dz <= max_jump * max_jump) with d = (double)t_fit - (double)world of its person, in f64 (a NaN rejects).
 * 5. OUTCOME.  Accepted: t_prev = t; R, t = the fitted instance's; views_used = the record's; have_prev = the old tracked;
 *    tracked = 1; age = age + 1; lost = 0 (an unseen entry too: it is followed as long as the model holds it); status
 *    DH_FIT_TRACK_CARRIED when the start was the carried one, else DH_FIT_TRACK_FITTED.  Not accepted: R, t, t_prev, views_used
 *    stay; tracked = have_prev = age = 0; lost = lost + 1; status DH_FIT_TRACK_REJECTED | the reason bits; a SEEN entry stays bound
 *    (its id is kept and the next step starts from the detection), an UNSEEN entry is freed (zeroed) after its record is
 *    written.  An unbound person runs the same from an entry of zeros, which is then dropped.
 * 6. OUTPUT.  records[g][s], one dh_rig_fit_record per slot: id (the entry's; the person's for an unbound person); the fitted
 *    instance when accepted, else the start; the fit's record; the status; age and lost after the step (before a zeroing);
 *    person = the index i of the slot's person in persons[g], or 0xffffffff when unseen.  Unused slots are zeros.
 * An entry lives only while the rig tracker still carries its id: the rig tracker drops an id after max_misses unmatched steps,
 * and an id that came back would be a new person.  So max_coast MUST NOT EXCEED the max_misses the ids come from:
 * dh_rig_fit_track_params carries that max_misses (default DH_TRACK_MAX_MISSES; pass the rig tracker's), create refuses a
 * max_coast above it, and the whole step refuses a rig tracker whose max_misses is below the tracker's max_coast.
 * dh_rig_fit_tracker_create: the tables and the model must outlive the tracker.  Every device buffer is allocated there (the
 * host forms' frame staging at the first host step, for its frame size): a _device step allocates nothing, uploads nothing but
 * kernel arguments, launches k_rig_fit_seed, the per-instance-schedule instance of k_fit_views and k_rig_fit_update on `stream`
 * and never waits on the host.  Steps of one tracker must be stream-ordered.  step_persons is the core step (host memory;
 * _device: device memory) with max_heads the row length of `heads`; step runs dh_rig_tracker_step_device of `rt` and then the
 * core step on one stream and also returns the rig step's outputs (rig_ids [n_cams][max_heads], tracks nullable).  records
 * [n_rigs][DH_RIG_MAX_TRACKS].  DH_EINVAL before anything is launched or allocated, with the outputs untouched:
 * create: NULL out / rig / views / model; unknown flags; a scale that is not finite; iterations_tracked above 64; rms_max or
 *   max_jump outside (0, 4096] (NaN included); max_coast above max_misses; a reserved word that is not 0; a view table bound to
 *   another dh_cameras handle than the rig table; a model on another device than the tables; |scale| * (the model's largest |v|)
 *   above DH_FIT_MAX_EXTENT; (cameras of the largest rig) * (the model's points) above DH_FIT_MAX_POINTS -- the device cannot
 *   refuse an instance at run time, so the bound of section 21's sums (2^62) is secured here.
 * step: NULL tracker / frames / n_heads / heads / n_persons / persons / records (and predictor, rig tracker, rig_ids for the
 *   whole step); w or h outside 1 .. DH_RENDER_MAX_SIZE; max_heads outside 1 .. DH_MAX_HEADS; the fit's own refusals of
 *   dh_fit_params; for the whole step a rig tracker of another rig table, one whose max_misses is below max_coast, and the rig
 *   step's own refusals.  reset: NULL tracker, a rig outside -1 .. n_rigs - 1.  state, params_default: NULL argument. */
typedef struct dh_rig_fit_track_params {
    uint32_t iterations_tracked;  /* 6: full steps of a carried start, at most 64 */
    uint32_t keep_points;         /* 30, counted over all views */
    double   rms_max;             /* 5.0 (mm), in (0, 4096] */
    double   max_jump;            /* 150.0 (mm), in (0, 4096] */
    uint32_t max_coast;           /* 3 steps without a present view; at most max_misses */
    uint32_t max_misses;          /* DH_TRACK_MAX_MISSES: the max_misses of the rig tracker the ids come from */
    uint64_t reserved[2];         /* 0 */
} dh_rig_fit_track_params;  /* 48 bytes */
typedef struct dh_rig_fit_state {
    uint32_t id;                  /* 0 = free entry */
    float    R[9], t[3], t_prev[3];
    uint64_t views_used;          /* of the last accepted fit */
    uint32_t tracked, have_prev, age, lost;
} dh_rig_fit_state;     /* 88 bytes, no padding */
typedef struct dh_rig_fit_record {
    dh_view_instance   instance;
    dh_view_fit_record fit;
    uint32_t id;
    uint32_t status;              /* DH_FIT_TRACK_*: kind in the low byte, reason bits above it */
    uint32_t age, lost;
    uint32_t person;              /* index into persons[g]; 0xffffffff: unseen */
    uint32_t reserved;            /* 0 */
} dh_rig_fit_record;    /* 128 bytes, no padding */
typedef struct dh_rig_fit_tracker dh_rig_fit_tracker;
int dh_rig_fit_track_params_default(dh_rig_fit_track_params *p);
/* params NULL selects dh_rig_fit_track_params_default */
int dh_rig_fit_tracker_create(const dh_rig *rig, const dh_fit_views *views, const dh_fit_model *model, float scale, uint32_t flags,
                              const dh_rig_fit_track_params *params, dh_rig_fit_tracker **out);
int dh_rig_fit_tracker_destroy(dh_rig_fit_tracker *t);
/* rig, or -1 for all, back to zeros; ordered on `stream` */
int dh_rig_fit_tracker_reset(dh_rig_fit_tracker *t, int rig, void *stream);
/* states [n_rigs][DH_RIG_MAX_TRACKS]; synchronises the device */
int dh_rig_fit_tracker_state(dh_rig_fit_tracker *t, dh_rig_fit_state *states);
int dh_rig_fit_tracker_step_persons(dh_rig_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                                    const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons, const dh_rig_person *persons,
                                    const dh_fit_params *fit_params, dh_rig_fit_record *records);
int dh_rig_fit_tracker_step_persons_device(dh_rig_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present, int max_heads,
                                           const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons,
                                           const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_fit_record *records,
                                           void *stream);
int dh_rig_fit_tracker_step(dh_predictor *p, dh_rig_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h,
                            const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads, uint32_t *rig_ids,
                            uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks, dh_rig_fit_record *records);
int dh_rig_fit_tracker_step_device(dh_predictor *p, dh_rig_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h,
                                   const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads,
                                   uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks,
                                   dh_rig_fit_record *records, void *stream);

/* ---- a shape per subject ----
 * The shape steps of sections 20 and 23 solve for an increment of the coefficients at the one model they are given; deforming the
 * model was the caller's step on the host.  A dh_fit_subjects keeps S deformable models of one base mesh ON THE DEVICE, one per
 * subject, evaluates each subject's coefficients into its model there, and the shape step over a set reads every instance at its
 * own subject's model: many subjects adapt at once and a whole alternation (fit, shape step, update) is stream-ordered with no
 * host wait.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  Arithmetic: f64 with + - * /, ONE
 * square root (correctly rounded, as IEEE 754 demands), compares and casts; every operation rounded on its own.
 * THE SET owns the base vertices v[n] (f32 triples), the triangles, each vertex's list of incident corners in ascending (triangle,
 *   corner) order (built once on the host), one dh_subject_state per subject and S models.  The basis (section 20) is borrowed and
 *   must outlive the set; K is its field count.  Every subject starts with all coefficients 0 and its model evaluated at them.
 * THE MODELS: dh_fit_subjects_model hands out subject s's model as an ordinary dh_fit_model that every call taking one accepts
 *   unchanged (dh_fit_depth*, dh_fit_depth_views*, the trackers, dh_fit_shape*, dh_fit_calibrate_views*).  It is owned by the set
 *   (never pass it to dh_fit_model_destroy), valid until the set is destroyed, and its contents change, stream-ordered, with each
 *   update: a call that reads it must be stream-ordered with the updates around it.  Its radius (dh_fit_model_info) is the SET'S
 *   BOUND, computed once in f64:  bound = radius(base) + (K * max_coeff) * (the basis's largest |B_k[i]|),
 *   radius(base) being the largest |v| as dh_fit_model_create computes it.  No coefficient the device can reach leaves
 *   [-max_coeff, max_coeff], so |v'| <= bound for every model the set ever holds, and the existing per-instance refusal
 *   |scale| * radius > DH_FIT_MAX_EXTENT keeps the magnitude arguments of sections 18 - 24 closed without the host knowing the
 *   coefficients.
 * THE UPDATE of subject s by its record r = records[s] (a dh_shape_record, what a shape step wrote):
 *   APPLY.  r.status != DH_SHAPE_OK: nothing is applied.  Else, if a delta[k], k < K, is not finite: rejected += 1, flags |=
 *     DH_SUBJECT_NONFINITE and nothing else changes.  Else for every k < K:  c_k = c_k + delta[k], then c_k > max_coeff becomes
 *     max_coeff and c_k < -max_coeff becomes -max_coeff, flags |= DH_SUBJECT_CLAMPED where either moved it; applied += 1.  The
 *     counters saturate at 2^32 - 1; the flags stay set until dh_fit_subjects_set_coeffs.
 *   POINTS, always from the BASE, never from the previous model, so nothing drifts:  x = (f64)v_i;  for k ascending
 *     x[j] = x[j] + c_k * (f64)B_k[i][j];  v'_i = (f32)x, rounded once (what fit.deform computes).
 *   NORMALS, from the f32 v' widened again (what fit.vertex_normals computes).  Per triangle (a, b, c):  u = v'_b - v'_a,
 *     w = v'_c - v'_a,  f = (u1 * w2 - u2 * w1,  u2 * w0 - u0 * w2,  u0 * w1 - u1 * w0).  Per vertex: m = +0.0, then m = m + f for
 *     every incident corner in (triangle, corner) order -- a triangle that names the vertex twice adds its f twice.  Then
 *     q = (m0 * m0 + m1 * m1) + m2 * m2,  ln = sqrt(q),  nrm = (f32)(m / (ln > 0 ? ln : 1)).  A vertex with ln = 0 keeps a zero
 *     normal: the fit never associates it (c < 0.0 fails), so nothing leaves the magnitude bound; zero_normals counts such
 *     vertices at the last evaluation.  Floating-point sums depend on their order, so the sum is a gather over the corner list in
 *     list order: no floating-point atomic anywhere.
 *   Every update evaluates ALL subjects, applied or not.
 * THE SHAPE STEP OVER A SET is ONE SHAPE STEP of section 20 with two changes: instance i is evaluated at the model of its subject
 *   subjects[i] (NULL: subject 0), and where fit_records is given, instance i takes no part unless fit_records[i].status is
 *   DH_FIT_OK (as if its subject were DH_SHAPE_SKIP) -- so the outputs of dh_fit_depth*_device chain straight in.  Sums, solve and
 *   records are section 20's, n_subjects <= S records; the per-instance refusals are section 20's with the set's bound for the
 *   model's radius, and so is the term limit.
 * CARRIED STARTS.  The instances of dh_fit_depth*_device are host memory, so a fit could not start from what an earlier fit left on
 *   the device.  dh_fit_depth_carried_device and its camera twin are dh_fit_depth_device and dh_fit_depth_cameras_device with one
 *   more argument, carried[n_instances] ON THE DEVICE (what an earlier dh_fit_depth*_device wrote to its `out`; it may be that very
 *   buffer of this call): after the upload of the call's tables one more kernel, k_fit_carry, gives instance i the R and t of
 *   carried[i] where all twelve are finite and R R^T is within DH_FIT_R_TOLERANCE of the identity (the tests of section 18, so its
 *   magnitude bound holds for whatever the buffer contains), and leaves the uploaded R and t elsewhere.  frame, mesh, scale and
 *   flags are always the host instance's, and every refusal of dh_fit_depth_device is made on the host instances as they are
 *   given.  DH_EINVAL in addition: carried NULL with n_instances > 0.
 * dh_fit_subjects_create -- DH_EINVAL before anything is allocated or launched, *out NULL, in this order: NULL out; NULL verts, tris or
 *   basis; n = 0 or above DH_FIT_MAX_POINTS; n_tris outside 1 .. DH_SUBJECTS_MAX_TRIS; n_subjects outside 1 ..
 *   DH_SHAPE_MAX_SUBJECTS; max_coeff not > 0 or not finite; device < 0; a vertex that is not finite; a triangle index >= n; a base
 *   mesh one of whose vertex normals is zero (as dh_fit_model_create refuses a zero normal); a basis of another n; a basis on
 *   another device.
 * dh_fit_subjects_set_coeffs (host, synchronous) sets the coefficients of subjects first .. first + count - 1 from coeffs[count][8]
 *   (f64; those of k >= K are ignored and kept 0), clears their flags, keeps their counters and evaluates those subjects.
 *   DH_EINVAL, nothing changed: NULL set or coeffs; first + count above S; a coefficient k < K that is not finite or whose magnitude
 *   exceeds max_coeff.
 * dh_fit_subjects_update (host records[S], synchronous) and dh_fit_subjects_update_device (device records[S]; exactly three kernels
 *   on `stream`, NULL = default stream -- k_subjects_apply, k_subjects_points, k_subjects_normals -- no host wait, no allocation) run
 *   THE UPDATE.  DH_EINVAL: NULL set or records.  dh_fit_subjects_state (host, synchronous; DH_EINVAL: NULL set or state) copies the S states out and
 *   dh_fit_subjects_read (host, synchronous; DH_EINVAL: NULL set, subject >= S) one subject's points and normals.  The host calls
 *   run on a stream of the set's own and wait for it alone: the caller orders them against device calls that use the models.
 * dh_fit_shape_subjects* -- DH_EINVAL as dh_fit_shape* and in its order, with a NULL subject set in place of the NULL model and basis,
 *   then, after the frames' refusals, a set that lives on another device than the fitter, and n_subjects outside 1 .. S.  The host forms skip an instance whose fit record is not DH_FIT_OK before any
 *   per-instance refusal.  The _device forms enqueue exactly three kernels on `stream`: k_shape_clear,
 *   k_shape_accumulate_subjects, k_shape_solve.  Bit-identical run to run and to tests/subjects_ref.py. */
#define DH_SUBJECTS_MAX_TRIS 131072u   /* triangles of a set's mesh */
#define DH_SUBJECT_CLAMPED 1u          /* dh_subject_state.flags: a coefficient was moved back to +-max_coeff */
#define DH_SUBJECT_NONFINITE 2u        /*   an increment that was not finite was rejected */
typedef struct dh_subject_state {
    double   coeffs[8];           /* offset 0:  c_k; 0 for k >= K */
    uint32_t applied;             /* offset 64: increments added */
    uint32_t rejected;            /* offset 68: increments rejected as not finite */
    uint32_t flags;               /* offset 72: DH_SUBJECT_* */
    uint32_t zero_normals;        /* offset 76: vertices whose normal was zero at the last evaluation */
} dh_subject_state;    /* 80 bytes, no padding */
typedef struct dh_fit_subjects dh_fit_subjects;
/* verts [n][3] f32 (mm), tris [n_tris][3] u32, basis of n points */
int dh_fit_subjects_create(const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis,
                           uint32_t n_subjects, double max_coeff, int device, dh_fit_subjects **out);
int dh_fit_subjects_destroy(dh_fit_subjects *s);
/* each pointer nullable; radius = the set's bound */
int dh_fit_subjects_info(const dh_fit_subjects *s, uint32_t *n, uint32_t *n_tris, uint32_t *n_fields, uint32_t *n_subjects,
                         double *radius, int *device);
/* *model: subject `subject`'s model, borrowed from the set.  DH_EINVAL: NULL set or model, subject >= S. */
int dh_fit_subjects_model(const dh_fit_subjects *s, uint32_t subject, const dh_fit_model **model);
int dh_fit_subjects_set_coeffs(dh_fit_subjects *s, uint32_t first, uint32_t count, const double *coeffs);
int dh_fit_subjects_state(dh_fit_subjects *s, dh_subject_state *state);
/* subject `subject`'s model as it stands: points [n][3] and normals [n][3] f32, each nullable */
int dh_fit_subjects_read(dh_fit_subjects *s, uint32_t subject, float *points, float *normals);
int dh_fit_subjects_update(dh_fit_subjects *s, const dh_shape_record *records);
int dh_fit_subjects_update_device(dh_fit_subjects *s, const dh_shape_record *records, void *stream);
/* as dh_fit_depth_device / dh_fit_depth_cameras_device; carried [n_instances] on the device */
int dh_fit_depth_carried_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9],
                                const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances,
                                uint32_t n_instances, const dh_render_instance *carried, const dh_fit_params *params,
                                dh_render_instance *out, dh_fit_record *records, void *stream);
int dh_fit_depth_cameras_carried_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                        const dh_fit_model *const *models, uint32_t n_models, const dh_render_instance *instances,
                                        uint32_t n_instances, const dh_render_instance *carried, const dh_fit_params *params,
                                        dh_render_instance *out, dh_fit_record *records, void *stream);
/* frames [n][h][w] u16; instances [n_instances]; subjects [n_instances] or NULL; fit_records [n_instances] or NULL; records [n_subjects] */
int dh_fit_shape_subjects(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                          const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                          const dh_fit_record *fit_records, const dh_shape_params *params, dh_shape_record *records);
int dh_fit_shape_subjects_cameras(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                  const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                  const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records,
                                  const dh_shape_params *params, dh_shape_record *records);
int dh_fit_shape_subjects_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                                 const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects,
                                 uint32_t n_subjects, const dh_fit_record *fit_records, const dh_shape_params *params,
                                 dh_shape_record *records, void *stream);
int dh_fit_shape_subjects_cameras_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                         const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                         const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records,
                                         const dh_shape_params *params, dh_shape_record *records, void *stream);

/* ---- a surface per subject ----
 * A basis of at most 8 fields cannot express a cheekbone, a brow or a jaw: whatever it does not span stays in the fit's residual.
 * A SURFACE SET is a dh_fit_subjects that holds, besides section 25's coefficients, one scalar offset o[s][i] (mm, f64) per subject
 * and vertex ALONG THE BASE MESH'S VERTEX NORMAL, and the SURFACE STEP re-estimates all offsets of all subjects from fitted frames
 * on the device.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  Arithmetic: f64 with + - * /,
 * compares and casts; every operation rounded on its own; the sums are int64 (their order is free); no floating-point atomic.
 * THE SET.  dh_fit_subjects_create_surface is dh_fit_subjects_create with one more argument, max_offset.  Besides what section 25
 *   holds, the set holds (all allocated at creation, nothing later): the base normals nb_i -- THE NORMALS of section 25 of the base
 *   vertices themselves (what fit.vertex_normals computes), as f32; each vertex's NEIGHBOUR LIST -- the unique vertices j != i
 *   that share an edge of a triangle with i, ascending; deg_i is its length; the offsets, all +0.0 at first; the step's sums, three
 *   u64 words per (subject, vertex), and four per subject (three used); two f64 per (subject, vertex) of scratch; one dh_surface_record per
 *   subject.  A set made by dh_fit_subjects_create is unchanged in every respect and every surface call refuses it.
 *   The set's bound grows:  bound = (radius(base) + (K * max_coeff) * largest) + max_offset * 1.01, 1.01 bounding |nb| (section 25
 *   derives |nrm| <= 1 + 1e-7).  No offset the device can reach leaves [-max_offset, max_offset], so the argument of section 25
 *   holds with this bound.
 * POINTS of a surface set, always from the base:  section 25's POINTS tree x (the fields for k ascending), then
 *   x[j] = x[j] + o_i * (f64)nb_i[j] for j = 0, 1, 2;  v'_i = (f32)x, rounded once.  NORMALS are section 25's, from v'.
 *   dh_fit_subjects_update, _update_device and _set_coeffs on a surface set evaluate the points so (k_subjects_points_surface in
 *   place of k_subjects_points; ordinary sets run the kernel they ran).
 * THE SURFACE STEP, over frames, K or cameras, instances, subjects[], n_subjects and fit_records exactly as dh_fit_shape_subjects*
 *   takes them; an instance takes part by that call's rule (its subject < n_subjects, its fit record DH_FIT_OK where records are
 *   given, none of the per-instance refusals) and, in addition, only while |scale| <= DH_SURFACE_MAX_SCALE.
 *   ACCUMULATE.  For every instance that takes part and every point i of its subject's model: p, nrm, c, the pixel, d and
 *     res = c * (d / p.z - 1) are the fit's one pass (section 18) at the instance's pose with gate `gate`; the point is kept only
 *     if it passes that and  c * c >= min_cos2 * ((p0 * p0 + p1 * p1) + p2 * p2)  (a grazing point carries a bad normal).  Then
 *     sb = (f64)nb_i * scale (per component),  w_r = (R[r][0] * sb0 + R[r][1] * sb1) + R[r][2] * sb2,
 *     J = (nrm0 * w0 + nrm1 * w1) + nrm2 * w2,  and with S = 2^20:
 *       a[s][i] += (int64)((J * J) * S);   b[s][i] += (int64)((J * res) * S);   cnt[s][i] += 1;
 *     and per subject  e += (int64)((res * res) * S), points += 1, and instances += 1 for every instance that kept a point.
 *     The sign is section 20's: a positive solution moves the model point along its normal toward the measurement.
 *     Magnitudes: |nb| <= 1.01, |R x| <= 1.03 |x| and |nrm| <= 1.05 give |J| <= 1.05 * 1.03 * 1.01 |scale| < 1.1 |scale| <= 70.4;
 *     the gate lies in (0, DH_SHAPE_MAX_GATE], so |res| < 538 while |p| <= 2 p.z (section 20): J J < 2^12.3, J res < 2^15.3, times
 *     2^20, times at most DH_SHAPE_MAX_TERMS = 2^23 instances into one vertex's words: below 2^59; e is section 20's word with its
 *     limit of 2^23 (instance, point) terms of one subject.  Outside |p| <= 2 p.z the words of section 20 hold.
 *   SOLVE, per subject s < n_subjects.  points < min_points: DH_SURFACE_FEW_POINTS, the offsets stay as they were.  Otherwise, per
 *     vertex:  A_i = (f64)(int64)a_i / S and B_i = (f64)(int64)b_i / S where cnt_i >= min_count, both +0.0 elsewhere;
 *     u = o; then exactly `iterations` JACOBI sweeps, every u' from the u of the sweep before:
 *       u'_i = ((A_i * o_i + B_i) + mu * s_i) / ((A_i + mu * (f64)deg_i) + eps),   s_i = +0.0, then s_i = s_i + u_j for every j of
 *       i's neighbour list in list order.
 *     It descends  sum_i A_i (u_i - o_i - B_i / A_i)^2 + mu * sum_edges (u_i - u_j)^2 + eps * sum_i u_i^2:  a vertex never seen is
 *     filled from its neighbours and decays to 0; the denominator is positive since eps > 0.  After the sweeps, per vertex: a u_i
 *     that is not finite keeps o_i and is counted (rejected); else u_i > max_offset becomes max_offset, u_i < -max_offset becomes
 *     -max_offset, each counted (clamped); o_i = u_i.  With iterations = 0, u = o.
 *   One dh_surface_record per subject: status; points; instances; observed = the vertices with cnt_i >= min_count; clamped;
 *     rejected; sum_r2_fixed = e; max_abs = the largest |o_i| of the subject after the step.  With DH_SURFACE_FEW_POINTS observed,
 *     clamped and rejected are 0 and max_abs is that of the offsets as they stand.
 *   Then POINTS and NORMALS of subjects 0 .. n_subjects - 1 (zero_normals counted anew): the models are current when the call
 *   returns (host forms) or when the stream reaches the end of the call (_device forms).
 * dh_fit_subjects_create_surface -- DH_EINVAL as dh_fit_subjects_create and in its order, then: max_offset not finite or outside
 *   (0, DH_SURFACE_MAX_OFFSET]; n_subjects * n above DH_SURFACE_MAX_CELLS (the sums are 24 bytes a cell: 100 MB at the limit).
 * dh_fit_subjects_set_offsets (host, synchronous) sets subject `subject`'s offsets from offsets[n] (f64) and evaluates that subject.
 *   DH_EINVAL, nothing changed: NULL set or offsets; a set without offsets; subject >= S; a value that is not finite or whose
 *   magnitude exceeds max_offset.  dh_fit_subjects_read_offsets (host, synchronous) copies out subject `subject`'s offsets [n] f64
 *   and the last step's cnt_i as counts [n] u32 (saturated; what the words hold: 0 after creation, stale for a subject the last
 *   step did not name), each nullable.  DH_EINVAL: NULL set; a set without offsets; subject >= S.
 * dh_fit_surface_subjects* -- DH_EINVAL, before anything is launched and with nothing written, in this order: NULL fitter, frames,
 *   records, subject set; the frames' refusals of dh_fit_shape*; a set on another device than the fitter; a set without offsets;
 *   n_subjects outside 1 .. S; a non-finite gate, min_cos2, mu or eps; a gate outside (0, DH_SHAPE_MAX_GATE]; min_cos2 outside
 *   [0, 1]; mu < 0; eps not > 0; min_count 0; min_points 0; iterations above DH_SURFACE_MAX_ITERATIONS; a reserved word that is not
 *   0; NULL instances with n_instances > 0; n_instances above DH_SHAPE_MAX_TERMS.  The host forms then refuse, per instance that
 *   takes part, what dh_fit_shape_subjects refuses (with the set's bound), then |scale| above DH_SURFACE_MAX_SCALE, then a subject
 *   whose instances times n exceed DH_SHAPE_MAX_TERMS.  The _device forms cannot read the instances: they refuse n_instances * n
 *   above DH_SHAPE_MAX_TERMS and the device skips every instance one of the per-instance refusals names.  n_instances = 0 is no
 *   error: every record is DH_SURFACE_FEW_POINTS.  params is host memory in both forms; NULL selects
 *   dh_fit_surface_params_default.  The _device forms enqueue exactly five kernels on `stream` (NULL = default stream), no host
 *   wait, no allocation: k_surface_clear, k_surface_accumulate, k_surface_solve, k_subjects_points_surface, k_subjects_normals.
 *   A set serves one surface step at a time (the sums are the set's).  Bit-identical run to run and to tests/surface_ref.py. */
#define DH_SURFACE_OK 0u
#define DH_SURFACE_FEW_POINTS 1u         /* the subject's instances kept fewer than min_points points */
#define DH_SURFACE_MAX_OFFSET 64.0       /* mm: the largest max_offset of a set */
#define DH_SURFACE_MAX_SCALE 64.0        /* |scale| of an instance of a surface step */
#define DH_SURFACE_MAX_CELLS 4194304u    /* 2^22: subjects times vertices of a surface set */
#define DH_SURFACE_MAX_ITERATIONS 256u   /* Jacobi sweeps of a step */
typedef struct dh_surface_params {
    double   gate;                /* 25 (mm), in (0, DH_SHAPE_MAX_GATE] */
    double   min_cos2;            /* 0.25: the squared cosine between normal and ray below which a point is dropped, in [0, 1] */
    double   mu;                  /* 0.5: weight of the edge term, >= 0 */
    double   eps;                 /* 0.05: weight of the offsets themselves, > 0 */
    uint32_t min_count;           /* 2: a vertex seen fewer times has no data term */
    uint32_t min_points;          /* 64: fewer kept points of a subject give DH_SURFACE_FEW_POINTS */
    uint32_t iterations;          /* 32: Jacobi sweeps, at most DH_SURFACE_MAX_ITERATIONS */
    uint32_t reserved0;           /* 0 */
    uint64_t reserved[2];         /* 0 */
} dh_surface_params;   /* 64 bytes */
typedef struct dh_surface_record {
    uint32_t status;              /* offset 0:  DH_SURFACE_* */
    uint32_t points;              /* offset 4:  kept points of the subject's instances */
    uint32_t instances;           /* offset 8:  instances that kept a point */
    uint32_t observed;            /* offset 12: vertices with cnt >= min_count */
    uint32_t clamped;             /* offset 16: offsets moved back to +-max_offset */
    uint32_t rejected;            /* offset 20: solutions that were not finite */
    int64_t  sum_r2_fixed;        /* offset 24: e */
    double   max_abs;             /* offset 32: the largest |o_i| after the step */
} dh_surface_record;   /* 40 bytes, no padding */
int dh_fit_subjects_create_surface(const float *verts, uint32_t n, const uint32_t *tris, uint32_t n_tris, const dh_fit_basis *basis,
                                   uint32_t n_subjects, double max_coeff, double max_offset, int device, dh_fit_subjects **out);
int dh_fit_subjects_set_offsets(dh_fit_subjects *s, uint32_t subject, const double *offsets);
int dh_fit_subjects_read_offsets(dh_fit_subjects *s, uint32_t subject, double *offsets, uint32_t *counts);
int dh_fit_surface_params_default(dh_surface_params *p);
/* frames [n][h][w] u16; instances [n_instances]; subjects [n_instances] or NULL; fit_records [n_instances] or NULL; records [n_subjects] */
int dh_fit_surface_subjects(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set,
                            const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects, uint32_t n_subjects,
                            const dh_fit_record *fit_records, const dh_surface_params *params, dh_surface_record *records);
int dh_fit_surface_subjects_cameras(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                    dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                    const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records,
                                    const dh_surface_params *params, dh_surface_record *records);
int dh_fit_surface_subjects_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], dh_fit_subjects *set,
                                   const dh_render_instance *instances, uint32_t n_instances, const uint32_t *subjects,
                                   uint32_t n_subjects, const dh_fit_record *fit_records, const dh_surface_params *params,
                                   dh_surface_record *records, void *stream);
int dh_fit_surface_subjects_cameras_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                           dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                           const uint32_t *subjects, uint32_t n_subjects, const dh_fit_record *fit_records,
                                           const dh_surface_params *params, dh_surface_record *records, void *stream);

/* ---- identifying the subject of a fitted head ----
 * Sections 25 and 26 keep a gallery on the device, but every call that uses it must be TOLD who is in each frame.  This call
 * answers that: given fitted heads and a set, it says for each head which enrolled subject it is, or that it is none of them.
 * Not in the reference: PARITY UNPINNED, the definition below is this library's.  Arithmetic: f64 with + - * /, compares and
 * casts; every operation rounded on its own; the sums are int64 (their order is free); no floating-point atomic.
 * INPUTS: frames with one K or a camera table; a subject set (ordinary or surface) and n_subjects <= S; enrolled[n_subjects], u8,
 *   nullable: subject s is a CANDIDATE where enrolled is NULL or enrolled[s] != 0 (a fresh set's unenrolled subjects all hold the
 *   generic head and would tie, hence the mask); n_instances fitted instances -- what dh_fit_depth* wrote; `mesh` and `flags` are
 *   ignored; fit_records[n_instances], nullable; a dh_ident_params (NULL: dh_fit_ident_params_default).
 * TAKING PART.  Instance i takes part by the rule of dh_fit_shape_subjects*: its frame is below n; fit_records[i].status is
 *   DH_FIT_OK where records are given; none of the per-instance refusals of section 18 and 20 applies, with the set's bound for
 *   the model's radius and the basis's largest |B_k[i]|.
 * THE SCORE of pair (i, s), for every instance i that takes part and every candidate s, is section 18's fit of subject s's model
 *   AS THE SET HOLDS IT NOW at frame instances[i].frame, started at the instance's (R, t) with its scale, on the schedule
 *   coarse_iterations = 0, `iterations` full steps at gate `gate` with `lambda`, and `min_points` for the fit's own min_points:
 *   a pass that associates fewer points ends it DH_FIT_FEW_POINTS, a pivot that is not > 0 DH_FIT_SINGULAR, a step with every
 *   |x_a| < 1e-6 ends it early, all as in section 18; then the last pass at `gate`.  The score is that fit's dh_fit_record
 *   (points, steps, status, sum_r2_fixed) and its refitted pose, R and t rounded to f32 once.  With iterations = 0 it is one pass
 *   at the given pose.  The sums are the fit's 29 words and their magnitude argument holds as it stands: the set's bound in the
 *   extent test keeps it closed for every model the set can hold (sections 25 and 26).
 * THE DECISION for instance i.  E, the ELIGIBLE candidates, are those whose score has status DH_FIT_OK and points >= min_points.
 *   For s in E:  m_s = ((f64)sum_r2_fixed / 2^20) / (f64)points  -- two correctly rounded divisions; finite, since min_points >= 6.
 *   (m_a, a) PRECEDES (m_b, b) when m_a < m_b, or m_a == m_b and a < b: a tie goes to the lower index.  best is the s in E
 *   that precedes all others, second the same over E without best.  The status is the first of these that applies:
 *     DH_IDENT_SKIPPED       the instance takes no part;
 *     DH_IDENT_NO_CANDIDATE  E is empty;
 *     DH_IDENT_FAR           not  m_best <= max_rms * max_rms  (the product formed once, on the host, in f64);
 *     DH_IDENT_AMBIGUOUS     a second exists and not  m_second >= min_ratio * m_best;
 *     DH_IDENT_OK            otherwise.
 * OUTPUTS per instance.  subjects_out[i] = best where the status is DH_IDENT_OK, else DH_IDENT_UNKNOWN -- which IS DH_SHAPE_SKIP,
 *   so the array can be handed to a shape or surface step as `subjects` unchanged and unknown heads take no part.  records[i], a
 *   dh_ident_record: best and second are reported whatever the status is (DH_IDENT_UNKNOWN where there is none, with points and
 *   sum_r2_fixed 0).  poses_out[i], nullable: the input instance with R and t replaced by the best pair's refitted pose where E is
 *   not empty, else the input copied through.  scores, nullable, [n_instances][n_subjects] dh_fit_record: every pair's score;
 *   a pair that did not run (its subject no candidate, its instance taking no part) holds zeros.
 * dh_fit_identify_subjects* -- argument order as dh_fit_surface_subjects*.  The host forms are synchronous and take host frames,
 *   instances, enrolled, fit_records and outputs.  The _device forms take all of these on the device (params stays host memory),
 *   enqueue exactly two kernels on `stream` (NULL = default stream) -- k_ident_score, one workgroup per (instance, subject) pair,
 *   and k_ident_decide, one wave per instance -- with no host wait, ordered after whatever the stream held (a _device fit, a
 *   _device update of the set).  The pair scratch -- one score and one pose per pair -- is the fitter's: taken at the first call,
 *   it grows as the fitter's other tables do (growing waits for the device; a call that fits allocates nothing).
 *   DH_EINVAL, before anything is launched and with nothing written, in this order: NULL fitter, frames, subjects_out, records,
 *   subject set; the frames' refusals of dh_fit_shape*; a set on another device than the fitter; n_subjects outside 1 .. S; a NaN
 *   in gate, lambda, max_rms or min_ratio; iterations above 64; a gate outside (0, 4096]; lambda negative or infinite; min_points
 *   below 6; max_rms not > 0 (+inf is allowed and disables the limit); min_ratio below 1; a reserved word that is not 0; NULL
 *   instances with n_instances > 0; n_instances * n_subjects above DH_IDENT_MAX_PAIRS.  The host forms then refuse, per instance
 *   whose fit record is DH_FIT_OK (or all, without records), what dh_fit_shape_subjects refuses: a frame >= n, then the
 *   per-instance refusals with the set's bound.  The _device forms cannot read the instances: the device skips every instance one
 *   of these names (DH_IDENT_SKIPPED).  n_instances = 0 is no error and writes nothing.
 *   Bit-identical run to run and to tests/ident_ref.py.
 * THE DEFAULT max_rms is measured (tests/test_ident_ref.py): three subjects enrolled from 8 frames each, 4
 *   held-out frames of each and of a stranger identified.  The largest best mean square of the 12 known probes was 2.2557 mm^2,
 *   the smallest of the 4 stranger probes 3.5547 mm^2; the default is the square root of their geometric mean, rounded to 1.68. */
#define DH_IDENT_OK 0u
#define DH_IDENT_SKIPPED 1u              /* the instance takes no part */
#define DH_IDENT_NO_CANDIDATE 2u         /* no candidate's score is eligible */
#define DH_IDENT_FAR 3u                  /* the best mean square exceeds max_rms^2: none of the candidates */
#define DH_IDENT_AMBIGUOUS 4u            /* the second is within min_ratio of the best */
#define DH_IDENT_UNKNOWN 0xFFFFFFFFu     /* subjects_out[i], best, second: no subject (== DH_SHAPE_SKIP) */
#define DH_IDENT_MAX_PAIRS 4194304u      /* 2^22: instances times subjects of a call */
#define DH_IDENT_DEFAULT_MAX_RMS 1.68    /* mm: sqrt(sqrt(2.2557 * 3.5547)) = 1.6828 (the measurement above) */
typedef struct dh_ident_params {
    uint32_t iterations;          /* offset 0:  4: full steps of a pair's refit, at most 64 */
    uint32_t min_points;          /* offset 4:  64: of the refit and of eligibility, at least 6 */
    double   gate;                /* offset 8:  25 (mm), in (0, 4096] */
    double   lambda;              /* offset 16: 1e-3 */
    double   max_rms;             /* offset 24: DH_IDENT_DEFAULT_MAX_RMS (mm), > 0; +inf disables the limit */
    double   min_ratio;           /* offset 32: 1.0, which disables the test; >= 1 */
    uint64_t reserved[3];         /* offset 40: 0 */
} dh_ident_params;     /* 64 bytes */
typedef struct dh_ident_record {
    uint32_t status;              /* offset 0:  DH_IDENT_* */
    uint32_t best;                /* offset 4:  the best eligible candidate, or DH_IDENT_UNKNOWN */
    uint32_t second;              /* offset 8:  the second, or DH_IDENT_UNKNOWN */
    uint32_t eligible;            /* offset 12: |E| */
    uint32_t points_best;         /* offset 16: points of the best's score */
    uint32_t points_second;       /* offset 20 */
    int64_t  sum_r2_best;         /* offset 24: sum_r2_fixed of the best's score */
    int64_t  sum_r2_second;       /* offset 32 */
} dh_ident_record;     /* 40 bytes, no padding */
int dh_fit_ident_params_default(dh_ident_params *p);
/* frames [n][h][w] u16; enrolled [n_subjects] u8 or NULL; instances [n_instances]; fit_records [n_instances] or NULL; subjects_out
 * [n_instances] u32; records [n_instances]; poses_out [n_instances] or NULL; scores [n_instances][n_subjects] or NULL */
int dh_fit_identify_subjects(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                             const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled, uint32_t n_subjects,
                             const dh_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out,
                             dh_ident_record *records, dh_render_instance *poses_out, dh_fit_record *scores);
int dh_fit_identify_subjects_cameras(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                     const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                     const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records,
                                     const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                     dh_render_instance *poses_out, dh_fit_record *scores);
int dh_fit_identify_subjects_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const float K[9], const dh_fit_subjects *set,
                                    const dh_render_instance *instances, uint32_t n_instances, const uint8_t *enrolled,
                                    uint32_t n_subjects, const dh_fit_record *fit_records, const dh_ident_params *params,
                                    uint32_t *subjects_out, dh_ident_record *records, dh_render_instance *poses_out,
                                    dh_fit_record *scores, void *stream);
int dh_fit_identify_subjects_cameras_device(dh_fitter *f, const uint16_t *frames, int n, int w, int h, const dh_cameras *c,
                                            const dh_fit_subjects *set, const dh_render_instance *instances, uint32_t n_instances,
                                            const uint8_t *enrolled, uint32_t n_subjects, const dh_fit_record *fit_records,
                                            const dh_ident_params *params, uint32_t *subjects_out, dh_ident_record *records,
                                            dh_render_instance *poses_out, dh_fit_record *scores, void *stream);

/* ---- identifying enrolled subjects across the views of a rig ----
 * The call above asks the gallery about a head seen through ONE camera.  A rig's fit (section 21) ends in one WORLD pose per person
 * and the mask of the cameras that see it; this call asks the gallery about such a person from ALL those cameras at once: one score
 * per (person, candidate), its sums taken over every (view, point) pair.  Not in the reference: PARITY UNPINNED, the definition
 * below is this library's.  The arithmetic conventions are the fit's: f64 with + - * /, compares and casts; every operation rounded
 * on its own; the sums are int64 (their order is free); no floating-point atomic; no library function on the device.
 * INPUTS: frames [n_sets][n][h][w] u16 with n the view table's cameras -- frame s * n + c is camera c at set s, as in
 *   dh_fit_shape_views*; a dh_fit_views table and through it the camera table; a subject set (ordinary or surface); n_instances
 *   dh_view_instance -- what dh_fit_depth_views* wrote; `model` and `flags` are ignored; sets[n_instances] (NULL: every instance is
 *   in set 0); enrolled[n_subjects], u8, nullable (NULL: every subject is a candidate), and n_subjects <= S, as in the section
 *   above; fit_records[n_instances] of dh_view_fit_record, nullable; a dh_ident_params (NULL: dh_fit_ident_views_params_default).
 * TAKING PART.  Instance i takes part when every one of these tests passes, in this order, a NaN failing each:
 *     1. views != 0;
 *     2. the highest set bit of views names a camera first_cam + k < n;
 *     3. its set is < n_sets;
 *     4. where fit records are given, fit_records[i].status is DH_FIT_OK;
 *     5. none of the refusals of section 18 and 20 for R, t and scale applies, with the set's bound for the model's radius and the
 *        basis's largest |B_k[i]|;
 *     6. popcount(views) * (the set's points) <= DH_FIT_MAX_POINTS, which keeps section 21's bound of 2^62 on the sums.
 *   (1 - 3 and 5 are the tests of dh_fit_shape_views* for one subject.)
 * THE SCORE of pair (i, s), for every instance i that takes part and every candidate s, is section 21's fit of subject s's model AS
 *   THE SET HOLDS IT NOW, started at the instance's world (R, t) with its scale, over the views of its mask, in the frames of its
 *   set (frame sets[i] * n + c for camera c), on the schedule coarse_iterations = 0, `iterations` full steps at gate `gate` with
 *   `lambda`, and `min_points` for the fit's own min_points -- DH_FIT_FEW_POINTS, DH_FIT_SINGULAR and the early exit as in section 21 --
 *   then the last pass at `gate`.  The score is that fit's dh_view_fit_record (points, steps, status, sum_r2_fixed, views_used) and
 *   its refitted world pose, R and t rounded to f32 once.  With iterations = 0 it is one pass at the given pose.
 * THE DECISION is the section above's, unchanged, over the scores' points, status and sum_r2_fixed: the eligible candidates, the
 *   mean square m_s (two divisions), the order with its tie to the lower index, DH_IDENT_SKIPPED / NO_CANDIDATE / FAR / AMBIGUOUS /
 *   OK, and DH_IDENT_UNKNOWN == DH_SHAPE_SKIP.  All candidates of an instance share one view mask, so points counts the same (view,
 *   point) pairs for each and the means are comparable; m_s is a mean over all the views.
 * OUTPUTS per instance.  subjects_out[i] and records[i] (a dh_ident_record) as in the section above.  poses_out[i], nullable, a
 *   dh_view_instance: the input with R and t replaced by the best pair's refitted world pose where there is a best, else the input
 *   copied through.  scores, nullable, [n_instances][n_subjects] dh_view_fit_record: every pair's score; a pair that did not run
 *   holds zeros.
 * IDENTITY WITH THE SINGLE-VIEW CALL.  With one view, V = I, u = 0 and n_sets = 1 every subject, every record byte and every
 *   refitted pose equals dh_fit_identify_subjects_cameras on the same pose, and every score equals the single-view score in its
 *   first 24 bytes (section 21 shows that every sum is then section 18's).
 * dh_fit_identify_subjects_views takes host frames, instances, sets, enrolled, fit_records and outputs and is synchronous.
 *   dh_fit_identify_subjects_views_device takes all of these on the device (params stays host memory), enqueues exactly two
 *   kernels on `stream` (NULL = default stream) -- k_ident_views_score, one workgroup per (instance, subject) pair, and
 *   k_ident_views_decide, one wave per instance -- and never waits on the host: it chains after dh_fit_depth_views_device, whose
 *   `out` and `records` are its `instances` and `fit_records`.  The pair scratch is the fitter's and grows as the section above's
 *   does (growing waits for the device; a call that fits allocates nothing); the poses share that section's buffer, so ALL IDENTIFY
 *   CALLS OF ONE FITTER, of this section and the one above, MUST BE STREAM-ORDERED WITH ONE ANOTHER.
 *   DH_EINVAL, before anything is launched and with nothing written, in this order: NULL fitter, frames, subjects_out, records,
 *   subject set; a NULL view table or one of another device than the fitter; n_sets of 0 or n_sets * n above 65535; w or h outside
 *   1 .. DH_RENDER_MAX_SIZE; a set on another device than the fitter; n_subjects outside 1 .. S; the params' refusals of the section
 *   above, in its order; NULL instances with n_instances > 0; n_instances * n_subjects above DH_IDENT_MAX_PAIRS.  The host form then
 *   refuses, per instance, each of the tests of TAKING PART in their order -- except that an instance which passes tests 1 - 3 and
 *   whose fit record is not DH_FIT_OK is no error: it is DH_IDENT_SKIPPED.  The _device form cannot read the instances: the device
 *   skips, AS A WHOLE, every instance that fails a test (DH_IDENT_SKIPPED), so no input leads out of a buffer or out of the
 *   magnitude bound.  n_instances = 0 is no error and writes nothing.
 *   Bit-identical run to run and to tests/ident_views_ref.py.
 * THE DEFAULT max_rms of this call is measured on its own (tests/test_ident_views_ref.py): section 27's 1.68
 *   was measured on single 320x240 views and does not carry over to a rig of 160x120 cameras.  Three subjects enrolled from the
 *   middle camera's frames of 4 sets each; 4 further sets of each and of a stranger fitted and identified over three views.  The
 *   largest best mean square of the 12 known probes was 4.0152 mm^2, the smallest of the 4 stranger probes 10.9989 mm^2; the
 *   default is the square root of their geometric mean, rounded to 2.58. */
#define DH_IDENT_VIEWS_DEFAULT_MAX_RMS 2.58   /* mm: sqrt(sqrt(4.0152 * 10.9989)) = 2.5779 (the measurement above) */
/* dh_fit_ident_params_default with max_rms = DH_IDENT_VIEWS_DEFAULT_MAX_RMS */
int dh_fit_ident_views_params_default(dh_ident_params *p);
/* frames [n_sets][n][h][w] u16 with n the view table's cameras; instances and sets (or NULL) [n_instances]; enrolled [n_subjects] u8
 * or NULL; fit_records [n_instances] or NULL; subjects_out [n_instances] u32; records [n_instances]; poses_out [n_instances] or
 * NULL; scores [n_instances][n_subjects] or NULL */
int dh_fit_identify_subjects_views(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                                   const dh_fit_subjects *set, const dh_view_instance *instances, uint32_t n_instances,
                                   const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects,
                                   const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out,
                                   dh_ident_record *records, dh_view_instance *poses_out, dh_view_fit_record *scores);
int dh_fit_identify_subjects_views_device(dh_fitter *f, const uint16_t *frames, uint32_t n_sets, int w, int h, const dh_fit_views *views,
                                          const dh_fit_subjects *set, const dh_view_instance *instances, uint32_t n_instances,
                                          const uint32_t *sets, const uint8_t *enrolled, uint32_t n_subjects,
                                          const dh_view_fit_record *fit_records, const dh_ident_params *params, uint32_t *subjects_out,
                                          dh_ident_record *records, dh_view_instance *poses_out, dh_view_fit_record *scores,
                                          void *stream);

/* ---- following each tracked head with its own subject's model ----
 * The fit tracker of section 19 follows every head with ONE model, the generic head; sections 25 - 27 keep a gallery of per-person
 * models on the device and can say whose a fitted head is.  A dh_subject_fit_tracker joins them: a track that starts is followed
 * with the generic model, identified against the gallery on the device, and from the next step on followed with its own subject's
 * model -- with no host wait and no allocation in a step.  Not in the reference: PARITY UNPINNED, the definition below is this
 * library's.  The arithmetic conventions are those of sections 19 and 27: f32 and f64 with + - * /, compares and casts, every
 * operation rounded on its own; int64 sums whose order is free; no sine, cosine or floating-point atomic on the device (the
 * angle table is section 19's).  tests/subject_track_ref.py restates it; the GPU equals it byte for byte.
 * CREATION: a camera table; a subject set of S subjects (ordinary or surface); a GENERIC dh_fit_model of the set's point count
 *   (its points need not be the set's base mesh); scale and flags (DH_FIT_TRACK_MOTION) as in section 19; a dh_fit_track_params
 *   (NULL: section 19's defaults), a dh_ident_params (NULL: dh_fit_ident_params_default) and a dh_subject_track_params (NULL:
 *   dh_subject_track_params_default); enrolled[S], u8, host memory, NULL meaning every subject is a candidate.  The tracker builds a
 *   device table of S + 1 models: entries 0 .. S - 1 name the set's models, whose buffers dh_fit_subjects_update* and the set_*
 *   calls rewrite in place -- an update of the set enqueued on the stream of the steps is seen by the next step --, entry S is the
 *   generic model.  The camera table, the set and the generic model must outlive the tracker.
 * STATE of camera c (dh_subject_track_state, 92 bytes): section 19's dh_fit_track_state, then `subject` (the bound subject < S, or
 *   DH_IDENT_UNKNOWN while unbound -- the library writes no other value), `wait` (accepted steps to pass before the next try),
 *   `tries` (identifications of this track that did not bind) and `bound_age` (accepted steps since the binding), the last two
 *   saturating at 2^32 - 1.  Created and reset to zeros with subject = DH_IDENT_UNKNOWN.
 * ONE STEP of camera c, from the inputs of section 19's step:
 * 1. Section 19's steps 0 - 6 on the first 76 bytes of the state, unchanged but for the start instance's `mesh`: the state's subject
 *    where it is < S (the camera is BOUND), else S.  The fit is section 18's over the table of S + 1 models: a bound camera is
 *    fitted with its subject's model as the set holds it now, an unbound one with the generic model.
 * 2. BINDING LIFECYCLE, on the state step 1 left.  tracked == 0 (the fit was rejected, there was no start, or an absent camera
 *    coasted past max_coast): subject = DH_IDENT_UNKNOWN, wait = tries = bound_age = 0.  Else, when this step's fit was ACCEPTED:
 *    a bound camera has bound_age = bound_age + 1; an unbound camera WANTS IDENTIFICATION when wait == 0 and (max_tries == 0 or
 *    tries < max_tries), and otherwise, when wait > 0, has wait = wait - 1.  Else (an absent camera within max_coast) nothing
 *    changes: the binding is kept.
 * 3. IDENTIFICATION of a camera that wants it is section 27's rule exactly: the one instance is this step's accepted fitted
 *    instance (frame c, fit record DH_FIT_OK), the frames and the camera table are the step's, the candidates the tracker's
 *    enrolled subjects among all S, the parameters the tracker's dh_ident_params; TAKING PART, THE SCORE of every (camera,
 *    candidate) pair and THE DECISION as stated there, with the set's models as they are at this point of the stream.  Status
 *    DH_IDENT_OK: subject = best, bound_age = 0 (two cameras may bind one subject).  Any other status: tries = tries + 1, wait =
 *    retry.  R and t of the state stay those of the accepted fit: the refitted pose of the best pair is not taken.
 * 4. OUTPUT.  One dh_subject_track_record per camera: `track`, section 19's record of step 1 (its instance names the mesh the
 *    fit used); `ident`, the identification's dh_ident_record, or where none ran all zeros with status DH_IDENT_SKIPPED; `subject`,
 *    the state's after the step; `model`, the subject whose model this step's fit used, DH_IDENT_UNKNOWN for the generic model
 *    or where no fit ran; `identified`, 1 where an identification ran, else 0; `tries` after the step.
 * A binding takes effect at the NEXT step's start.  dh_subject_fit_tracker_bind is the caller's own binding of one camera:
 *   subject < S binds it (wait = tries = bound_age = 0), DH_IDENT_UNKNOWN unbinds it (the same, and the track may be identified
 *   again); ordered on `stream`.  Rule 2 holds for it as for any binding: a camera that is not tracked keeps a caller's binding
 *   only through a step whose fit is accepted.  dh_subject_fit_tracker_set_enrolled replaces the mask (NULL: all candidates),
 *   ordered on `stream`; it returns once the mask has left the caller's memory.  Bindings made under an earlier mask stay.
 * A _device step allocates nothing, never waits on the host and is five launches on `stream`, a linear chain:
 *   k_subject_track_seed, the per-instance-schedule instance of k_fit, k_subject_track_update (which appends the cameras that
 *   want identification to a device list), k_subject_track_score -- a grid fixed at creation of min(n_cams * S, 2 * the device's
 *   compute units) workgroups that loop over the list's (camera, subject) pairs, so a step in which nobody wants identification
 *   costs a launch of workgroups that leave at once, not n_cams * S of them -- and k_subject_track_bind.  The pair scratch
 *   (n_cams * S scores and poses) is the tracker's own, allocated at creation.  Steps, resets, binds and mask changes of one
 *   tracker must be stream-ordered with one another and with the updates of its set.  The step functions take the arguments
 *   of dh_fit_tracker_step* with records [n_cams] of dh_subject_track_record.
 * DH_EINVAL before anything is launched, with the outputs untouched.  create, in this order: NULL out; unknown flags; a scale that
 *   is not finite; iterations_tracked above 64; rms_max or max_jump outside (0, 4096] (NaN included); conf_den 0 or conf_num >
 *   conf_den; a reserved word of the dh_fit_track_params that is not 0; NULL cameras, set or generic model; the dh_ident_params'
 *   refusals of section 27 in its order; a reserved word of the dh_subject_track_params that is not 0; a set or a generic model
 *   on another device than the camera table; a generic model whose point count is not the set's; |scale| * (the set's bound)
 *   above DH_FIT_MAX_EXTENT; |scale| * (the generic model's largest |v|) above DH_FIT_MAX_EXTENT; n_cams * S above
 *   DH_IDENT_MAX_PAIRS.  step: section 19's step refusals.  reset: NULL tracker, a camera outside -1 .. n - 1.  bind: NULL tracker, a
 *   camera outside 0 .. n - 1, a subject that is neither < S nor DH_IDENT_UNKNOWN.  set_enrolled, state, info, params_default: NULL
 *   tracker / argument (info's outputs are each nullable).
 * THE DEFAULTS.  retry = 4 and max_tries = 4 (tests/test_subject_track_ref.py: the runs that chose them);
 *   max_rms NULL-selected is section 27's DH_IDENT_DEFAULT_MAX_RMS. */
typedef struct dh_subject_track_params {
    uint32_t retry;               /* 4: accepted steps an unbound track waits after an identification that did not bind */
    uint32_t max_tries;           /* 4: identifications of one track that may fail before it stays generic; 0: no limit */
    uint64_t reserved[2];         /* 0 */
} dh_subject_track_params;  /* 24 bytes */
typedef struct dh_subject_track_state {
    dh_fit_track_state fit;       /* offset 0 */
    uint32_t subject;             /* offset 76: < S, or DH_IDENT_UNKNOWN */
    uint32_t wait;                /* offset 80 */
    uint32_t tries;               /* offset 84 */
    uint32_t bound_age;           /* offset 88 */
} dh_subject_track_state;   /* 92 bytes, no padding */
typedef struct dh_subject_track_record {
    dh_fit_track_record track;    /* offset 0 */
    dh_ident_record     ident;    /* offset 104 */
    uint32_t subject;             /* offset 144: the state's after the step */
    uint32_t model;               /* offset 148: whose model the step's fit used, or DH_IDENT_UNKNOWN */
    uint32_t identified;          /* offset 152: 0 or 1 */
    uint32_t tries;               /* offset 156 */
} dh_subject_track_record;  /* 160 bytes, no padding */
typedef struct dh_subject_fit_tracker dh_subject_fit_tracker;
int dh_subject_track_params_default(dh_subject_track_params *p);
/* track_params, ident_params, params, enrolled: each NULL selects its default (enrolled: all S subjects) */
int dh_subject_fit_tracker_create(const dh_cameras *c, const dh_fit_subjects *set, const dh_fit_model *generic, float scale, uint32_t flags,
                                  const dh_fit_track_params *track_params, const dh_ident_params *ident_params,
                                  const dh_subject_track_params *params, const uint8_t *enrolled, dh_subject_fit_tracker **out);
int dh_subject_fit_tracker_destroy(dh_subject_fit_tracker *t);
/* camera, or -1 for all, back to the initial state; ordered on `stream` */
int dh_subject_fit_tracker_reset(dh_subject_fit_tracker *t, int camera, void *stream);
/* states [n_cams]; synchronises the device */
int dh_subject_fit_tracker_state(dh_subject_fit_tracker *t, dh_subject_track_state *states);
/* the cameras, S, and the workgroups of k_subject_track_score; each output nullable */
int dh_subject_fit_tracker_info(const dh_subject_fit_tracker *t, int *n_cams, uint32_t *n_subjects, uint32_t *score_workgroups);
/* enrolled [S] u8, host memory, or NULL for all */
int dh_subject_fit_tracker_set_enrolled(dh_subject_fit_tracker *t, const uint8_t *enrolled, void *stream);
int dh_subject_fit_tracker_bind(dh_subject_fit_tracker *t, int camera, uint32_t subject, void *stream);
int dh_subject_fit_tracker_step_poses(dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                      const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params,
                                      dh_subject_track_record *records);
int dh_subject_fit_tracker_step_poses_device(dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                             const dh_pose *poses, const dh_support *support, const dh_fit_params *fit_params,
                                             dh_subject_track_record *records, void *stream);
int dh_subject_fit_tracker_step(dh_predictor *p, dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out, dh_support *support_out,
                                dh_subject_track_record *records);
int dh_subject_fit_tracker_step_device(dh_predictor *p, dh_subject_fit_tracker *t, const uint16_t *frames, int w, int h,
                                       const uint8_t *present, uint32_t radius, const dh_fit_params *fit_params, dh_pose *poses_out,
                                       dh_support *support_out, dh_subject_track_record *records, void *stream);

/* ---- following each rig person with its own subject's model ----
 * The rig twin of the section above: a dh_rig_subject_fit_tracker is section 22's rig fit tracker bound to a subject set.  An entry
 * that starts is followed with the generic model, identified OVER ALL ITS PRESENT VIEWS against the enrolled subjects on the device
 * (section 28), and from the next step on fitted with its own subject's model as the set holds it then -- with no host wait and no
 * allocation in a step.  Not in the reference: PARITY UNPINNED, the definition below is this library's.  It composes sections 22, 28
 * and 29 and restates none of them; the arithmetic conventions are theirs (f32 and f64 with + - * /, compares and casts, every
 * operation rounded on its own; int64 sums whose order is free; no sine, cosine or floating-point atomic on the device).
 * tests/rig_subject_track_ref.py restates it; the GPU equals it byte for byte.
 * CREATION: a rig table and a view table bound to ONE dh_cameras handle (section 22's contract on their consistency holds); a
 *   subject set of S subjects (ordinary or surface); a GENERIC dh_fit_model of the set's point count; scale and flags
 *   (DH_FIT_TRACK_MOTION); a dh_rig_fit_track_params (NULL: section 22's defaults), a dh_ident_params (NULL:
 *   dh_fit_ident_views_params_default) and a dh_subject_track_params (NULL: section 29's defaults); enrolled[S], u8, host memory,
 *   NULL meaning every subject is a candidate.  The tracker builds section 29's device table of S + 1 models -- entries 0 .. S - 1
 *   name the set's buffers, so an update of the set enqueued on the stream of the steps is seen by the next step; entry S is the
 *   generic model -- and allocates every device buffer of a step: the pair scratch [n_rigs * DH_RIG_MAX_TRACKS][S] of scores and
 *   poses, the want list and the per-slot words.  The tables, the set and the generic model must outlive the tracker.
 * STATE of rig g: DH_RIG_MAX_TRACKS entries of dh_rig_subject_state (104 bytes): section 22's dh_rig_fit_state, then section 29's
 *   `subject`, `wait`, `tries` and `bound_age`.  A free entry is zeros with subject = DH_IDENT_UNKNOWN: EVERY PLACE where section 22
 *   zeroes an entry -- a free entry taken for a new id, an unseen untracked entry freed by the bind, an entry freed after a coast past
 *   max_coast, an unseen entry freed after a rejection, reset -- also sets the four words to (DH_IDENT_UNKNOWN, 0, 0, 0).
 * ONE STEP of rig g, from the inputs of section 22's step:
 * 1. Section 22's steps 0 - 6 on the first 88 bytes of every entry, unchanged but for the start's `model`: the entry's subject (after
 *    the bind of step 1) where it is < S, else S.  An UNBOUND PERSON (one with no entry) is always fitted with model S, is never
 *    identified and carries nothing.  With pm == 0 the whole state of the rig, bindings included, is kept.
 * 2. BINDING LIFECYCLE: section 29's rule 2, per entry, on the state step 1 left.  tracked == 0 (a rejected fit; a freed entry is
 *    zeros): the binding is dropped, the four words (DH_IDENT_UNKNOWN, 0, 0, 0).  Else, when this step's fit was ACCEPTED (an unseen
 *    entry's too): a bound entry has bound_age = bound_age + 1 (saturating); an unbound entry WANTS IDENTIFICATION when wait == 0 and
 *    (max_tries == 0 or tries < max_tries), and otherwise, when wait > 0, has wait = wait - 1.  Else (a coast within max_coast)
 *    nothing changes.
 * 3. IDENTIFICATION of a slot that wants it is section 28's rule exactly: the one instance is the slot's accepted fitted
 *    dh_view_instance (its `views` are the start's mask), its fit record DH_FIT_OK, the frames the step's with n_sets = 1 and set 0,
 *    the candidates the tracker's enrolled subjects among all S, the parameters the tracker's dh_ident_params; TAKING PART (test 6
 *    holds for every mask: creation secures it), THE SCORE of every (slot, candidate) pair and THE DECISION as stated there, with the
 *    set's models as they are at this point of the stream.  DH_IDENT_OK: subject = best, bound_age = 0.  Any other status, SKIPPED
 *    from a failed test of taking part included: tries = tries + 1 (saturating), wait = retry.  The refitted pose is not taken.  Two
 *    slots of one rig MAY BIND ONE SUBJECT: a rule across the slots of a rig is not part of this section.
 * 4. OUTPUT.  records[g][s], one dh_rig_subject_record (184 bytes) per slot: `track`, section 22's record of the slot (its instance
 *    names the model of the table the fit used); `ident`, the identification's dh_ident_record, or where none ran all zeros with
 *    status DH_IDENT_SKIPPED; `subject`, the subject word of the slot's entry after the step; `model`, the subject whose model this
 *    step's fit used, DH_IDENT_UNKNOWN for the generic model or where no fit ran; `identified`, 1 where an identification ran, else
 *    0; `tries`, the entry's after the step.  A slot that is no entry after the step -- unused, an unbound person, a freed entry, and
 *    every slot of a rig with pm == 0 whose entry is free -- so reads subject = DH_IDENT_UNKNOWN and tries = 0: an UNUSED SLOT IS
 *    ZEROS BUT FOR ident.status = DH_IDENT_SKIPPED, subject = DH_IDENT_UNKNOWN and model = DH_IDENT_UNKNOWN.  In a rig with pm == 0
 *    track is section 22's (zeros, status DH_FIT_TRACK_ABSENT) and subject and tries are the kept entry's.
 * A binding takes effect at the NEXT step's start.  dh_rig_subject_fit_tracker_bind is the caller's own binding: it acts on the
 *   entry of `rig` that holds `id` -- subject < S binds it, DH_IDENT_UNKNOWN unbinds it, wait = tries = bound_age = 0 either way --
 *   and where no entry holds the id it does nothing; ordered on `stream` (one small launch).  Rule 2 holds for it as for any
 *   binding.  set_enrolled, reset (a rig, or -1), state, info (the rigs, S, the workgroups of k_rig_subject_score) are section 29's
 *   with a rig for a camera.  Section 22's condition on max_coast and max_misses holds unchanged.
 * A _device step allocates nothing, never waits on the host and is five launches on `stream`, a linear chain: k_rig_subject_seed,
 *   the per-instance-schedule instance of k_fit_views over the S + 1 table, k_rig_subject_update (which appends the slots that want
 *   identification to a device list), k_rig_subject_score -- a grid fixed at creation of min(n_rigs * DH_RIG_MAX_TRACKS * S, 2 * the
 *   device's compute units) workgroups that loop over the list's (slot, subject) pairs -- and k_rig_subject_bind.  Steps, resets,
 *   binds and mask changes of one tracker must be stream-ordered with one another and with the updates of its set.  The step
 *   functions take the arguments of dh_rig_fit_tracker_step* with records [n_rigs][DH_RIG_MAX_TRACKS] of dh_rig_subject_record.
 * DH_EINVAL before anything is launched or allocated, with the outputs untouched (create: *out NULL).  create, in this order: NULL
 *   out; unknown flags; a scale that is not finite; iterations_tracked above 64; rms_max or max_jump outside (0, 4096] (NaN included);
 *   max_coast above max_misses; a reserved word of the dh_rig_fit_track_params that is not 0; NULL rig, views, set or generic model;
 *   a view table bound to another dh_cameras handle than the rig table; the dh_ident_params' refusals of section 27 in its order; a
 *   reserved word of the dh_subject_track_params that is not 0; a set or a generic model on another device than the tables; a
 *   generic model whose point count is not the set's; |scale| * (the set's bound) above DH_FIT_MAX_EXTENT; |scale| * (the generic
 *   model's largest |v|) above DH_FIT_MAX_EXTENT; (cameras of the largest rig) * (the set's points) above DH_FIT_MAX_POINTS;
 *   n_rigs * DH_RIG_MAX_TRACKS * S above DH_IDENT_MAX_PAIRS.  step: section 22's step refusals.  reset: NULL tracker, a rig outside
 *   -1 .. n_rigs - 1.  bind: NULL tracker, a rig outside 0 .. n_rigs - 1, id 0, a subject that is neither < S nor DH_IDENT_UNKNOWN.
 *   set_enrolled, state, info: NULL tracker / argument (info's outputs are each nullable).
 * THE DEFAULTS.  retry and max_tries are section 29's; max_rms NULL-selected is section 28's DH_IDENT_VIEWS_DEFAULT_MAX_RMS
 *   (DESIGN.md section 30 holds the measurement on moving frames that keeps it). */
typedef struct dh_rig_subject_state {
    dh_rig_fit_state fit;         /* offset 0 */
    uint32_t subject;             /* offset 88: < S, or DH_IDENT_UNKNOWN */
    uint32_t wait;                /* offset 92 */
    uint32_t tries;               /* offset 96 */
    uint32_t bound_age;           /* offset 100 */
} dh_rig_subject_state;     /* 104 bytes, no padding */
typedef struct dh_rig_subject_record {
    dh_rig_fit_record track;      /* offset 0 */
    dh_ident_record   ident;      /* offset 128 */
    uint32_t subject;             /* offset 168: the entry's after the step */
    uint32_t model;               /* offset 172: whose model the step's fit used, or DH_IDENT_UNKNOWN */
    uint32_t identified;          /* offset 176: 0 or 1 */
    uint32_t tries;               /* offset 180 */
} dh_rig_subject_record;    /* 184 bytes, no padding */
typedef struct dh_rig_subject_fit_tracker dh_rig_subject_fit_tracker;
/* track_params, ident_params, params, enrolled: each NULL selects its default (enrolled: all S subjects) */
int dh_rig_subject_fit_tracker_create(const dh_rig *rig, const dh_fit_views *views, const dh_fit_subjects *set, const dh_fit_model *generic,
                                      float scale, uint32_t flags, const dh_rig_fit_track_params *track_params,
                                      const dh_ident_params *ident_params, const dh_subject_track_params *params, const uint8_t *enrolled,
                                      dh_rig_subject_fit_tracker **out);
int dh_rig_subject_fit_tracker_destroy(dh_rig_subject_fit_tracker *t);
/* rig, or -1 for all, back to the initial state; ordered on `stream` */
int dh_rig_subject_fit_tracker_reset(dh_rig_subject_fit_tracker *t, int rig, void *stream);
/* states [n_rigs][DH_RIG_MAX_TRACKS]; synchronises the device */
int dh_rig_subject_fit_tracker_state(dh_rig_subject_fit_tracker *t, dh_rig_subject_state *states);
/* the rigs, S, and the workgroups of k_rig_subject_score; each output nullable */
int dh_rig_subject_fit_tracker_info(const dh_rig_subject_fit_tracker *t, int *n_rigs, uint32_t *n_subjects, uint32_t *score_workgroups);
/* enrolled [S] u8, host memory, or NULL for all */
int dh_rig_subject_fit_tracker_set_enrolled(dh_rig_subject_fit_tracker *t, const uint8_t *enrolled, void *stream);
int dh_rig_subject_fit_tracker_bind(dh_rig_subject_fit_tracker *t, int rig, uint32_t id, uint32_t subject, void *stream);
int dh_rig_subject_fit_tracker_step_persons(dh_rig_subject_fit_tracker *t, const uint16_t *frames, int w, int h, const uint8_t *present,
                                            int max_heads, const uint32_t *n_heads, const dh_head *heads, const uint32_t *n_persons,
                                            const dh_rig_person *persons, const dh_fit_params *fit_params, dh_rig_subject_record *records);
int dh_rig_subject_fit_tracker_step_persons_device(dh_rig_subject_fit_tracker *t, const uint16_t *frames, int w, int h,
                                                   const uint8_t *present, int max_heads, const uint32_t *n_heads, const dh_head *heads,
                                                   const uint32_t *n_persons, const dh_rig_person *persons,
                                                   const dh_fit_params *fit_params, dh_rig_subject_record *records, void *stream);
int dh_rig_subject_fit_tracker_step(dh_predictor *p, dh_rig_subject_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w, int h,
                                    const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads, dh_head *heads,
                                    uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons, dh_rig_track *tracks,
                                    dh_rig_subject_record *records);
int dh_rig_subject_fit_tracker_step_device(dh_predictor *p, dh_rig_subject_fit_tracker *t, dh_rig_tracker *rt, const uint16_t *frames, int w,
                                           int h, const uint8_t *present, const dh_fit_params *fit_params, uint32_t *n_heads,
                                           dh_head *heads, uint32_t *rig_ids, uint32_t *n_persons, dh_rig_person *persons,
                                           dh_rig_track *tracks, dh_rig_subject_record *records, void *stream);

/* ---- BIWI Kinect Head Pose Database formats (frame ingest, src/db_reader/biwi.rs) ----
 * read_depth (biwi.rs:81-103): run-length coded depth `.bin` -> row-major u16.  Call with out == NULL
 * to obtain *w, *h.  Where the reference returns an io::Error (truncated file) or panics (a run
 * overruns the image) this returns DH_EINVAL. */
int dh_biwi_decode_depth(const uint8_t *buf, size_t len, uint16_t *out, size_t cap_px, uint32_t *w, uint32_t *h);
/* read_cal (biwi.rs:27-60): `depth.cal` text -> row-major 3x3 intrinsic (first three lines). */
int dh_biwi_parse_cal(const char *text, size_t len, float K[9]);
/* read_gt (biwi.rs:63-77): 24-byte pose file -> head position (mm), its projection, rotation (deg). */
int dh_biwi_parse_pose(const uint8_t *buf, size_t len, const float K[9], float pos3d[3], float pos2d[2], float rot[3]);

/* ---- training: HoughLearning (src/hough/prediction.rs:103-234) ----
 * HoughLearning::new(...).learn(sigma, data) grows the forests every HoughPrediction uses.  The parts the reference pins
 * (sample extraction, the feature generator, binarize, impurity, early_stop, comp_leaf_data) are restated exactly; the
 * random draws (thread_rng there) and stamm's tree growing are defined here, keyed by `seed` (DESIGN.md section 11:
 * PARITY UNPINNED).  A trainer is not thread-safe. */
typedef struct dh_train_params {
    uint32_t stepwidth;             /* sliding-window step (iterate_subimage, types.rs:352-384)              */
    uint32_t subimage_width;
    uint32_t subimage_height;
    uint32_t max_depth;             /* a node at depth >= max_depth is a leaf; the root has depth 0           */
    uint32_t n_trees;
    uint32_t subset_per_tree;       /* samples drawn (with replacement) from the pool for each tree           */
    double   subrect_feature_scale; /* in (0, 1]: every split rectangle is trunc(W * s) x trunc(H * s)        */
    uint32_t features_per_node;     /* candidates generated per node (>= 1)                                   */
    uint32_t min_subset_size;       /* a node with fewer samples is a leaf                                    */
    double   steepness;             /* > 0: regression weight 1 - exp(-depth / steepness)                     */
    uint64_t seed;
} dh_train_params; /* 56 bytes */

/* Statistics of a trainer: the pool after the last dh_trainer_add_frames, the rest of the last dh_trainer_fit. */
typedef struct dh_train_stats {
    uint64_t frames;          /* frames added                                                                  */
    uint64_t pool_size;       /* samples kept (at most 20 negatives + 20 positives per frame)                   */
    uint64_t pool_positives;
    uint64_t neg_det;         /* impurity evaluations whose det sum fell below -0.001 (the reference panics there,
                               * houghforest.rs:283); scored as 0                                               */
    uint32_t levels;          /* tree levels the last fit ran                                                   */
    uint32_t reserved;
} dh_train_stats; /* 40 bytes */

typedef struct dh_trainer dh_trainer;

/* Rejected with DH_EINVAL where HoughLearning::new returns None or the first node would panic: a factor outside (0, 1],
 * features == 0, steepness <= 0 (HoughTreeFunctions::new :143-158, random_subrect_iterator types.rs:106-109); also
 * n_trees == 0, stepwidth == 0, an empty patch, and (DH_ESIZE) a patch whose pixel sum can reach 2^32. */
int dh_trainer_create(const dh_train_params *p, int device, dh_trainer **out);
int dh_trainer_destroy(dh_trainer *t);
/* Sample extraction of learn (prediction.rs:145-215) for n frames (row-major u16 depth, u8 mask, index y*w+x); K: [n][9]
 * row-major intrinsics, pos3d [n][3] mm, rot_deg [n][3] degrees.  Frames are uploaded in chunks and windowed on the device;
 * only the kept samples stay resident.  The pool does not depend on how frames are split across calls.  Frames smaller
 * than the patch: DH_ESIZE.  A rot_deg a forest cannot hold as a vote (+-inf, or outside -543 < deg < 540; NaN is held):
 * DH_EINVAL, with nothing added.  Non-finite pos3d or offsets (e.g. a K whose third row gives r[2] = 0) are kept. */
int dh_trainer_add_frames(dh_trainer *t, const uint16_t *frames, const uint8_t *masks, int n, int w, int h, const float *K,
                          const float *pos3d, const float *rot_deg);
/* Grow n_trees trees on the device from the pool; *out is an ordinary forest (validated like dh_forest_create; child_one
 * is the Binar::One side).  The pool is kept: fitting again gives the same forest. */
int dh_trainer_fit(dh_trainer *t, dh_forest **out);
/* nodes_per_level / leaves_per_level / level_ms: [cap_levels] each, may be NULL (split nodes and leaves made at each
 * depth; device time of each level's kernels). */
int dh_trainer_stats(const dh_trainer *t, dh_train_stats *out, uint32_t *nodes_per_level, uint32_t *leaves_per_level,
                     float *level_ms, uint32_t cap_levels);

/* Copy a forest back into caller arrays sized by dh_forest_info and *n_off / *n_rot.  NULL array pointers are skipped:
 * call with all NULL to obtain the vote counts. */
int dh_forest_export(const dh_forest *f, int32_t *roots, dh_node *nodes, double *leaf_prob, uint32_t *off_begin,
                     uint32_t *rot_begin, float *offsets, double *rotations, uint32_t *n_off, uint32_t *n_rot);

/* ---- profiling ---- */
int dh_set_profiling(dh_predictor *p, int on); /* HIP events around each kernel, on the launch stream; and roctx ranges
                                                * ("dh:batch ...", "dh:boxsum", "dh:traverse", "dh:emit", "dh:vote", "dh:cluster") around the
                                                * launches, visible to rocprofv3 --marker-trace when a roctx library is present */
int dh_get_timing(dh_predictor *p, dh_timing *out); /* synchronises the recorded events */

/* ---- parity taps (tests only; each refers to the LAST batch run on this predictor) ----
 * dh_debug_enable(1) makes the next batch record leaf indices, patch flags and mean-shift traces. */
int dh_debug_enable(dh_predictor *p, int on);
/* [n][n_patches][n_trees] leaf index per (patch, tree), -1 for background patches. */
int dh_debug_leaf_indices(dh_predictor *p, int32_t *out, size_t cap_elems);
/* [n][n_patches]: bit0 = non-background (prediction.rs:567-571), bit1 = prob gate passed (:584). */
int dh_debug_patch_flags(dh_predictor *p, uint8_t *out, size_t cap_elems);
/* Coarse guess grids (prediction.rs:529-533): pos_grid [n][400], rot_grid [n][8000]. */
int dh_debug_grids(dh_predictor *p, uint32_t *pos_grid, uint32_t *rot_grid);
/* [n][6]: mean-shift start cells, mid x,y,z then rot x,y,z (prediction.rs:437-460, :750). */
int dh_debug_guesses(dh_predictor *p, int32_t *out);
/* Every vote of one frame as (x, y, z, value) records, unaggregated and in no particular order:
 * which = 0 the position accumulator `mid` (prediction.rs:667), 1 the rotation accumulator `rot`
 * (:635).  *count receives the number of votes (may exceed cap; then only cap are written). */
int dh_debug_votes(dh_predictor *p, int frame, int which, int32_t *out, size_t cap_records, size_t *count);
/* Mean-shift positions: trace [n][iterations+1][3] (entry 0 = start), steps [n] = updates done
 * (meanshift.rs:336-395). which as above. */
int dh_debug_meanshift(dh_predictor *p, int which, int32_t *trace, uint32_t *steps);
/* Per-frame number of (patch, leaf) hit records kept for voting. */
int dh_debug_hit_counts(dh_predictor *p, uint32_t *out);
/* Tiling the runtime chose for the current workspace (tests construct edge cases from it):
 * out[0..9] = path (bit 0: uniform-rectangle path; bit 8: its walks use the walk table (always, unless the forest has more than 4096
 * nodes with an ambiguity band); bit 9: the tiles of a batch run the probability gate themselves and list only the windows that pass
 * it (not with the taps on, nor under DH_NO_TILE_GATE); bits 16..: tree levels walked from LDS), tile px, py, tiles_x, tiles_y, column de-interleave log2,
 * plane stride q, LDS row stride, rectangle w, rectangle h. */
int dh_debug_geometry(dh_predictor *p, int32_t out[10]);
/* The tile lists of the last batch -- of its last resident slice, as for every tap, when DH_MAX_RESIDENT_FRAMES cut it into slices
 * (large batches in product mode; DH_ESTATE when it ran without them).  Each frame of such a batch
 * chooses the shift of its tile grid -- within the grid's slack over the window grid -- that leaves the fewest tiles to walk:
 * shifts [n][2] = {sx, sy} in windows per frame (zeros where the geometry or DH_TILE_SHIFT=off leaves the one shift (0, 0);
 * DH_TILE_SHIFT=sx,sy forces one shift), counts [8] = tiles walked for the frames = x mod 8.  Waits for the batch; debug only. */
int dh_debug_tile_shifts(dh_predictor *p, int32_t *shifts, uint32_t counts[8]);
/* [n]: per frame of the last batch, the windows that passed the probability gate (prediction.rs:582-584) -- patch flag 3 of
 * dh_debug_patch_flags, without the taps.  Waits for the batch; debug only. */
int dh_debug_window_totals(dh_predictor *p, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* DEPTHHEAD_HIP_H */
