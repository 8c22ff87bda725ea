// dh_train.h -- the host-only half of the trainer behind dh_trainer_* (include/depthhead_hip.h): parameter validation,
// the keyed random draws, the window grid, the upload chunk plan, and the level-by-level bookkeeping of tree growing
// (early_stop, comp_leaf_data, stable partitions, assembly of the forest in CSR form).  The device half (window pass,
// rectangle-sum images, split search) is k_train.hip; dh_api_train.hip sequences the two.
//
// Like dh_host.h, no HIP call appears in dh_train.cpp: it builds with plain g++ under AddressSanitizer / UBSan /
// ThreadSanitizer (tests/host/train_check.cpp).  The draws below are also compiled for the device (DH_HD).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "dh_host.h"

#if defined(__HIPCC__)
#define DH_HD __host__ __device__
#else
#define DH_HD
#endif

// ------------------------------------------------------------------ keyed draws (PARITY UNPINNED: thread_rng in the reference)
// Every draw is a pure function of (seed, purpose tag, a, b): no draw depends on launch order, chunking or thread count.
enum { DH_TAG_WINDOW = 1, DH_TAG_SUBSET = 2, DH_TAG_CAND = 3 };
#define DH_TRAIN_KEEP 20   // negatives and positives kept per frame (prediction.rs:212-215)
#define DH_TRAIN_MAX_DEPTH 30   // heap index of a node (root 1, children 2i / 2i + 1) fits 32 bits

DH_HD inline uint64_t dh_mix64_(uint64_t z) {   // splitmix64 finaliser (synth.SplitMix)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
DH_HD inline uint64_t dh_train_key_(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    uint64_t h = dh_mix64_(seed + (tag + 1) * G);
    h = dh_mix64_(h + (a + 1) * G);
    return dh_mix64_(h + (b + 1) * G);
}
DH_HD inline double dh_u01_(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1), 53 bits
// Candidate k (0..4) draw of candidate c of node `heap` in tree `tree`: a = tree << 32 | heap, b = c * 8 + k.
DH_HD inline double dh_cand_u01_(uint64_t seed, uint32_t tree, uint32_t heap, uint32_t c, uint32_t k) {
    return dh_u01_(dh_train_key_(seed, DH_TAG_CAND, ((uint64_t)tree << 32) | heap, (uint64_t)c * 8 + k));
}
// Rect::scale_and_replace with min == max factor (types.rs:80-91, 148-159): the corner of a W x H patch's sub-rectangle,
// nx = (0.0 + u * (W - nw)) as u32 with nw = W * scale.
DH_HD inline uint32_t dh_subrect_corner_(uint32_t W, double scale, double u) {
    const double nw = (double)W * scale;
    return (uint32_t)(0.0 + u * ((double)W - nw));
}
// Threshold gen_range(-256, 256) (houghforest.rs:230-234).
DH_HD inline double dh_cand_threshold_(double u) { return -256.0 + u * 512.0; }

// ------------------------------------------------------------------ validation and geometry
int dh_train_validate_(const dh_train_params *p);
// iterate_subimage (types.rs:352-384): window centres x = lw + i * step < w - (W - lw), y likewise.
struct TrainGeom {
    uint32_t lw = 0, lh = 0, nx = 0, ny = 0;   // first centre, windows across / down
    uint32_t rw = 0, rh = 0;                   // the one split-rectangle size trunc(W * s) x trunc(H * s)
    uint32_t bw = 0, bh = 0;                   // rectangle-sum image of a sample: (W - rw + 1) x (H - rh + 1), 0 x 0 for empty rectangles
};
int dh_train_geom_(const dh_train_params &p, int w, int h, TrainGeom &g);   // DH_ESIZE for frames smaller than the patch
// Truth a forest can hold: every rot_deg of the n frames passes dh_rot_vote_ok_ (widened to f64, as the pool stores it);
// otherwise DH_EINVAL before anything is uploaded (the fit's forest would fail dh_forest_build_ after all the work).
int dh_train_check_rotations_(const float *rot_deg, int n);
// Frames per upload chunk for frames of w x h (a chunk's frames, masks and summed-area tables stay below ~256 MB).
int dh_train_chunk_frames_(int w, int h);

// ------------------------------------------------------------------ tree growing (host half)
// Best split of a node as the device's k_train_best writes it.
struct TrainBest {
    int32_t cand;        // winning candidate, -1 = no candidate leaves both sides non-empty
    uint16_t r1[4], r2[4];
    int32_t pad;
    double threshold, score;
};
static_assert(sizeof(TrainBest) == 40, "TrainBest is shared with k_train.hip");
// A node of the level being grown: its samples are idx[begin, end) in subset-draw order.
struct TrainNode {
    uint32_t tree, heap, begin, end;
};
struct TrainLevelStat {
    uint32_t nodes = 0, leaves = 0;
    float ms = 0.f;
};

class TrainGrower {
  public:
    // lab / off / rot: host copy of the pool (label, f32 offset x3, f64 rotation x3 per sample).
    TrainGrower(const dh_train_params &p, const uint8_t *lab, const float *off, const double *rot, size_t pool);
    // Root level: tree t's subset_per_tree draws idx = mulhi64(key(seed, SUBSET, t, i), pool).
    void roots(std::vector<uint32_t> &idx, std::vector<TrainNode> &level) const;
    // early_stop (houghforest.rs:302-310) for every node of `level` at `depth`: leaves are recorded (comp_leaf_data), the
    // nodes to split are returned in order.
    void stop_rules(uint32_t depth, const std::vector<uint32_t> &idx, const std::vector<TrainNode> &level,
                    std::vector<TrainNode> &split);
    // best[i] / side bytes (1 = Binar::One) of split[i]'s samples: nodes without a valid candidate become leaves, the
    // others record their split and hand two children (zero side, then one side, both stable) to the next level.
    void apply(const std::vector<uint32_t> &idx, const std::vector<TrainNode> &split, const TrainBest *best,
               const uint8_t *side, std::vector<uint32_t> &next_idx, std::vector<TrainNode> &next);
    // Trees breadth-first, one after the other, leaves in the same order; validated by dh_forest_build_.
    int assemble(dh_forest **out) const;
    std::vector<TrainLevelStat> stats;

  private:
    struct Item {
        uint32_t heap;
        bool leaf;
        dh_node node;                       // split: rectangles and threshold (children filled by assemble)
        std::vector<uint32_t> positives;    // leaf: its positive samples in node order
        double prob;
    };
    void leaf(uint32_t depth, const TrainNode &n, const std::vector<uint32_t> &idx);
    TrainLevelStat &level_stat(uint32_t depth);
    const dh_train_params p_;
    const uint8_t *lab_;
    const float *off_;
    const double *rot_;
    size_t pool_;
    std::vector<std::vector<Item>> items_;   // per tree, in creation order
};
