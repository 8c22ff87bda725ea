// train_check.cpp -- drives the host half of the trainer (depthhead_amd/csrc/dh_train.cpp: parameter validation, window
// geometry, chunk sizes, the keyed subset draws, early_stop / partition / comp_leaf_data bookkeeping and the assembly of
// the forest) under the CPU sanitizers: built by tests/test_train_host.py with g++ -fsanitize=address,undefined and once
// more with -fsanitize=thread (several growers on several threads).  Prints "train_check ok" and exits 0.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <thread>
#include <vector>

#include "../../depthhead_amd/csrc/dh_train.h"

static int g_fail = 0;
#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); ++g_fail; } \
    } while (0)

static dh_train_params base() {
    dh_train_params p{};
    p.stepwidth = 10; p.subimage_width = 80; p.subimage_height = 80; p.max_depth = 15; p.n_trees = 20;
    p.subset_per_tree = 5200; p.subrect_feature_scale = 0.3; p.features_per_node = 2000; p.min_subset_size = 20;
    p.steepness = 5.0; p.seed = 1;
    return p;
}

static void validation() {
    dh_train_params p = base();
    CHECK(dh_train_validate_(&p) == DH_OK);
    CHECK(dh_train_validate_(nullptr) == DH_EINVAL);
    for (double s : {0.0, -0.1, 1.0000001, 2.0}) { p = base(); p.subrect_feature_scale = s; CHECK(dh_train_validate_(&p) == DH_EINVAL); }
    p = base(); p.subrect_feature_scale = 1.0; CHECK(dh_train_validate_(&p) == DH_OK);
    p = base(); p.features_per_node = 0; CHECK(dh_train_validate_(&p) == DH_EINVAL);
    p = base(); p.steepness = 0.0; CHECK(dh_train_validate_(&p) == DH_EINVAL);
    p = base(); p.steepness = -1.0; CHECK(dh_train_validate_(&p) == DH_EINVAL);
    p = base(); p.max_depth = 31; CHECK(dh_train_validate_(&p) == DH_EINVAL);
    p = base(); p.subimage_width = 256; p.subimage_height = 257; CHECK(dh_train_validate_(&p) == DH_ESIZE);   // 65792 * 65535 >= 2^32
    p = base(); p.subimage_width = 256; p.subimage_height = 256; CHECK(dh_train_validate_(&p) == DH_OK);
    TrainGeom g;
    p = base();
    CHECK(dh_train_geom_(p, 79, 480, g) == DH_ESIZE);
    CHECK(dh_train_geom_(p, 640, 480, g) == DH_OK);
    CHECK(g.lw == 40 && g.nx == 56 && g.ny == 40 && g.rw == 24 && g.rh == 24 && g.bw == 57 && g.bh == 57);
    CHECK(dh_train_geom_(p, 80, 80, g) == DH_OK && g.nx == 0 && g.ny == 0);
    p.subimage_width = 81; p.subimage_height = 79; p.stepwidth = 7;
    CHECK(dh_train_geom_(p, 203, 157, g) == DH_OK);
    uint32_t nx = 0;   // iterate_subimage's loop
    for (uint32_t x = 40; x < 203u - 41u; x += 7) nx++;
    CHECK(g.nx == nx);
    for (int w : {80, 320, 640, 4096}) CHECK(dh_train_chunk_frames_(w, w) >= 1 && dh_train_chunk_frames_(w, w) <= 256);
    // the chunk boundaries the training families cross (tests/train_ref/train_families.py): 257 frames of 48 x 40 are
    // chunks of 256 + 1, 32 frames of 1280 x 960 chunks of 31 + 1
    CHECK(dh_train_chunk_frames_(48, 40) == 256);
    CHECK(dh_train_chunk_frames_(640, 480) == 124);
    CHECK(dh_train_chunk_frames_(1280, 960) == 31);
    p = base(); p.subimage_width = 198; p.subimage_height = 331; CHECK(dh_train_validate_(&p) == DH_ESIZE);   // 65 538 pixels
    // truth a forest can hold: rotation bins in [0, 120) after one wrap, -543 < deg < 540, NaN in bin 60
    for (float d : {0.f, 539.75f, -542.75f, NAN}) CHECK(dh_rot_vote_ok_(d));
    for (float d : {540.f, -543.f, INFINITY, -INFINITY, 1e30f}) CHECK(!dh_rot_vote_ok_(d));
    const float rots[6] = {10.f, -20.f, NAN, 1.f, 2.f, 3.f};
    CHECK(dh_train_check_rotations_(rots, 2) == DH_OK);
    const float bad[6] = {10.f, -20.f, 30.f, 1.f, -INFINITY, 3.f};
    CHECK(dh_train_check_rotations_(bad, 1) == DH_OK && dh_train_check_rotations_(bad, 2) == DH_EINVAL);
}

// A random pool and random device answers: the grower's bookkeeping must keep every sample, partition stably and
// assemble a forest dh_forest_build_ accepts.
static void grow(uint64_t seed) {
    dh_train_params p = base();
    p.n_trees = 4; p.subset_per_tree = 300; p.max_depth = 8; p.min_subset_size = 5; p.seed = seed;
    const size_t pool = 257;
    std::vector<uint8_t> lab(pool);
    std::vector<float> off(pool * 3);
    std::vector<double> rot(pool * 3);
    for (size_t i = 0; i < pool; ++i) {
        lab[i] = (uint8_t)(dh_train_key_(seed, 9, i, 0) & 1);
        for (int k = 0; k < 3; ++k) { off[i * 3 + k] = (float)(i % 17) - 8.f; rot[i * 3 + k] = (double)(i % 13) - 6.0; }
    }
    TrainGrower gr(p, lab.data(), off.data(), rot.data(), pool);
    std::vector<uint32_t> idx, nidx;
    std::vector<TrainNode> level, split, next;
    gr.roots(idx, level);
    CHECK(idx.size() == 1200 && level.size() == 4);
    for (uint32_t s : idx) CHECK(s < pool);
    uint32_t depth = 0;
    for (;; ++depth) {
        gr.stop_rules(depth, idx, level, split);
        if (split.empty()) break;
        std::vector<TrainBest> best(split.size());
        std::vector<uint8_t> side(idx.size(), 7);
        for (size_t i = 0; i < split.size(); ++i) {
            best[i] = TrainBest{};
            best[i].cand = (dh_train_key_(seed, 8, depth, i) % 5) == 0 ? -1 : 3;
            best[i].r1[2] = best[i].r1[3] = best[i].r2[2] = best[i].r2[3] = 24;
            for (uint32_t q = split[i].begin; q < split[i].end; ++q) side[q] = (uint8_t)(dh_train_key_(seed, 7, q, depth) & 1);
        }
        gr.apply(idx, split, best.data(), side.data(), nidx, next);
        size_t kept = 0;
        for (size_t i = 0; i < split.size(); ++i) if (best[i].cand >= 0) kept += split[i].end - split[i].begin;
        CHECK(nidx.size() == kept);
        idx.swap(nidx);
        level.swap(next);
        if (level.empty()) break;
    }
    CHECK(depth <= p.max_depth);
    dh_forest *f = nullptr;
    CHECK(gr.assemble(&f) == DH_OK);
    if (f) {
        CHECK(f->roots.size() == 4 && f->max_depth <= 8);
        CHECK(f->off_begin.back() * 3 == f->offsets.size() && f->rot_begin.back() * 3 == f->rotations.size());
        delete f;
    }
}

int main() {
    const bool light = getenv("TRAIN_CHECK_LIGHT") != nullptr;
    validation();
    for (uint64_t s = 1; s <= (light ? 4u : 40u); ++s) grow(s);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t) th.emplace_back([t] { for (int i = 0; i < 3; ++i) grow(1000 + t * 10 + i); validation(); });
    for (auto &x : th) x.join();
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("train_check ok\n");
    return 0;
}
