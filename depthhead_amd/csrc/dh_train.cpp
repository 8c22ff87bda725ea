// dh_train.cpp -- host-only half of the trainer (see dh_train.h).  Plain C++: built by hipcc into the library and by g++
// under sanitizers (tests/host/train_check.cpp).
#include "dh_train.h"

#include <algorithm>
#include <unordered_map>

// HoughLearning::new -> HoughTreeFunctions::new (houghforest.rs:143-158) and random_subrect_iterator (types.rs:106-109),
// which runs at the first node: the two together refuse a factor outside (0, 1], features == 0 and steepness <= 0.
int dh_train_validate_(const dh_train_params *p) {
    if (!p) return dh_fail_(DH_EINVAL, "dh_trainer_create: NULL parameters");
    const double s = p->subrect_feature_scale;
    if (!(s > 0.0 && s <= 1.0)) return dh_fail_(DH_EINVAL, "subrect_feature_scale %g outside (0, 1]", s);
    if (p->features_per_node == 0) return dh_fail_(DH_EINVAL, "feature_number_per_node must be > 0");
    if (!(p->steepness > 0.0)) return dh_fail_(DH_EINVAL, "steepness_weighting %g must be > 0", p->steepness);
    if (p->n_trees == 0) return dh_fail_(DH_EINVAL, "num_of_trees must be > 0");
    if (p->stepwidth == 0) return dh_fail_(DH_EINVAL, "stepwidth must be > 0");   // iterate_subimage would never advance
    if (p->subimage_width == 0 || p->subimage_height == 0) return dh_fail_(DH_EINVAL, "empty patch");
    if (p->subimage_width > 4096 || p->subimage_height > 4096) return dh_fail_(DH_ESIZE, "patch larger than 4096");
    if (p->max_depth > DH_TRAIN_MAX_DEPTH) return dh_fail_(DH_EINVAL, "max_depth %u above %d", p->max_depth, DH_TRAIN_MAX_DEPTH);
    // rectangle and patch sums are taken modulo 2^32: exact while W * H * 65535 < 2^32 (the bound of dh_predictor_create)
    if ((uint64_t)p->subimage_width * p->subimage_height * 65535ull >= (1ull << 32))
        return dh_fail_(DH_ESIZE, "patch area %ux%u too large for u32 rectangle sums", p->subimage_width, p->subimage_height);
    return DH_OK;
}

int dh_train_geom_(const dh_train_params &p, int w, int h, TrainGeom &g) {
    const uint32_t W = p.subimage_width, H = p.subimage_height;
    if (w <= 0 || h <= 0) return dh_fail_(DH_EINVAL, "frame size %dx%d", w, h);
    if ((uint32_t)w < W || (uint32_t)h < H)
        return dh_fail_(DH_ESIZE, "frame %dx%d smaller than the %ux%u patch", w, h, W, H);
    g.lw = W / 2; g.lh = H / 2;                                           // types.rs:366-369
    const uint32_t rw_ = W - g.lw, rh_ = H - g.lh;
    g.nx = (uint32_t)w - rw_ > g.lw ? ((uint32_t)w - rw_ - g.lw + p.stepwidth - 1) / p.stepwidth : 0;   // x < w - right_w
    g.ny = (uint32_t)h - rh_ > g.lh ? ((uint32_t)h - rh_ - g.lh + p.stepwidth - 1) / p.stepwidth : 0;
    g.rw = (uint32_t)((double)W * p.subrect_feature_scale);             // nw as u32 (types.rs:90)
    g.rh = (uint32_t)((double)H * p.subrect_feature_scale);
    g.bw = g.rw && g.rh ? W - g.rw + 1 : 0;
    g.bh = g.rw && g.rh ? H - g.rh + 1 : 0;
    return DH_OK;
}

int dh_train_check_rotations_(const float *rot_deg, int n) {
    for (size_t i = 0; i < (size_t)n * 3; ++i)
        if (!dh_rot_vote_ok_((double)rot_deg[i]))
            return dh_fail_(DH_EINVAL, "frame %zu: rot_deg[%zu] = %g degrees is outside what a forest can hold (-543 < deg < 540 or NaN)",
                            i / 3, i % 3, (double)rot_deg[i]);
    return DH_OK;
}

int dh_train_chunk_frames_(int w, int h) {
    const size_t per = (size_t)w * h * 3 + (size_t)(w + 1) * (h + 1) * 4;   // frame + mask + summed-area table
    return (int)std::max<size_t>(1, std::min<size_t>(256, (256u << 20) / per));
}

TrainGrower::TrainGrower(const dh_train_params &p, const uint8_t *lab, const float *off, const double *rot, size_t pool)
    : p_(p), lab_(lab), off_(off), rot_(rot), pool_(pool), items_(p.n_trees) {}

TrainLevelStat &TrainGrower::level_stat(uint32_t depth) {
    if (stats.size() <= depth) stats.resize(depth + 1);
    return stats[depth];
}

void TrainGrower::roots(std::vector<uint32_t> &idx, std::vector<TrainNode> &level) const {
    const uint32_t S = p_.subset_per_tree;
    idx.resize((size_t)p_.n_trees * S);
    level.clear();
    for (uint32_t t = 0; t < p_.n_trees; ++t) {
        for (uint32_t i = 0; i < S; ++i) {
            const uint64_t k = dh_train_key_(p_.seed, DH_TAG_SUBSET, t, i);
            idx[(size_t)t * S + i] = (uint32_t)(((unsigned __int128)k * pool_) >> 64);
        }
        level.push_back({t, 1u, t * S, (t + 1) * S});
    }
}

// comp_leaf_data (houghforest.rs:204-225): prob = positives / len, every positive's offset and rotation in node order.
void TrainGrower::leaf(uint32_t depth, const TrainNode &n, const std::vector<uint32_t> &idx) {
    Item it{n.heap, true, dh_node{}, {}, 0.0};
    for (uint32_t q = n.begin; q < n.end; ++q)
        if (lab_[idx[q]]) it.positives.push_back(idx[q]);
    it.prob = n.end > n.begin ? (double)it.positives.size() / (double)(n.end - n.begin) : 0.0;
    items_[n.tree].push_back(std::move(it));
    level_stat(depth).leaves++;
}

void TrainGrower::stop_rules(uint32_t depth, const std::vector<uint32_t> &idx, const std::vector<TrainNode> &level,
                             std::vector<TrainNode> &split) {
    split.clear();
    level_stat(depth);
    for (const TrainNode &n : level) {
        bool any = false;
        for (uint32_t q = n.begin; q < n.end && !any; ++q) any = lab_[idx[q]] != 0;
        if (!any || depth >= p_.max_depth || n.end - n.begin < p_.min_subset_size) leaf(depth, n, idx);   // :303-308
        else split.push_back(n);
    }
}

void TrainGrower::apply(const std::vector<uint32_t> &idx, const std::vector<TrainNode> &split, const TrainBest *best,
                        const uint8_t *side, std::vector<uint32_t> &next_idx, std::vector<TrainNode> &next) {
    next_idx.clear();
    next.clear();
    for (size_t i = 0; i < split.size(); ++i) {
        const TrainNode &n = split[i];
        const uint32_t depth = 31 - __builtin_clz(n.heap);
        if (best[i].cand < 0) { leaf(depth, n, idx); continue; }
        Item it{n.heap, false, dh_node{}, {}, 0.0};
        std::copy(best[i].r1, best[i].r1 + 4, it.node.r1);
        std::copy(best[i].r2, best[i].r2 + 4, it.node.r2);
        it.node.threshold = best[i].threshold;
        items_[n.tree].push_back(std::move(it));
        level_stat(depth).nodes++;
        for (int s = 0; s < 2; ++s) {   // heap 2i: Binar::Zero, 2i + 1: Binar::One
            const uint32_t b = (uint32_t)next_idx.size();
            for (uint32_t q = n.begin; q < n.end; ++q)
                if (side[q] == s) next_idx.push_back(idx[q]);
            next.push_back({n.tree, 2 * n.heap + s, b, (uint32_t)next_idx.size()});
        }
    }
}

int TrainGrower::assemble(dh_forest **out) const {
    std::vector<int32_t> roots;
    std::vector<dh_node> nodes;
    std::vector<double> prob;
    std::vector<uint32_t> ob{0}, rb{0};
    std::vector<float> offs;
    std::vector<double> rots;
    for (uint32_t t = 0; t < p_.n_trees; ++t) {
        std::unordered_map<uint32_t, const Item *> by_heap;
        for (const Item &it : items_[t]) by_heap[it.heap] = &it;
        // breadth-first: split nodes get consecutive node indices, leaves consecutive leaf indices; a parent's child
        // links are patched when the child is numbered
        struct Q { uint32_t heap; int32_t parent; int side; };
        std::vector<Q> queue{{1u, -1, 0}};
        for (size_t qi = 0; qi < queue.size(); ++qi) {
            const Q q = queue[qi];
            auto f = by_heap.find(q.heap);
            if (f == by_heap.end()) return dh_fail_(DH_EINVAL, "tree %u: node %u was never grown", t, q.heap);
            const Item &it = *f->second;
            int32_t ref;
            if (it.leaf) {
                ref = ~(int32_t)prob.size();
                prob.push_back(it.prob);
                for (uint32_t s : it.positives) {
                    offs.insert(offs.end(), off_ + (size_t)s * 3, off_ + (size_t)s * 3 + 3);
                    rots.insert(rots.end(), rot_ + (size_t)s * 3, rot_ + (size_t)s * 3 + 3);
                }
                ob.push_back((uint32_t)(offs.size() / 3));
                rb.push_back((uint32_t)(rots.size() / 3));
            } else {
                ref = (int32_t)nodes.size();
                nodes.push_back(it.node);
                queue.push_back({2 * q.heap, ref, 0});
                queue.push_back({2 * q.heap + 1, ref, 1});
            }
            if (q.parent < 0) roots.push_back(ref);
            else if (q.side == 0) nodes[q.parent].child_zero = ref;
            else nodes[q.parent].child_one = ref;
        }
    }
    dh_forest_desc d{};
    d.n_trees = (uint32_t)roots.size();
    d.roots = roots.data();
    d.n_nodes = (uint32_t)nodes.size();
    d.nodes = nodes.data();
    d.n_leaves = (uint32_t)prob.size();
    d.leaf_prob = prob.data();
    d.off_begin = ob.data();
    d.rot_begin = rb.data();
    d.offsets = offs.data();
    d.rotations = rots.data();
    return dh_forest_build_(&d, out);
}
