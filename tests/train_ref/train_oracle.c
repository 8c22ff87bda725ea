/* train_oracle.c -- sequential C restatement of the trainer contract, test infrastructure only:
 * built with gcc at test time and loaded through ctypes by tests/test_train_*.py.  It shares no code with the library.
 *
 * Pinned by the reference: sample extraction (prediction.rs:145-234, types.rs:352-384, img_to_space_coord :432-445),
 * features (houghforest.rs:227-246, types.rs:80-159), binarize / average_value_in_rect (houghforest.rs:185-193,
 * types.rs:317-339), impurity with the two-pass estimate_mean_cov (houghforest.rs:250-295, meancov_estimation.rs:359-378),
 * early_stop (:302-310), comp_leaf_data (:204-225).  Defined by this project (parity unpinned): the keyed draws, root
 * depth 0, the candidate / tie rules, stable partitions, breadth-first numbering of every tree.
 *
 * Patches are kept whole; rectangle sums come from a per-sample u64 summed-area table (the library uses u32 sums taken
 * from the frame's table modulo 2^32).  glibc log / exp.  Build with -O2 -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint32_t stepwidth, W, H, max_depth, n_trees, subset;
    double scale;
    uint32_t F, min_subset;
    double steep;
    uint64_t seed;
} TOParams; /* = dh_train_params */

typedef struct {
    uint16_t r1[4], r2[4];
    double threshold;
    int32_t child_zero, child_one;
} TONode; /* = dh_node */

static uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
uint64_t to_key(uint64_t seed, uint64_t tag, uint64_t a, uint64_t b) {
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    uint64_t h = mix64(seed + (tag + 1) * G);
    h = mix64(h + (a + 1) * G);
    return mix64(h + (b + 1) * G);
}
static double u01(uint64_t u) { return (double)(u >> 11) * (1.0 / 9007199254740992.0); }

/* ---- pool ---- */
static uint64_t g_frames;
static size_t g_n, g_cap;
static uint32_t g_W, g_H;
static uint64_t *g_sat;   /* [n][(H+1)(W+1)] */
static uint8_t *g_lab;
static float *g_off;
static double *g_rot;

void to_reset(void) {
    free(g_sat); free(g_lab); free(g_off); free(g_rot);
    g_sat = NULL; g_lab = NULL; g_off = NULL; g_rot = NULL;
    g_frames = 0; g_n = g_cap = 0; g_W = g_H = 0;
}
size_t to_pool_size(void) { return g_n; }
void to_pool_get(uint8_t *lab, float *off, double *rot) {
    memcpy(lab, g_lab, g_n);
    memcpy(off, g_off, g_n * 12);
    memcpy(rot, g_rot, g_n * 24);
}

/* Mat3<f32>::inv (meancov_estimation.rs:344-352) */
static void inv3(const float *m, float *o) {
    float a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    float det = a * (e * i - f * h) - d * (b * i - c * h) + g * (b * f - c * e);
    o[0] = (e * i - f * h) / det; o[1] = (c * h - b * i) / det; o[2] = (b * f - c * e) / det;
    o[3] = (f * g - d * i) / det; o[4] = (a * i - c * g) / det; o[5] = (c * d - a * f) / det;
    o[6] = (d * h - e * g) / det; o[7] = (b * g - a * h) / det; o[8] = (a * e - b * d) / det;
}

typedef struct { uint64_t key; uint32_t idx; } KI;
static int ki_cmp(const void *x, const void *y) {
    const KI *a = x, *b = y;
    if (a->key != b->key) return a->key < b->key ? -1 : 1;
    return a->idx < b->idx ? -1 : (a->idx > b->idx);
}

static int push_sample(const uint16_t *img, int w, uint32_t x0, uint32_t y0, int lab, const float *off, const double *rot) {
    const uint32_t W = g_W, H = g_H;
    if (g_n == g_cap) {
        size_t nc = g_cap * 2 + 64;
        uint64_t *s = realloc(g_sat, nc * (W + 1) * (H + 1) * 8);
        if (!s) return -1;
        g_sat = s;
        uint8_t *l = realloc(g_lab, nc); if (!l) return -1; g_lab = l;
        float *o = realloc(g_off, nc * 12); if (!o) return -1; g_off = o;
        double *r = realloc(g_rot, nc * 24); if (!r) return -1; g_rot = r;
        g_cap = nc;
    }
    uint64_t *S = g_sat + g_n * (W + 1) * (H + 1);
    for (uint32_t x = 0; x <= W; ++x) S[x] = 0;
    for (uint32_t y = 1; y <= H; ++y) {
        uint64_t row = 0;
        S[y * (W + 1)] = 0;
        for (uint32_t x = 1; x <= W; ++x) {
            row += img[(size_t)(y0 + y - 1) * w + x0 + x - 1];
            S[y * (W + 1) + x] = S[(y - 1) * (W + 1) + x] + row;
        }
    }
    g_lab[g_n] = (uint8_t)lab;
    for (int k = 0; k < 3; ++k) { g_off[g_n * 3 + k] = off[k]; g_rot[g_n * 3 + k] = rot[k]; }
    g_n++;
    return 0;
}

/* learn's extraction loop (prediction.rs:164-215) for n frames.  Returns 0, -1 (memory), -5 (frame smaller than patch). */
int to_add(const TOParams *p, const uint16_t *frames, const uint8_t *masks, int n, int w, int h, const float *K, const float *pos3d,
           const float *rot_deg) {
    const uint32_t W = p->W, H = p->H;
    if ((uint32_t)w < W || (uint32_t)h < H) return -5;
    if (g_n && (g_W != W || g_H != H)) return -1;
    g_W = W; g_H = H;
    const uint32_t lw = W / 2, rw = W - lw, lh = H / 2, rh = H - lh;
    size_t maxwin = ((size_t)w / p->stepwidth + 2) * ((size_t)h / p->stepwidth + 2);
    KI *neg = malloc(maxwin * sizeof(KI)), *pos = malloc(maxwin * sizeof(KI));
    if (!neg || !pos) { free(neg); free(pos); return -1; }
    for (int f = 0; f < n; ++f) {
        const uint16_t *img = frames + (size_t)f * w * h;
        const uint8_t *mask = masks + (size_t)f * w * h;
        const uint64_t frame = g_frames + (uint64_t)f;
        size_t nn = 0, np = 0;
        uint32_t nx = 0;
        for (uint32_t x = lw; x < (uint32_t)w - rw; x += p->stepwidth) nx++;
        uint32_t iy = 0;
        for (uint32_t y = lh; y < (uint32_t)h - rh; y += p->stepwidth, ++iy) {
            uint32_t ix = 0;
            for (uint32_t x = lw; x < (uint32_t)w - rw; x += p->stepwidth, ++ix) {
                uint64_t sum = 0;   /* average_value_in_rect(Rect(0, 0, W, H)) > 0 */
                for (uint32_t yy = 0; yy < H; ++yy)
                    for (uint32_t xx = 0; xx < W; ++xx) sum += img[(size_t)(y - lh + yy) * w + x - lw + xx];
                if (!((double)sum / (double)((uint64_t)W * H) > 0.0)) continue;
                const uint32_t i = iy * nx + ix;
                KI e = {to_key(p->seed, 1, frame, i), i};
                if (mask[(size_t)y * w + x]) pos[np++] = e; else neg[nn++] = e;
            }
        }
        qsort(neg, nn, sizeof(KI), ki_cmp);
        qsort(pos, np, sizeof(KI), ki_cmp);
        float kinv[9];
        inv3(K + (size_t)f * 9, kinv);
        for (int cls = 0; cls < 2; ++cls) {
            KI *list = cls ? pos : neg;
            size_t cnt = cls ? np : nn;
            for (size_t j = 0; j < cnt && j < 20; ++j) {
                const uint32_t x = lw + (list[j].idx % nx) * p->stepwidth, y = lh + (list[j].idx / nx) * p->stepwidth;
                float off[3] = {0, 0, 0};
                double rot[3] = {0, 0, 0};
                if (cls) {
                    const float v[3] = {(float)x, (float)y, 1.0f};
                    float r[3];
                    for (int jj = 0; jj < 3; ++jj) {
                        float t = v[0] * kinv[jj * 3];
                        t = t + v[1] * kinv[jj * 3 + 1];
                        t = t + v[2] * kinv[jj * 3 + 2];
                        r[jj] = t;
                    }
                    const float c = (float)img[(size_t)y * w + x] / r[2];
                    for (int k = 0; k < 3; ++k) {
                        off[k] = r[k] * c - pos3d[(size_t)f * 3 + k];
                        rot[k] = (double)rot_deg[(size_t)f * 3 + k];
                    }
                }
                if (push_sample(img, w, x - lw, y - lh, cls, off, rot)) { free(neg); free(pos); return -1; }
            }
        }
    }
    g_frames += (uint64_t)n;
    free(neg); free(pos);
    return 0;
}

/* ---- fit ---- */
typedef struct { uint32_t x1, y1, x2, y2; double th; } Cand;
static uint32_t corner(uint32_t W, double scale, double u) {
    double nw = (double)W * scale;
    return (uint32_t)(0.0 + u * ((double)W - nw));
}
static Cand make_cand(const TOParams *p, uint32_t tree, uint32_t heap, uint32_t c) {
    const uint64_t a = ((uint64_t)tree << 32) | heap;
    Cand k;
    k.x1 = corner(p->W, p->scale, u01(to_key(p->seed, 3, a, (uint64_t)c * 8 + 0)));
    k.y1 = corner(p->H, p->scale, u01(to_key(p->seed, 3, a, (uint64_t)c * 8 + 1)));
    k.x2 = corner(p->W, p->scale, u01(to_key(p->seed, 3, a, (uint64_t)c * 8 + 2)));
    k.y2 = corner(p->H, p->scale, u01(to_key(p->seed, 3, a, (uint64_t)c * 8 + 3)));
    k.th = -256.0 + u01(to_key(p->seed, 3, a, (uint64_t)c * 8 + 4)) * 512.0;
    return k;
}
static uint32_t g_rw, g_rh;
static double avg_rect(uint32_t s, uint32_t x, uint32_t y) {   /* average_value_in_rect, count 0 -> 0.0 */
    const uint64_t count = (uint64_t)g_rw * g_rh;
    if (count == 0) return 0.0;
    const uint64_t *S = g_sat + (size_t)s * (g_W + 1) * (g_H + 1);
    const uint32_t st = g_W + 1;
    const uint64_t sum = S[(y + g_rh) * st + x + g_rw] - S[y * st + x + g_rw] - S[(y + g_rh) * st + x] + S[y * st + x];
    return (double)sum / (double)count;
}
static int binarize(const Cand *k, uint32_t s) { return avg_rect(s, k->x1, k->y1) - avg_rect(s, k->x2, k->y2) > k->th; }

static double ln0(double x) { return x == 0.0 ? 0.0 : log(x); }
static double entropy(const uint32_t *set, size_t n) {
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) pos += g_lab[set[i]];
    const double prob = (double)pos / (double)n;
    return prob * ln0(prob) + (1.0 - prob) * ln0(1.0 - prob);
}
static double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[1][0] * (m[0][1] * m[2][2] - m[0][2] * m[2][1]) +
           m[2][0] * (m[0][1] * m[1][2] - m[0][2] * m[1][1]);
}
/* estimate_mean_cov (meancov_estimation.rs:359-378) of the positives' vectors, which = 0 offsets (f32 -> f64), 1 rotations */
static void mean_cov(const uint32_t *set, size_t n, int which, double cov[3][3]) {
    double mean[3];
    size_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!g_lab[set[i]]) continue;
        for (int k = 0; k < 3; ++k) {
            const double v = which ? g_rot[set[i] * 3 + k] : (double)g_off[set[i] * 3 + k];
            mean[k] = m == 0 ? v : mean[k] + v;
        }
        m++;
    }
    for (int k = 0; k < 3; ++k) mean[k] = mean[k] / (double)m;
    size_t q = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!g_lab[set[i]]) continue;
        double d[3];
        for (int k = 0; k < 3; ++k) d[k] = (which ? g_rot[set[i] * 3 + k] : (double)g_off[set[i] * 3 + k]) - mean[k];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) cov[a][b] = q == 0 ? d[a] * d[b] : cov[a][b] + d[a] * d[b];
        q++;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) cov[a][b] = cov[a][b] / (double)(m - 1);
}
static uint64_t g_neg;
static double regression_log(const uint32_t *set, size_t n) {
    size_t pos = 0;
    for (size_t i = 0; i < n; ++i) pos += g_lab[set[i]];
    if (pos == 0) return 0.0;
    double c1[3][3], c2[3][3];
    mean_cov(set, n, 0, c1);
    mean_cov(set, n, 1, c2);
    const double x = det3(c1) + det3(c2);
    if (x > 0.0) return log(x);
    if (x < -0.001) g_neg++;
    return 0.0;
}
double to_impurity(const uint32_t *l, size_t nl, const uint32_t *r, size_t nr, uint32_t depth, double steep) {
    const size_t count = nl + nr;
    const double lf = (double)nl / (double)count, rf = (double)nr / (double)count;
    const double imp = -(lf * entropy(l, nl) + rf * entropy(r, nr));
    const double reg = lf * regression_log(l, nl) + rf * regression_log(r, nr);
    const double f = exp(-((double)depth / steep));
    return imp + (1.0 - f) * reg;
}

typedef struct { uint32_t heap; int32_t parent; int side; uint32_t *set; size_t n; } QE;

/* Fit; output arrays sized by the caller (nodes / leaves <= n_trees * (2 * subset + 1), votes <= n_trees * subset).
 * counts[0..2] = nodes, leaves, votes.  *margin = smallest gap between a split node's best and second-best distinct
 * score (+inf if none).  Returns 0, -1 (memory), -6 (empty pool). */
int to_fit(const TOParams *p, int32_t *roots, TONode *nodes, double *prob, uint32_t *ob, uint32_t *rb, float *offs, double *rots,
           uint32_t *counts, double *margin, uint64_t *neg_det) {
    if (g_n == 0) return -6;
    g_rw = (uint32_t)((double)p->W * p->scale);
    g_rh = (uint32_t)((double)p->H * p->scale);
    g_neg = 0;
    *margin = INFINITY;
    uint32_t nn = 0, nl = 0, nv = 0;
    ob[0] = rb[0] = 0;
    double *scores = malloc(sizeof(double) * p->F);
    uint32_t *l = malloc(sizeof(uint32_t) * (p->subset + 1)), *r = malloc(sizeof(uint32_t) * (p->subset + 1));
    QE *queue = malloc(sizeof(QE) * (2 * (size_t)p->subset + 3));
    if (!scores || !l || !r || !queue) return -1;
    for (uint32_t t = 0; t < p->n_trees; ++t) {
        size_t qh = 0, qt = 0;
        uint32_t *root = malloc(sizeof(uint32_t) * (p->subset + 1));
        for (uint32_t i = 0; i < p->subset; ++i)
            root[i] = (uint32_t)(((unsigned __int128)to_key(p->seed, 2, t, i) * g_n) >> 64);
        queue[qt++] = (QE){1, -1, 0, root, p->subset};
        while (qh < qt) {
            QE e = queue[qh++];
            const uint32_t depth = 31 - __builtin_clz(e.heap);
            size_t pos = 0;
            for (size_t i = 0; i < e.n; ++i) pos += g_lab[e.set[i]];
            int best = -1;
            double bs = INFINITY, second = INFINITY;
            if (pos && depth < p->max_depth && e.n >= p->min_subset) {
                for (uint32_t c = 0; c < p->F; ++c) {
                    const Cand k = make_cand(p, t, e.heap, c);
                    size_t a = 0, b = 0;
                    for (size_t i = 0; i < e.n; ++i) {
                        if (binarize(&k, e.set[i])) r[b++] = e.set[i]; else l[a++] = e.set[i];
                    }
                    if (a == 0 || b == 0) continue;
                    const double sc = to_impurity(l, a, r, b, depth, p->steep);
                    if (best < 0 || sc < bs) { if (best >= 0 && bs < second) second = bs; bs = sc; best = (int)c; }
                    else if (sc > bs && sc < second) second = sc;
                }
            }
            int32_t ref;
            if (best < 0) {
                ref = ~(int32_t)nl;
                prob[nl] = e.n ? (double)pos / (double)e.n : 0.0;
                for (size_t i = 0; i < e.n; ++i) {
                    if (!g_lab[e.set[i]]) continue;
                    for (int k = 0; k < 3; ++k) { offs[(size_t)nv * 3 + k] = g_off[e.set[i] * 3 + k]; rots[(size_t)nv * 3 + k] = g_rot[e.set[i] * 3 + k]; }
                    nv++;
                }
                nl++;
                ob[nl] = rb[nl] = nv;
                free(e.set);
            } else {
                if (second - bs < *margin) *margin = second - bs;
                const Cand k = make_cand(p, t, e.heap, (uint32_t)best);
                ref = (int32_t)nn;
                TONode *nd = &nodes[nn++];
                nd->r1[0] = k.x1; nd->r1[1] = k.y1; nd->r1[2] = k.x1 + g_rw; nd->r1[3] = k.y1 + g_rh;
                nd->r2[0] = k.x2; nd->r2[1] = k.y2; nd->r2[2] = k.x2 + g_rw; nd->r2[3] = k.y2 + g_rh;
                nd->threshold = k.th;
                nd->child_zero = nd->child_one = 0;
                uint32_t *z = malloc(sizeof(uint32_t) * (e.n + 1)), *o = malloc(sizeof(uint32_t) * (e.n + 1));
                size_t a = 0, b = 0;
                for (size_t i = 0; i < e.n; ++i) {
                    if (binarize(&k, e.set[i])) o[b++] = e.set[i]; else z[a++] = e.set[i];
                }
                free(e.set);
                queue[qt++] = (QE){2 * e.heap, ref, 0, z, a};
                queue[qt++] = (QE){2 * e.heap + 1, ref, 1, o, b};
            }
            if (e.parent < 0) roots[t] = ref;
            else if (e.side == 0) nodes[e.parent].child_zero = ref;
            else nodes[e.parent].child_one = ref;
        }
    }
    free(scores); free(l); free(r); free(queue);
    counts[0] = nn; counts[1] = nl; counts[2] = nv;
    *neg_det = g_neg;
    return 0;
}

/* estimate_mean_cov + det of an arbitrary 3-vector list (KAT of meancov_estimation.rs:461-490). */
double to_cov_det(const double *v, size_t n, double *cov_out) {
    double mean[3], cov[3][3];
    for (int k = 0; k < 3; ++k) mean[k] = v[k];
    for (size_t i = 1; i < n; ++i)
        for (int k = 0; k < 3; ++k) mean[k] = mean[k] + v[i * 3 + k];
    for (int k = 0; k < 3; ++k) mean[k] = mean[k] / (double)n;
    for (size_t i = 0; i < n; ++i) {
        double d[3];
        for (int k = 0; k < 3; ++k) d[k] = v[i * 3 + k] - mean[k];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) cov[a][b] = i == 0 ? d[a] * d[b] : cov[a][b] + d[a] * d[b];
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { cov[a][b] = cov[a][b] / (double)(n - 1); if (cov_out) cov_out[a * 3 + b] = cov[a][b]; }
    return det3(cov);
}

/* Rect::scale_and_replace for a rectangle at (x, y) of w x h (types.rs:80-91): out = x0, y0, x1, y1. */
void to_scale_and_replace(uint32_t x, uint32_t y, uint32_t w, uint32_t h, double scale, double rx, double ry, uint32_t out[4]) {
    if (scale > 1.0) { out[0] = x; out[1] = y; out[2] = x + w; out[3] = y + h; return; }
    const double nw = (double)w * scale, nh = (double)h * scale;
    const double nx = (double)x + rx * ((double)w - nw), ny = (double)y + ry * ((double)h - nh);
    out[0] = (uint32_t)nx; out[1] = (uint32_t)ny; out[2] = (uint32_t)nx + (uint32_t)nw; out[3] = (uint32_t)ny + (uint32_t)nh;
}
uint64_t to_neg_det(void) { return g_neg; }

/* Replace the pool's truth by caller arrays (impurity KATs: no patches, no fit). */
int to_pool_set(size_t n, const uint8_t *lab, const float *off, const double *rot) {
    to_reset();
    g_lab = malloc(n + 1); g_off = malloc(n * 12 + 12); g_rot = malloc(n * 24 + 24);
    if (!g_lab || !g_off || !g_rot) return -1;
    memcpy(g_lab, lab, n); memcpy(g_off, off, n * 12); memcpy(g_rot, rot, n * 24);
    g_n = g_cap = n;
    g_neg = 0;
    return 0;
}

/* ---- verifier ----
 * Walks trees [tree_begin, tree_end) of a given forest over the oracle's pool: rebuilds each node's sample multiset (the
 * subset draws, partitioned by the forest's own splits), regenerates the node's candidates and checks that
 *   - early_stop holds: a node the rules stop is a leaf, one they do not stop is split unless no candidate is valid;
 *   - a split is bitwise one of the node's valid candidates and its score is <= min + 1e-12 * max(1, |min|);
 *   - a leaf is bitwise comp_leaf_data (prob, offsets, rotations, order; a NaN vote matches any NaN);
 * and accumulates the negative-det count over every valid candidate of every searched node (comparable with the
 * trainer's count when all trees are walked).  *gap = smallest best / second-best distinct score gap over split nodes;
 * visited[0..1] = split nodes / leaves reached.  Returns 0, or -1 with a message in msg. */
#include <stdio.h>
typedef struct { int32_t ref; uint32_t heap; uint32_t *set; size_t n; } VE;
/* A leaf vote against its sample: bitwise, except that a NaN matches any NaN (NaN bit patterns are not part of the
 * contract: the device and this oracle need not produce the same NaN from 0 / 0 or inf * 0). */
static int same_vote(const float *o, const float *so, const double *r, const double *sr) {
    for (int k = 0; k < 3; ++k) {
        if (isnan(o[k]) ? !isnan(so[k]) : memcmp(&o[k], &so[k], 4) != 0) return 0;
        if (isnan(r[k]) ? !isnan(sr[k]) : memcmp(&r[k], &sr[k], 8) != 0) return 0;
    }
    return 1;
}
int to_verify(const TOParams *p, const int32_t *roots, const TONode *nodes, uint32_t n_nodes, const double *prob, const uint32_t *ob,
              const uint32_t *rb, uint32_t n_leaves, const float *offs, const double *rots, uint32_t tree_begin, uint32_t tree_end,
              double *gap, uint64_t *neg_det, uint32_t *visited, char *msg, size_t msgn) {
    if (g_n == 0) { snprintf(msg, msgn, "empty pool"); return -1; }
    g_rw = (uint32_t)((double)p->W * p->scale);
    g_rh = (uint32_t)((double)p->H * p->scale);
    g_neg = 0;
    *gap = INFINITY;
    visited[0] = visited[1] = 0;
    int rc = 0;
    double *scores = malloc(sizeof(double) * p->F);
    uint8_t *valid = malloc(p->F);
    uint32_t *l = malloc(sizeof(uint32_t) * (p->subset + 1)), *r = malloc(sizeof(uint32_t) * (p->subset + 1));
    VE *stack = malloc(sizeof(VE) * (2 * (size_t)p->subset + 64));
    if (!scores || !valid || !l || !r || !stack) { snprintf(msg, msgn, "out of memory"); return -1; }
    size_t sp = 0;
    for (uint32_t t = tree_begin; t < tree_end && rc == 0; ++t) {
        uint32_t *root = malloc(sizeof(uint32_t) * (p->subset + 1));
        for (uint32_t i = 0; i < p->subset; ++i) root[i] = (uint32_t)(((unsigned __int128)to_key(p->seed, 2, t, i) * g_n) >> 64);
        stack[sp++] = (VE){roots[t], 1, root, p->subset};
        while (sp && rc == 0) {
            VE e = stack[--sp];
            const uint32_t depth = 31 - __builtin_clz(e.heap);
            size_t pos = 0;
            for (size_t i = 0; i < e.n; ++i) pos += g_lab[e.set[i]];
            const int stop = !pos || depth >= p->max_depth || e.n < p->min_subset;
            double mn = INFINITY, second = INFINITY;
            int any = 0;
            if (!stop) {
                for (uint32_t c = 0; c < p->F; ++c) {
                    const Cand k = make_cand(p, t, e.heap, c);
                    size_t a = 0, b = 0;
                    for (size_t i = 0; i < e.n; ++i) {
                        if (binarize(&k, e.set[i])) r[b++] = e.set[i]; else l[a++] = e.set[i];
                    }
                    valid[c] = a && b;
                    if (!valid[c]) continue;
                    scores[c] = to_impurity(l, a, r, b, depth, p->steep);
                    if (!any || scores[c] < mn) { if (any && mn < second) second = mn; mn = scores[c]; }
                    else if (scores[c] > mn && scores[c] < second) second = scores[c];
                    any = 1;
                }
            }
            if (stop || !any) {
                if (e.ref >= 0) {
                    rc = -1;
                    snprintf(msg, msgn, "tree %u heap %u: split node %d where early_stop / no valid candidate makes a leaf", t, e.heap, e.ref);
                    break;
                }
                const uint32_t L = (uint32_t)~e.ref;
                const double want = e.n ? (double)pos / (double)e.n : 0.0;
                if (L >= n_leaves || memcmp(&prob[L], &want, 8) != 0 || ob[L + 1] - ob[L] != pos || rb[L + 1] - rb[L] != pos) {
                    rc = -1;
                    snprintf(msg, msgn, "tree %u heap %u: leaf %u is not comp_leaf_data (prob %.17g want %.17g, %u votes want %zu)", t,
                             e.heap, L, L < n_leaves ? prob[L] : -1.0, want, L < n_leaves ? ob[L + 1] - ob[L] : 0, pos);
                    break;
                }
                size_t v = 0;
                for (size_t i = 0; i < e.n && rc == 0; ++i) {
                    const uint32_t s = e.set[i];
                    if (!g_lab[s]) continue;
                    if (!same_vote(&offs[(size_t)(ob[L] + v) * 3], &g_off[(size_t)s * 3], &rots[(size_t)(rb[L] + v) * 3], &g_rot[(size_t)s * 3])) {
                        rc = -1;
                        snprintf(msg, msgn, "tree %u heap %u: leaf %u vote %zu differs from its positive sample %u", t, e.heap, L, v, s);
                    }
                    v++;
                }
                visited[1]++;
                free(e.set);
                continue;
            }
            if (e.ref < 0 || (uint32_t)e.ref >= n_nodes) {
                rc = -1;
                snprintf(msg, msgn, "tree %u heap %u: leaf %d where a split is required (best score %.17g)", t, e.heap, ~e.ref, mn);
                break;
            }
            const TONode *nd = &nodes[e.ref];
            int found = -1;
            for (uint32_t c = 0; c < p->F && found < 0; ++c) {
                if (!valid[c]) continue;
                const Cand k = make_cand(p, t, e.heap, c);
                const uint16_t r1[4] = {(uint16_t)k.x1, (uint16_t)k.y1, (uint16_t)(k.x1 + g_rw), (uint16_t)(k.y1 + g_rh)};
                const uint16_t r2[4] = {(uint16_t)k.x2, (uint16_t)k.y2, (uint16_t)(k.x2 + g_rw), (uint16_t)(k.y2 + g_rh)};
                if (!memcmp(r1, nd->r1, 8) && !memcmp(r2, nd->r2, 8) && !memcmp(&k.th, &nd->threshold, 8)) found = (int)c;
            }
            if (found < 0) {
                rc = -1;
                snprintf(msg, msgn, "tree %u heap %u: node %d's split is not one of its valid candidates", t, e.heap, e.ref);
                break;
            }
            const double tol = 1e-12 * (fabs(mn) > 1.0 ? fabs(mn) : 1.0);
            if (!(scores[found] <= mn + tol)) {
                rc = -1;
                snprintf(msg, msgn, "tree %u heap %u: node %d takes candidate %d scoring %.17g, the minimum is %.17g", t, e.heap, e.ref, found,
                         scores[found], mn);
                break;
            }
            if (second - mn < *gap) *gap = second - mn;
            visited[0]++;
            const Cand k = make_cand(p, t, e.heap, (uint32_t)found);
            uint32_t *z = malloc(sizeof(uint32_t) * (e.n + 1)), *o = malloc(sizeof(uint32_t) * (e.n + 1));
            size_t a = 0, b = 0;
            for (size_t i = 0; i < e.n; ++i) {
                if (binarize(&k, e.set[i])) o[b++] = e.set[i]; else z[a++] = e.set[i];
            }
            free(e.set);
            stack[sp++] = (VE){nd->child_one, 2 * e.heap + 1, o, b};
            stack[sp++] = (VE){nd->child_zero, 2 * e.heap, z, a};
        }
    }
    while (sp) free(stack[--sp].set);
    free(scores); free(valid); free(l); free(r); free(stack);
    *neg_det = g_neg;
    return rc;
}
