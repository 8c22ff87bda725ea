// The host side of a subject set that is plain functions (depthhead_amd/csrc/dh_fit.h), for
// tests/test_subjects_host.py: dh_subjects_corner_lists, each vertex's incident corners in ascending (triangle, corner) order --
// against a search through the triangles, on a tetrahedron, a fan whose hub lies in 300 triangles, a triangle that names a vertex
// twice, a vertex no triangle names, seeded random meshes, and the refusal of an index >= n; dh_subjects_first_zero_normal, the
// base-mesh refusal; and dh_subjects_radius_bound against the deformed points themselves at the corners of the coefficient cube.
// A stand-alone program: it prints what it checked and exits 0, or says what differed and exits 1.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "dh_fit.h"

static int failures = 0;
static long checks = 0;
#define EXPECT(cond, ...)                                                                                                       \
    do {                                                                                                                        \
        ++checks;                                                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: " #cond ": ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++failures; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % below);
}

// begin / corners of `tris` against the definition: the corners q = t * 3 + c with tris[q] == v, ascending
static void check_lists(const char *what, const std::vector<uint32_t> &tris, uint32_t n) {
    const uint32_t n_tris = (uint32_t)(tris.size() / 3);
    std::vector<uint32_t> begin(n + 1, 0xABABABABu), corners(tris.size(), 0xCDCDCDCDu);
    uint32_t bad = 77;
    EXPECT(dh_subjects_corner_lists(tris.data(), n_tris, n, begin.data(), corners.data(), &bad), "%s: refused", what);
    EXPECT(bad == 77, "%s: bad_tri written", what);
    EXPECT(begin[0] == 0 && begin[n] == tris.size(), "%s: begin[0] = %u, begin[n] = %u", what, begin[0], begin[n]);
    for (uint32_t v = 0; v < n; ++v) {
        std::vector<uint32_t> want;
        for (uint32_t q = 0; q < tris.size(); ++q)
            if (tris[q] == v) want.push_back(q);
        EXPECT(begin[v] <= begin[v + 1] && begin[v + 1] - begin[v] == want.size(), "%s: vertex %u has %u corners, expected %zu", what, v,
               begin[v + 1] - begin[v], want.size());
        if (begin[v + 1] - begin[v] != want.size()) continue;
        for (size_t j = 0; j < want.size(); ++j) EXPECT(corners[begin[v] + j] == want[j], "%s: vertex %u corner %zu is %u, expected %u", what, v, j, corners[begin[v] + j], want[j]);
    }
}

int main() {
    // ---- corner lists
    const std::vector<uint32_t> tetra = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
    check_lists("tetrahedron", tetra, 4);
    std::vector<uint32_t> fan;
    for (uint32_t t = 0; t < 300; ++t) { fan.push_back(0); fan.push_back(1 + t); fan.push_back(1 + (t + 1) % 300); }
    check_lists("fan", fan, 301);
    check_lists("a vertex twice in one triangle, vertex 2 in none", {0, 0, 1, 3, 1, 0, 1, 1, 1}, 4);
    check_lists("one triangle", {2, 1, 0}, 3);
    for (int round = 0; round < 20; ++round) {
        const uint32_t n = 1 + rnd(40), n_tris = 1 + rnd(200);
        std::vector<uint32_t> tris(3 * (size_t)n_tris);
        for (auto &v : tris) v = rnd(n);
        check_lists("random", tris, n);
    }
    {   // an index >= n: refused, the first such triangle named
        std::vector<uint32_t> tris = {0, 1, 2, 0, 2, 4, 9, 1, 2};
        std::vector<uint32_t> begin(5), corners(9);
        uint32_t bad = 77;
        EXPECT(!dh_subjects_corner_lists(tris.data(), 3, 4, begin.data(), corners.data(), &bad) && bad == 1, "index 4 of 4: bad = %u", bad);
        EXPECT(!dh_subjects_corner_lists(tris.data(), 3, 4, begin.data(), corners.data(), nullptr), "NULL bad_tri");
        tris[5] = 3;
        EXPECT(!dh_subjects_corner_lists(tris.data(), 3, 4, begin.data(), corners.data(), &bad) && bad == 2, "index 9 of 4: bad = %u", bad);
        tris[6] = 0xFFFFFFFFu;
        EXPECT(!dh_subjects_corner_lists(tris.data(), 3, 4, begin.data(), corners.data(), &bad) && bad == 2, "index 2^32 - 1: bad = %u", bad);
        EXPECT(dh_subjects_corner_lists(tris.data(), 2, 4, begin.data(), corners.data(), &bad), "the first two triangles alone");
    }

    // ---- the base mesh's zero normals
    {
        const float pts[] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5};
        std::vector<uint32_t> begin(6), corners(12);
        EXPECT(dh_subjects_corner_lists(tetra.data(), 4, 4, begin.data(), corners.data(), nullptr), "tetrahedron");
        EXPECT(dh_subjects_first_zero_normal(pts, tetra.data(), begin.data(), corners.data(), 4) == 4, "a tetrahedron has no zero normal");
        // a fifth vertex that no triangle names
        EXPECT(dh_subjects_corner_lists(tetra.data(), 4, 5, begin.data(), corners.data(), nullptr), "five vertices");
        EXPECT(dh_subjects_first_zero_normal(pts, tetra.data(), begin.data(), corners.data(), 5) == 4, "the vertex without a triangle");
        // all four points on one line: every face product is zero
        const float line[] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
        EXPECT(dh_subjects_corner_lists(tetra.data(), 4, 4, begin.data(), corners.data(), nullptr), "tetrahedron");
        EXPECT(dh_subjects_first_zero_normal(line, tetra.data(), begin.data(), corners.data(), 4) == 0, "collinear points");
        // two triangles back to back: their face products cancel at the shared vertices
        const std::vector<uint32_t> pair = {0, 1, 2, 0, 2, 1};
        EXPECT(dh_subjects_corner_lists(pair.data(), 2, 3, begin.data(), corners.data(), nullptr), "back to back");
        EXPECT(dh_subjects_first_zero_normal(pts, pair.data(), begin.data(), corners.data(), 3) == 0, "back to back");
    }

    // ---- the radius bound: no point deformed with |c_k| <= max_coeff lies further out
    EXPECT(dh_subjects_radius_bound(100.0, 4, 0.5, 10.0) == 120.0, "100 + 4 * 0.5 * 10");
    EXPECT(dh_subjects_radius_bound(100.0, 8, 0.25, 0.0) == 100.0, "a basis of zeros");
    EXPECT(dh_subjects_radius_bound(0.0, 1, 1e-3, 256.0) == 0.256, "a base mesh at the origin");
    for (int round = 0; round < 50; ++round) {
        const uint32_t n = 1 + rnd(30), nk = 1 + rnd(8);
        const double max_coeff = (1 + rnd(1000)) / 500.0;
        std::vector<float> v(3 * (size_t)n), B((size_t)nk * 3 * n);
        for (auto &x : v) x = (float)((int)rnd(4001) - 2000) / 7.0f;
        for (auto &x : B) x = (float)((int)rnd(2001) - 1000) / 3.0f;
        double r2 = 0.0, l2 = 0.0;
        for (uint32_t i = 0; i < n; ++i) {
            double v2 = 0.0;
            for (int c = 0; c < 3; ++c) v2 += (double)v[3 * i + c] * (double)v[3 * i + c];
            r2 = v2 > r2 ? v2 : r2;
            for (uint32_t k = 0; k < nk; ++k) {
                double b2 = 0.0;
                for (int c = 0; c < 3; ++c) b2 += (double)B[((size_t)k * n + i) * 3 + c] * (double)B[((size_t)k * n + i) * 3 + c];
                l2 = b2 > l2 ? b2 : l2;
            }
        }
        const double bound = dh_subjects_radius_bound(sqrt(r2), nk, max_coeff, sqrt(l2));
        for (int corner = 0; corner < 16; ++corner)
            for (uint32_t i = 0; i < n; ++i) {
                double x[3] = {(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]};
                for (uint32_t k = 0; k < nk; ++k) {
                    const double ck = (rnd(2) ? max_coeff : -max_coeff);
                    for (int c = 0; c < 3; ++c) x[c] = x[c] + ck * (double)B[((size_t)k * n + i) * 3 + c];
                }
                const float f[3] = {(float)x[0], (float)x[1], (float)x[2]};
                const double len = sqrt(((double)f[0] * f[0] + (double)f[1] * f[1]) + (double)f[2] * f[2]);
                EXPECT(len <= bound * (1.0 + 1.2e-7), "round %d point %u: |v'| = %.17g above the bound %.17g", round, i, len, bound);
            }
    }

    if (failures) { fprintf(stderr, "%d of %ld checks failed\n", failures, checks); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
