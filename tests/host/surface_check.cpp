// The host side of a surface set that is plain functions (depthhead_amd/csrc/dh_fit.h), for
// tests/test_surface_host.py: dh_subjects_neighbour_lists -- each vertex's unique neighbours along triangle edges, itself
// excluded, ascending -- against a search through the triangles, on a tetrahedron, a fan whose hub lies in 300 triangles, a
// triangle that names a vertex twice, a vertex no triangle names (degree 0), seeded random meshes, and the refusal of an index
// >= n; and dh_surface_radius_bound against the points themselves, evaluated at random corners of the coefficient and offset
// cube with unit normals rounded to f32.  A stand-alone program: it prints what it checked and exits 0, or says what differed and
// exits 1.
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

// begin / list of `tris` against the definition: j is a neighbour of v when j != v and some triangle names both
static void check_lists(const char *what, const std::vector<uint32_t> &tris, uint32_t n) {
    const uint32_t n_tris = (uint32_t)(tris.size() / 3);
    std::vector<uint32_t> begin(n + 1, 0xABABABABu), list(6 * (size_t)n_tris + 1, 0xCDCDCDCDu), work(6 * (size_t)n_tris + 1, 0xEFEFEFEFu);
    uint32_t bad = 77;
    EXPECT(dh_subjects_neighbour_lists(tris.data(), n_tris, n, begin.data(), list.data(), work.data(), &bad), "%s: refused", what);
    EXPECT(bad == 77, "%s: bad_tri written", what);
    EXPECT(begin[0] == 0 && begin[n] <= 6 * n_tris, "%s: begin[0] = %u, begin[n] = %u", what, begin[0], begin[n]);
    EXPECT(list[6 * (size_t)n_tris] == 0xCDCDCDCDu && work[6 * (size_t)n_tris] == 0xEFEFEFEFu, "%s: written past 6 n_tris", what);
    for (uint32_t v = 0; v < n; ++v) {
        std::vector<uint32_t> want;
        for (uint32_t j = 0; j < n; ++j) {
            bool shared = false;
            for (uint32_t t = 0; t < n_tris && !shared; ++t) {
                bool has_v = false, has_j = false;
                for (int c = 0; c < 3; ++c) { has_v = has_v || tris[3 * t + c] == v; has_j = has_j || tris[3 * t + c] == j; }
                shared = has_v && has_j;
            }
            if (shared && j != v) want.push_back(j);
        }
        EXPECT(begin[v] <= begin[v + 1] && begin[v + 1] - begin[v] == want.size(), "%s: vertex %u has %u neighbours, expected %zu", what, v,
               begin[v + 1] - begin[v], want.size());
        if (begin[v + 1] - begin[v] != want.size()) continue;
        for (size_t j = 0; j < want.size(); ++j) EXPECT(list[begin[v] + j] == want[j], "%s: vertex %u neighbour %zu is %u, expected %u", what, v, j, list[begin[v] + j], want[j]);
    }
}

int main() {
    // ---- neighbour lists
    check_lists("tetrahedron", {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3}, 4);
    std::vector<uint32_t> fan;
    for (uint32_t t = 0; t < 300; ++t) { fan.push_back(0); fan.push_back(1 + t); fan.push_back(1 + (t + 1) % 300); }
    check_lists("fan", fan, 301);
    check_lists("a vertex twice in one triangle, vertex 2 in none", {0, 0, 1, 3, 1, 0, 1, 1, 1}, 4);
    check_lists("one triangle, two vertices of degree 0", {2, 1, 0}, 5);
    check_lists("a triangle of one vertex", {1, 1, 1}, 2);
    for (int round = 0; round < 20; ++round) {
        const uint32_t n = 1 + rnd(40), n_tris = 1 + rnd(200);
        std::vector<uint32_t> tris(3 * (size_t)n_tris);
        for (auto &v : tris) v = rnd(n);
        check_lists("random", tris, n);
    }
    {   // an index >= n: refused, the first such triangle named
        std::vector<uint32_t> tris = {0, 1, 2, 0, 2, 4, 9, 1, 2};
        std::vector<uint32_t> begin(5), list(18), work(18);
        uint32_t bad = 77;
        EXPECT(!dh_subjects_neighbour_lists(tris.data(), 3, 4, begin.data(), list.data(), work.data(), &bad) && bad == 1, "index 4 of 4: bad = %u", bad);
        EXPECT(!dh_subjects_neighbour_lists(tris.data(), 3, 4, begin.data(), list.data(), work.data(), nullptr), "NULL bad_tri");
        tris[5] = 3;
        EXPECT(!dh_subjects_neighbour_lists(tris.data(), 3, 4, begin.data(), list.data(), work.data(), &bad) && bad == 2, "index 9 of 4: bad = %u", bad);
        EXPECT(dh_subjects_neighbour_lists(tris.data(), 2, 4, begin.data(), list.data(), work.data(), &bad), "the first two triangles alone");
    }

    // ---- the radius bound: no point with |c_k| <= max_coeff and |o| <= max_offset lies further out
    EXPECT(dh_surface_radius_bound(100.0, 4, 0.5, 10.0, 8.0) == 120.0 + 8.0 * 1.01, "100 + 4 * 0.5 * 10 + 8 * 1.01");
    EXPECT(dh_surface_radius_bound(100.0, 8, 0.25, 0.0, DH_SURFACE_MAX_OFFSET) == 100.0 + 64.0 * 1.01, "a basis of zeros, the largest offset");
    for (int round = 0; round < 50; ++round) {
        const uint32_t n = 1 + rnd(30), nk = 1 + rnd(8);
        const double max_coeff = (1 + rnd(1000)) / 500.0, max_offset = (1 + rnd(6400)) / 100.0;
        std::vector<float> v(3 * (size_t)n), B((size_t)nk * 3 * n), nb(3 * (size_t)n);
        for (auto &x : v) x = (float)((int)rnd(4001) - 2000) / 7.0f;
        for (auto &x : B) x = (float)((int)rnd(2001) - 1000) / 3.0f;
        for (uint32_t i = 0; i < n; ++i) {                                         // a unit vector rounded to f32, as section 25's normals are
            double m[3] = {(double)((int)rnd(2001) - 1000), (double)((int)rnd(2001) - 1000), (double)rnd(1000) + 1.0};
            const double ln = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            for (int c = 0; c < 3; ++c) nb[3 * i + c] = (float)(m[c] / ln);
        }
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
            const double nl = sqrt(((double)nb[3 * i] * nb[3 * i] + (double)nb[3 * i + 1] * nb[3 * i + 1]) + (double)nb[3 * i + 2] * nb[3 * i + 2]);
            EXPECT(nl <= DH_SURFACE_NB_BOUND, "|nb| = %.17g", nl);
        }
        const double bound = dh_surface_radius_bound(sqrt(r2), nk, max_coeff, sqrt(l2), max_offset);
        EXPECT(bound > dh_subjects_radius_bound(sqrt(r2), nk, max_coeff, sqrt(l2)), "the bound grows");
        for (int corner = 0; corner < 16; ++corner)
            for (uint32_t i = 0; i < n; ++i) {
                double x[3] = {(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]};
                for (uint32_t k = 0; k < nk; ++k) {
                    const double ck = (rnd(2) ? max_coeff : -max_coeff);
                    for (int c = 0; c < 3; ++c) x[c] = x[c] + ck * (double)B[((size_t)k * n + i) * 3 + c];
                }
                const double o = rnd(2) ? max_offset : -max_offset;
                for (int c = 0; c < 3; ++c) x[c] = x[c] + o * (double)nb[3 * i + c];
                const float f[3] = {(float)x[0], (float)x[1], (float)x[2]};
                const double len = sqrt(((double)f[0] * f[0] + (double)f[1] * f[1]) + (double)f[2] * f[2]);
                EXPECT(len <= bound * (1.0 + 1.2e-7), "round %d point %u: |v'| = %.17g above the bound %.17g", round, i, len, bound);
            }
    }

    if (failures) { fprintf(stderr, "%d of %ld checks failed\n", failures, checks); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
