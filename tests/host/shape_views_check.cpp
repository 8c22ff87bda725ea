// The two decisions of a multi-view shape step that are plain functions (depthhead_amd/csrc/dh_fit.h) on
// the host, for tests/test_shape_views_rule.py: dh_shape_view_bit, the r-th set bit of a view mask, against a naive loop for
// every rank of hand-made masks and 400 seeded ones; and dh_shape_views_skip, the whole-instance test that the host form turns
// into its refusals and k_shape_accumulate_views into a skip, on hand cases.  A stand-alone program: it prints what it checked
// and exits 0, or says what differed and exits 1.
#include <math.h>
#include <stdio.h>

#include "dh_fit.h"

static int failures = 0;
#define EXPECT(cond, ...)                                                                                                       \
    do {                                                                                                                        \
        if (!(cond)) { fprintf(stderr, "%s:%d: " #cond ": ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++failures; } \
    } while (0)

// the r-th set bit by walking the bits upward; 64 where there is none
static uint32_t naive_bit(uint64_t mask, uint32_t r) {
    for (uint32_t k = 0; k < 64; ++k)
        if ((mask >> k) & 1ull) {
            if (r == 0) return k;
            --r;
        }
    return 64;
}

static uint64_t splitmix(uint64_t &state) {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long check_mask(uint64_t mask) {
    long checks = 0;
    const uint32_t count = (uint32_t)__builtin_popcountll(mask);
    for (uint32_t r = 0; r <= 65; ++r, ++checks) {
        const uint32_t got = dh_shape_view_bit(mask, r), want = naive_bit(mask, r);
        EXPECT(got == want, "mask %016llx rank %u: %u, expected %u", (unsigned long long)mask, r, got, want);
        EXPECT((r < count) == (got < 64), "mask %016llx rank %u of %u set bits gives %u", (unsigned long long)mask, r, count, got);
    }
    EXPECT(dh_shape_view_bit(mask, 0xffffffffu) == 64, "mask %016llx rank 2^32 - 1", (unsigned long long)mask);
    return checks + 1;
}

static dh_view_instance instance(uint32_t first_cam, uint64_t views) {
    dh_view_instance in;
    memset(&in, 0, sizeof in);
    in.first_cam = first_cam; in.views = views;
    in.R[0] = in.R[4] = in.R[8] = 1.0f;
    in.t[2] = 800.0f;
    in.scale = 1.0f;
    return in;
}

int main() {
    long checks = 0;
    const uint64_t hand[] = {1ull, 1ull << 63, ~0ull, 0b101ull, 0ull, 0x8000000000000001ull, 0xAAAAAAAAAAAAAAAAull, 0x00000000FFFFFFFFull,
                             0xFFFFFFFF00000000ull};
    for (uint64_t m : hand) checks += check_mask(m);
    EXPECT(dh_shape_view_bit(0b101ull, 0) == 0 && dh_shape_view_bit(0b101ull, 1) == 2 && dh_shape_view_bit(0b101ull, 2) == 64, "0b101");
    EXPECT(dh_shape_view_bit(1ull << 63, 0) == 63 && dh_shape_view_bit(~0ull, 63) == 63 && dh_shape_view_bit(~0ull, 64) == 64, "the ends");
    uint64_t state = 2300;
    for (int i = 0; i < 400; ++i) {
        uint64_t m = splitmix(state);
        if (i % 4 == 1) m &= splitmix(state) & splitmix(state);          // sparse
        if (i % 4 == 2) m |= splitmix(state) | splitmix(state);          // dense
        if (i % 4 == 3) m <<= splitmix(state) % 64;                      // nothing below a seeded bit
        checks += check_mask(m);
    }

    // ---- the whole-instance test: n = 6 cameras, 2 sets, 3 subjects, a model of radius 100 mm, a basis whose largest field is 120 mm
    struct Case { const char *what; dh_view_instance in; uint32_t set, subject; int why; };
    auto why = [](const dh_view_instance &in, uint32_t set, uint32_t subject) {
        return dh_shape_views_skip(in, set, subject, 6, 2, 3, 100.0, 120.0).why;
    };
    dh_view_instance nan_R = instance(0, 0b111), nan_t = instance(0, 0b111), inf_scale = instance(0, 0b111), skew = instance(0, 0b111),
                     far = instance(0, 0b111), wide = instance(0, 0b111), at_field = instance(0, 0b111);
    nan_R.R[4] = NAN; nan_t.t[1] = NAN; inf_scale.scale = INFINITY; skew.R[1] = 0.5f;
    far.scale = 41.0f;                    // 4100 mm > DH_FIT_MAX_EXTENT
    wide.scale = 2.2f;                    // 264 mm > DH_SHAPE_MAX_FIELD
    at_field.scale = 2.125f;              // 255 mm
    const Case cases[] = {
        {"three views", instance(0, 0b111), 0, 0, DH_SHAPE_VIEWS_OK},
        {"the last camera, set and subject", instance(5, 1), 1, 2, DH_SHAPE_VIEWS_OK},
        {"bit 5 from camera 0", instance(0, 1ull << 5), 0, 0, DH_SHAPE_VIEWS_OK},
        {"the field at its limit", at_field, 0, 0, DH_SHAPE_VIEWS_OK},
        {"DH_SHAPE_SKIP", instance(0, 0b111), 0, DH_SHAPE_SKIP, DH_SHAPE_VIEWS_SKIPPED},
        {"DH_SHAPE_SKIP comes before everything", instance(99, 0), 7, DH_SHAPE_SKIP, DH_SHAPE_VIEWS_SKIPPED},
        {"no view", instance(0, 0), 0, 0, DH_SHAPE_VIEWS_NO_VIEW},
        {"no view comes before the set", instance(0, 0), 2, 0, DH_SHAPE_VIEWS_NO_VIEW},
        {"bit 6 from camera 0", instance(0, 1ull << 6), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"bit 1 from camera 5", instance(5, 0b11), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"bit 63", instance(0, (1ull << 63) | 1ull), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"first_cam 2^32 - 1 and bit 63 do not wrap", instance(0xffffffffu, 1ull << 63), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"first_cam 2^32 - 1 and bit 1 do not wrap", instance(0xffffffffu, 0b10), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"set 2 of 2", instance(0, 0b111), 2, 0, DH_SHAPE_VIEWS_SET},
        {"set 2^32 - 1", instance(0, 0b111), 0xffffffffu, 0, DH_SHAPE_VIEWS_SET},
        {"the camera comes before the set", instance(4, 0b100), 2, 0, DH_SHAPE_VIEWS_CAMERA},
        {"subject 3 of 3", instance(0, 0b111), 0, 3, DH_SHAPE_VIEWS_SUBJECT},
        {"subject 2^32 - 2", instance(0, 0b111), 0, 0xfffffffeu, DH_SHAPE_VIEWS_SUBJECT},
        {"the set comes before the subject", instance(0, 0b111), 2, 3, DH_SHAPE_VIEWS_SET},
        {"a NaN in R", nan_R, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"a NaN in t", nan_t, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"an infinite scale", inf_scale, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"an R that is no rotation", skew, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"beyond the extent", far, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"beyond the field limit", wide, 0, 0, DH_SHAPE_VIEWS_FAULT},
    };
    for (const Case &c : cases) {
        const int got = why(c.in, c.set, c.subject);
        EXPECT(got == c.why, "%s: %d, expected %d", c.what, got, c.why);
        ++checks;
    }
    // what the fault is, for the host's message
    EXPECT(dh_shape_views_skip(nan_R, 0, 0, 6, 2, 3, 100.0, 120.0).fault.why == DH_FIT_INST_NOT_FINITE, "NaN in R: the fault");
    EXPECT(dh_shape_views_skip(skew, 0, 0, 6, 2, 3, 100.0, 120.0).fault.why == DH_FIT_INST_NOT_ORTHONORMAL, "skew: the fault");
    EXPECT(dh_shape_views_skip(far, 0, 0, 6, 2, 3, 100.0, 120.0).fault.why == DH_FIT_INST_EXTENT, "far: the fault");
    EXPECT(dh_shape_views_skip(wide, 0, 0, 6, 2, 3, 100.0, 120.0).fault.why == DH_FIT_INST_FIELD, "wide: the fault");
    EXPECT(dh_shape_views_skip(instance(5, 0b11), 0, 0, 6, 2, 3, 100.0, 120.0).last == 6, "the camera of the highest bit");
    // an instance that passes names only cameras below n with every rank below its count
    for (uint64_t m : {0b111111ull, 0b100001ull, 0b010ull}) {
        const dh_view_instance in = instance(0, m);
        EXPECT(why(in, 1, 2) == DH_SHAPE_VIEWS_OK, "mask %llx", (unsigned long long)m);
        for (uint32_t r = 0; r < (uint32_t)__builtin_popcountll(m); ++r, ++checks)
            EXPECT(in.first_cam + dh_shape_view_bit(m, r) < 6, "mask %llx rank %u", (unsigned long long)m, r);
    }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
