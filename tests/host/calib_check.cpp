// The decisions of a calibration step that are plain functions (depthhead_amd/csrc/dh_fit.h) on the host,
// for tests/test_calibrate_rule.py: dh_calib_skip, the whole-instance test that the host form turns into its refusals and
// k_calib_accumulate into a skip -- each refusal in the header's order, a NaN in every field -- and dh_calib_pair, the test of
// one (instance, view) pair: held cameras, the arm limit at exactly DH_CALIB_MAX_ARM and just beyond it, and the composite
// pose and pivot it hands to the kernel.  A stand-alone program: it prints what it checked and exits 0, or says what differed
// and exits 1.
#include <math.h>
#include <stdio.h>

#include "dh_fit.h"

static int failures = 0;
static long checks = 0;
#define EXPECT(cond, ...)                                                                                                       \
    do {                                                                                                                        \
        ++checks;                                                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: " #cond ": ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++failures; } \
    } while (0)

static dh_view_instance instance(uint32_t first_cam, uint64_t views) {
    dh_view_instance in;
    memset(&in, 0, sizeof in);
    in.first_cam = first_cam; in.views = views;
    in.R[0] = in.R[4] = in.R[8] = 1.0f;
    in.t[2] = 800.0f;
    in.scale = 1.0f;
    return in;
}
static FitView view(float ux, float uy, float uz) {
    FitView v;
    memset(&v, 0, sizeof v);
    v.V[0] = v.V[4] = v.V[8] = 1.0f;
    v.u[0] = ux; v.u[1] = uy; v.u[2] = uz;
    return v;
}

int main() {
    // ---- the whole-instance test: n = 6 cameras, 2 sets, a model of radius 100 mm
    struct Case { const char *what; dh_view_instance in; uint32_t set, take; int why; };
    auto why = [](const dh_view_instance &in, uint32_t set, uint32_t take) { return dh_calib_skip(in, set, take, 6, 2, 100.0).why; };
    dh_view_instance inf_scale = instance(0, 0b111), nan_scale = instance(0, 0b111), skew = instance(0, 0b111), far = instance(0, 0b111),
                     at_extent = instance(0, 0b111), big = instance(0, 0b111);
    inf_scale.scale = INFINITY; nan_scale.scale = NAN; skew.R[1] = 0.5f;
    far.scale = 41.0f;                    // 4100 mm > DH_FIT_MAX_EXTENT
    at_extent.scale = 40.96f;             // (float)40.96 * 100 is just below 4096
    big.scale = -40.0f;                   // the sign does not matter, and no basis: no field limit
    const Case cases[] = {
        {"three views", instance(0, 0b111), 0, 0, DH_SHAPE_VIEWS_OK},
        {"the last camera and set", instance(5, 1), 1, 0, DH_SHAPE_VIEWS_OK},
        {"any take but DH_CALIB_SKIP takes part", instance(0, 0b111), 0, 7, DH_SHAPE_VIEWS_OK},
        {"take 2^32 - 2 takes part", instance(0, 0b111), 0, 0xfffffffeu, DH_SHAPE_VIEWS_OK},
        {"bit 5 from camera 0", instance(0, 1ull << 5), 0, 0, DH_SHAPE_VIEWS_OK},
        {"the extent at its limit", at_extent, 0, 0, DH_SHAPE_VIEWS_OK},
        {"a negative scale below the extent", big, 0, 0, DH_SHAPE_VIEWS_OK},
        {"DH_CALIB_SKIP", instance(0, 0b111), 0, DH_CALIB_SKIP, DH_SHAPE_VIEWS_SKIPPED},
        {"DH_CALIB_SKIP comes before everything", instance(99, 0), 7, DH_CALIB_SKIP, DH_SHAPE_VIEWS_SKIPPED},
        {"no view", instance(0, 0), 0, 0, DH_SHAPE_VIEWS_NO_VIEW},
        {"no view comes before the camera and the set", instance(9, 0), 2, 0, DH_SHAPE_VIEWS_NO_VIEW},
        {"bit 6 from camera 0", instance(0, 1ull << 6), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"bit 1 from camera 5", instance(5, 0b11), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"bit 63", instance(0, (1ull << 63) | 1ull), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"first_cam 2^32 - 1 and bit 63 do not wrap", instance(0xffffffffu, 1ull << 63), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"first_cam 2^32 - 1 and bit 1 do not wrap", instance(0xffffffffu, 0b10), 0, 0, DH_SHAPE_VIEWS_CAMERA},
        {"the camera comes before the set", instance(4, 0b100), 2, 0, DH_SHAPE_VIEWS_CAMERA},
        {"set 2 of 2", instance(0, 0b111), 2, 0, DH_SHAPE_VIEWS_SET},
        {"set 2^32 - 1", instance(0, 0b111), 0xffffffffu, 0, DH_SHAPE_VIEWS_SET},
        {"the set comes before the pose", skew, 2, 0, DH_SHAPE_VIEWS_SET},
        {"an infinite scale", inf_scale, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"a NaN scale", nan_scale, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"an R that is no rotation", skew, 0, 0, DH_SHAPE_VIEWS_FAULT},
        {"beyond the extent", far, 0, 0, DH_SHAPE_VIEWS_FAULT},
    };
    for (const Case &c : cases) {
        const int got = why(c.in, c.set, c.take);
        EXPECT(got == c.why, "%s: %d, expected %d", c.what, got, c.why);
    }
    // a NaN and an infinity in every field of the pose: NOT_FINITE, whatever else is wrong with it
    for (int q = 0; q < 13; ++q)
        for (float bad : {NAN, INFINITY, -INFINITY}) {
            dh_view_instance in = instance(0, 0b111);
            if (q < 9) in.R[q] = bad; else if (q < 12) in.t[q - 9] = bad; else in.scale = bad;
            const ShapeViewsSkip s = dh_calib_skip(in, 0, 0, 6, 2, 100.0);
            EXPECT(s.why == DH_SHAPE_VIEWS_FAULT && s.fault.why == DH_FIT_INST_NOT_FINITE, "field %d = %g: %d / %d", q, (double)bad, s.why, s.fault.why);
            EXPECT(dh_calib_skip(in, 0, DH_CALIB_SKIP, 6, 2, 100.0).why == DH_SHAPE_VIEWS_SKIPPED, "field %d = %g with DH_CALIB_SKIP", q, (double)bad);
        }
    // what the fault is, for the host's message; the order within the pose: finite, orthonormal, extent
    EXPECT(dh_calib_skip(skew, 0, 0, 6, 2, 100.0).fault.why == DH_FIT_INST_NOT_ORTHONORMAL, "skew: the fault");
    EXPECT(dh_calib_skip(far, 0, 0, 6, 2, 100.0).fault.why == DH_FIT_INST_EXTENT, "far: the fault");
    dh_view_instance skew_far = far; skew_far.R[1] = 0.5f;
    EXPECT(dh_calib_skip(skew_far, 0, 0, 6, 2, 100.0).fault.why == DH_FIT_INST_NOT_ORTHONORMAL, "skew comes before the extent");
    EXPECT(dh_calib_skip(instance(5, 0b11), 0, 0, 6, 2, 100.0).last == 6, "the camera of the highest bit");

    // ---- the pair test.  V = I, so t_v = t_w + u and g_c = o + u exactly: the arm is t_w - o
    const double origin[3] = {0.0, 0.0, 0.0};
    {
        const dh_view_instance in = instance(0, 1);                      // t = (0, 0, 800)
        const FitView v = view(10.0f, -20.0f, 30.0f);
        const CalibPair p = dh_calib_pair(in, v, origin, false);
        EXPECT(p.why == DH_CALIB_PAIR_OK, "a pair within the arm: %d", p.why);
        EXPECT(p.t[0] == 10.0 && p.t[1] == -20.0 && p.t[2] == 830.0, "t_v = (%g, %g, %g)", p.t[0], p.t[1], p.t[2]);
        EXPECT(p.g[0] == 10.0 && p.g[1] == -20.0 && p.g[2] == 30.0, "g_c = (%g, %g, %g)", p.g[0], p.g[1], p.g[2]);
        for (int q = 0; q < 9; ++q) EXPECT(p.R[q] == (q == 0 || q == 4 || q == 8 ? 1.0 : 0.0), "R_v[%d] = %g", q, p.R[q]);
        EXPECT(dh_calib_pair(in, v, origin, true).why == DH_CALIB_PAIR_HELD, "a held camera");
        double g[3];
        dh_calib_pivot(v, origin, g);
        EXPECT(g[0] == p.g[0] && g[1] == p.g[1] && g[2] == p.g[2], "dh_calib_pivot is the pair's g_c");
        const double o[3] = {1.0, 2.0, 3.0};
        const CalibPair po = dh_calib_pair(in, v, o, false);
        EXPECT(po.g[0] == 11.0 && po.g[1] == -18.0 && po.g[2] == 33.0, "a pivot off the origin: (%g, %g, %g)", po.g[0], po.g[1], po.g[2]);
    }
    // a turned camera: V is a quarter turn about y, camera x = world z, camera z = -world x
    {
        FitView v = view(0.0f, 0.0f, 1000.0f);
        v.V[0] = 0.0f; v.V[2] = 1.0f; v.V[6] = -1.0f; v.V[8] = 0.0f;
        dh_view_instance in = instance(0, 1);
        in.t[0] = -100.0f; in.t[1] = 50.0f; in.t[2] = 800.0f;
        const CalibPair p = dh_calib_pair(in, v, origin, false);
        EXPECT(p.why == DH_CALIB_PAIR_OK && p.t[0] == 800.0 && p.t[1] == 50.0 && p.t[2] == 1100.0, "turned: %d (%g, %g, %g)", p.why, p.t[0], p.t[1], p.t[2]);
        EXPECT(p.R[2] == 1.0 && p.R[4] == 1.0 && p.R[6] == -1.0 && p.R[0] == 0.0 && p.R[8] == 0.0, "turned: R_v = V");
    }
    // the arm limit, on every axis and both signs: exactly 2048 takes part, the next float beyond it does not, nor does a NaN
    for (int axis = 0; axis < 3; ++axis)
        for (float sign : {1.0f, -1.0f}) {
            dh_view_instance in = instance(0, 1);
            in.t[0] = in.t[1] = in.t[2] = 0.0f;
            in.t[axis] = sign * 2048.0f;
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), origin, false).why == DH_CALIB_PAIR_OK, "axis %d sign %g at 2048", axis, (double)sign);
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), origin, true).why == DH_CALIB_PAIR_HELD, "axis %d sign %g at 2048, held", axis, (double)sign);
            in.t[axis] = sign * nextafterf(2048.0f, 4096.0f);
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), origin, false).why == DH_CALIB_PAIR_ARM, "axis %d sign %g just beyond 2048", axis, (double)sign);
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), origin, true).why == DH_CALIB_PAIR_HELD, "held comes before the arm");
            // the pivot moves the limit with it
            double o[3] = {0.0, 0.0, 0.0};
            o[axis] = (double)sign * 0.5;
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), o, false).why == DH_CALIB_PAIR_OK, "axis %d sign %g: the pivot half a millimetre along", axis, (double)sign);
            in.t[axis] = sign * 2048.0f;
            o[axis] = -(double)sign * 0.5;
            EXPECT(dh_calib_pair(in, view(5.0f, 6.0f, 7.0f), o, false).why == DH_CALIB_PAIR_ARM, "axis %d sign %g: the pivot half a millimetre back", axis, (double)sign);
            FitView nv = view(0.0f, 0.0f, 0.0f);
            nv.u[axis] = NAN;
            in.t[axis] = 0.0f;
            EXPECT(dh_calib_pair(in, nv, origin, false).why == DH_CALIB_PAIR_ARM, "axis %d: a NaN arm fails the test", axis);
        }
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("ok %ld checks\n", checks);
    return 0;
}
