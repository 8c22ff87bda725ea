// The live-tracking rule (depthhead_amd/csrc/dh_track.h) on the host, for tests/test_track_rule.py.  Reads one case per line
// from stdin -- flags, then the new midpoint, the stored midpoint (f32 bit patterns, hex) and has_rot -- applies
// dh_track_update and prints the stored midpoint (bit patterns), the mask and has_rot after it.
#include <stdio.h>
#include <string.h>

#include "dh_track.h"

static float f32(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

int main() {
    unsigned flags, m[3], st[3], hr;
    int cases = 0;
    while (scanf("%x %x %x %x %x %x %x %x", &flags, &m[0], &m[1], &m[2], &st[0], &st[1], &st[2], &hr) == 8) {
        const float mid[3] = {f32(m[0]), f32(m[1]), f32(m[2])};
        float midp[3] = {f32(st[0]), f32(st[1]), f32(st[2])};
        const double rot[3] = {0.1 * cases, -0.2, 0.3};
        double srot[3] = {0, 0, 0};
        uint8_t mask = 0xff, has_rot = (uint8_t)hr;
        // the mask a step would read before this update: what --prevguess offers from the stored state
        const unsigned before = dh_track_mask(flags, midp, has_rot != 0);
        dh_track_update(flags, mid, rot, midp, srot, &mask, &has_rot);
        if (srot[0] != rot[0] || srot[1] != rot[1] || srot[2] != rot[2]) { printf("rotation not stored\n"); return 1; }
        printf("%08x %08x %08x %u %u %u\n", bits(midp[0]), bits(midp[1]), bits(midp[2]), (unsigned)mask, (unsigned)has_rot, before);
        ++cases;
    }
    fprintf(stderr, "%d cases\n", cases);
    return cases > 0 ? 0 : 1;
}
