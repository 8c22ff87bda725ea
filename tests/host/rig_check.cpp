// The rig tracker step (depthhead_amd/csrc/dh_rig.h) on the host, for tests/test_rig_rule.py.  Reads cases from stdin, binary:
// eight u32 (n_cams, max_heads, fuse_gate, gate, max_misses, next_id, cam0, has_present), then DH_RIG_MAX_TRACKS dh_rig_track
// records, R [n_cams][9] f32, t [n_cams][3] f32, present [n_cams] u32, n_heads [n_cams] u32 and n_cams * max_heads dh_head
// records.  For each it runs dh_rig_step, the sequential statement of what one workgroup of k_rig_fuse does, and writes the
// records after the step, next_id, the n_cams * max_heads ids, n_persons and the DH_RIG_MAX_PERSONS person records.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dh_rig.h"

template <typename T>
static bool rd(std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), stdin) == v.size(); }

int main() {
    uint32_t hdr[8];
    int cases = 0;
    while (fread(hdr, sizeof hdr, 1, stdin) == 1) {
        const int n_cams = (int)hdr[0], max_heads = (int)hdr[1];
        if (n_cams < 1 || n_cams > DH_RIG_MAX_CAMERAS || max_heads < 1 || max_heads > DH_MAX_HEADS) {
            fprintf(stderr, "n_cams %d max_heads %d\n", n_cams, max_heads);
            return 1;
        }
        dh_rig_track tr[DH_RIG_MAX_TRACKS];
        std::vector<float> R((size_t)n_cams * 9), t((size_t)n_cams * 3);
        std::vector<uint32_t> pres32((size_t)n_cams), n_heads((size_t)n_cams);
        std::vector<dh_head> heads((size_t)n_cams * max_heads);
        if (fread(tr, sizeof tr, 1, stdin) != 1 || !rd(R) || !rd(t) || !rd(pres32) || !rd(n_heads) || !rd(heads)) {
            fprintf(stderr, "truncated case %d\n", cases);
            return 1;
        }
        std::vector<uint8_t> present((size_t)n_cams);
        for (int k = 0; k < n_cams; ++k) present[(size_t)k] = pres32[(size_t)k] ? 1 : 0;
        std::vector<uint32_t> ids(heads.size(), 0xdeadbeefu);
        dh_rig_person persons[DH_RIG_MAX_PERSONS];
        memset(persons, 0xee, sizeof persons);
        uint32_t next_id = hdr[5], n_persons = 0xdeadbeefu;
        dh_rig_step(tr, &next_id, R.data(), t.data(), hdr[7] ? present.data() : nullptr, n_heads.data(), heads.data(), n_cams, hdr[6],
                    max_heads, hdr[2], hdr[3], hdr[4], ids.data(), &n_persons, persons);
        fwrite(tr, sizeof tr, 1, stdout);
        fwrite(&next_id, sizeof next_id, 1, stdout);
        fwrite(ids.data(), sizeof(uint32_t), ids.size(), stdout);
        fwrite(&n_persons, sizeof n_persons, 1, stdout);
        fwrite(persons, sizeof persons, 1, stdout);
        ++cases;
    }
    fprintf(stderr, "%d cases\n", cases);
    return cases > 0 ? 0 : 1;
}
