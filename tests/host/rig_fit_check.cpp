// The bind of a rig fit tracker's step (depthhead_amd/csrc/dh_rig_fit.h) on the host, for tests/test_rig_fit_rule.py.  Reads
// cases from stdin, binary: three u32 (n_persons, n_cams, max_heads), then DH_RIG_MAX_TRACKS dh_rig_fit_state records,
// DH_RIG_MAX_PERSONS dh_rig_person records and n_heads [n_cams] u32.  For each it runs dh_rig_fit_bind, the sequential
// statement of what lane 0 of k_rig_fit_seed's workgroup does, and writes the entries after the bind and the role and the
// person of every slot.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dh_rig_fit.h"

int main() {
    uint32_t hdr[3];
    int cases = 0;
    while (fread(hdr, sizeof hdr, 1, stdin) == 1) {
        const int n_cams = (int)hdr[1], max_heads = (int)hdr[2];
        if (n_cams < 1 || n_cams > 4096 || max_heads < 1 || max_heads > DH_MAX_HEADS) {
            fprintf(stderr, "n_cams %d max_heads %d\n", n_cams, max_heads);
            return 1;
        }
        dh_rig_fit_state st[DH_RIG_MAX_TRACKS];
        dh_rig_person persons[DH_RIG_MAX_PERSONS];
        std::vector<uint32_t> n_heads((size_t)n_cams);
        if (fread(st, sizeof st, 1, stdin) != 1 || fread(persons, sizeof persons, 1, stdin) != 1 ||
            fread(n_heads.data(), sizeof(uint32_t), n_heads.size(), stdin) != n_heads.size()) {
            fprintf(stderr, "truncated case %d\n", cases);
            return 1;
        }
        uint32_t role[DH_RIG_MAX_TRACKS], person[DH_RIG_MAX_TRACKS];
        memset(role, 0xee, sizeof role);
        memset(person, 0xee, sizeof person);
        dh_rig_fit_bind(st, persons, hdr[0], n_heads.data(), n_cams, max_heads, role, person);
        fwrite(st, sizeof st, 1, stdout);
        fwrite(role, sizeof role, 1, stdout);
        fwrite(person, sizeof person, 1, stdout);
        ++cases;
    }
    fprintf(stderr, "%d cases\n", cases);
    return cases > 0 ? 0 : 1;
}
