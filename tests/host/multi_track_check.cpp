// The multi-head tracker step (depthhead_amd/csrc/dh_track_heads.h) on the host, for tests/test_multi_track_rule.py.  Reads
// cases from stdin, binary: six u32 (max_heads, n_heads, gate, max_misses, next_id, present), then DH_MAX_TRACKS dh_head_track
// records and max_heads dh_head records.  For each it applies what one lane of k_track_heads applies and writes the records
// after the step, next_id and max_heads u32 ids.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dh_track_heads.h"

int main() {
    uint32_t hdr[6];
    int cases = 0;
    while (fread(hdr, sizeof hdr, 1, stdin) == 1) {
        const int max_heads = (int)hdr[0];
        if (max_heads < 1 || max_heads > DH_MAX_HEADS) { fprintf(stderr, "max_heads %d\n", max_heads); return 1; }
        dh_head_track tr[DH_MAX_TRACKS];
        std::vector<dh_head> heads((size_t)max_heads);
        std::vector<uint32_t> ids((size_t)max_heads, 0xdeadbeefu);
        if (fread(tr, sizeof tr, 1, stdin) != 1 || fread(heads.data(), sizeof(dh_head), heads.size(), stdin) != heads.size()) {
            fprintf(stderr, "truncated case %d\n", cases);
            return 1;
        }
        uint32_t next_id = hdr[4];
        if (hdr[5]) dh_track_heads_step(tr, &next_id, heads.data(), hdr[1], max_heads, hdr[2], hdr[3], ids.data());
        else for (int j = 0; j < max_heads; ++j) ids[(size_t)j] = 0;
        fwrite(tr, sizeof tr, 1, stdout);
        fwrite(&next_id, sizeof next_id, 1, stdout);
        fwrite(ids.data(), sizeof(uint32_t), ids.size(), stdout);
        ++cases;
    }
    fprintf(stderr, "%d cases\n", cases);
    return cases > 0 ? 0 : 1;
}
