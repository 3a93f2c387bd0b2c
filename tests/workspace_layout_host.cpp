// The render workspace's layout header (csrc/mdvt_workspace.h) compiled for the host: prints what it answers, one line per case, for
// tests/test_workspace_layout_cpu.py to check.  Reads "W H" pairs from the command line:
//   workspace_layout_host 2x2 100x31 ...
// Per (size, slots in 1..32, huge_lists in {1, 2}) a line "L ..." of the fields named in kFields, then per bank_slots with
// 2 * bank_slots <= slots a line "B bank_slots bank_counters_at(1) coarse_at".
#include "mdvt_workspace.h"

#include <stdio.h>

static const char* const kFields =
    "W H slots huge_lists plane_bytes tri_invalid_bytes unused_bytes elist_bytes elist_count_at vlist_at vlist_count_at "
    "queue_bytes queue_slots bigq_cap counters_at counter_words huge_at huge_list_dwords tie_flag_at tie_tiles_at tie_words "
    "elist_stride queue_stride tie_tiles_stride queue_slots_max nominal nominal_edge_flags nominal_edge_points";

int main(int argc, char** argv)
{
    printf("F %s\n", kFields);
    for (int k = 1; k < argc; ++k) {
        int W = 0, H = 0;
        if (sscanf(argv[k], "%dx%d", &W, &H) != 2 || W < 2 || H < 2) { fprintf(stderr, "bad size %s\n", argv[k]); return 2; }
        for (int slots = 1; slots <= 32; ++slots)
            for (int hl = 1; hl <= 2; ++hl) {
                const mdvt::RenderWorkspaceLayout L(W, H, slots, hl);
                const size_t v[] = {L.W, L.H, L.slots, L.huge_lists, L.plane_bytes(), L.tri_invalid_bytes(), L.unused_bytes(), L.elist_bytes(),
                                    L.elist_count_at(), L.vlist_at(), L.vlist_count_at(), L.queue_bytes(), L.queue_slots(),
                                    L.bigq_cap(), L.counters_at(), L.counter_words(), L.huge_at(), L.huge_list_dwords(),
                                    L.tie_flag_at(), L.tie_tiles_at(), L.tie_words, L.elist_stride(),
                                    L.queue_stride(), L.tie_tiles_stride(), mdvt::queue_slots_max(W, H), mdvt::nominal_slot_bytes(W, H, false, false),
                                    mdvt::nominal_slot_bytes(W, H, false, true), mdvt::nominal_slot_bytes(W, H, true, true)};
                printf("L");
                for (size_t x : v) printf(" %zu", x);
                printf("\n");
                if (L.bank_counters_at(0, slots) != 0) { fprintf(stderr, "bank 0 does not start at the counters\n"); return 1; }
                for (int bs = 1; 2 * bs <= slots; ++bs)
                    printf("B %d %zu %zu\n", bs, L.bank_counters_at(1, bs), mdvt::queue_coarse_at(bs, H));
            }
    }
    return 0;
}
