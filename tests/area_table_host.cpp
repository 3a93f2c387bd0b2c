// area_table_host.cpp -- csrc/mdvt_area_table.h in a program of its own: tests/test_megasam_cpu.py compiles it at test time (plain, and
// with -fsanitize=address,undefined where the compiler has the runtime), runs it directly and compares the tables it writes with the
// restatement's (tests/megasam_ref.py).
//
//   area_table_host <results file> <in> <out> [<in> <out> ...]
//
// Per pair the results file holds 32-bit words: status (1 built, 0 refused), in, out, ktaps, first[out], count[out], then the bits of
// the float32 weights w[out][ktaps].
#include <stdio.h>
#include <stdlib.h>

#include "mdvt_area_table.h"

int main(int argc, char** argv)
{
    if (argc < 4 || argc % 2 != 0) {
        fprintf(stderr, "usage: %s <results file> <in> <out> [<in> <out> ...]\n", argv[0]);
        return 2;
    }
    FILE* fh = fopen(argv[1], "wb");
    if (!fh) return 3;
    for (int k = 2; k + 1 < argc; k += 2) {
        mdvt::host::AreaTable t;
        const int in = atoi(argv[k]), out = atoi(argv[k + 1]);
        const bool ok = mdvt::host::build_area_table(in, out, t);
        const int32_t head[4] = {ok ? 1 : 0, in, out, ok ? t.ktaps : 0};
        fwrite(head, sizeof head, 1, fh);
        if (ok) {
            fwrite(t.first.data(), sizeof(int32_t), t.first.size(), fh);
            fwrite(t.count.data(), sizeof(int32_t), t.count.size(), fh);
            fwrite(t.w.data(), sizeof(float), t.w.size(), fh);
        }
    }
    return fclose(fh) == 0 ? 0 : 4;
}
