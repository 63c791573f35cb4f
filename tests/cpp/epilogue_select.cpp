// tests/test_epilogue_select_cpu.py: the lean epilogue variants and their selection (onnxstream_amd/csrc/osg_gemm_epi.h), for the Python side.
//   list      one line per entry of kLeanEntries: index, its index in kV2Entries, bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, mask
//   select    reads launches from standard input, one per line --
//               entry M N batch splits fold bias bias_f32 rowbias residual c2 rowstats sinks act other ldc ldc2 rb_ld rs_np align_or force_generic
//             -- and prints "select_epi epi_form epi_whole" for each
#include "osg_gemm_epi.h"
#include <cstdio>
#include <cstring>

using namespace osg_mm;

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "list")) {
        printf("bits %d %d %d %d %d %d %d %d %d %d %d %d any %d count %d\n", EPI_BIAS16, EPI_BIAS32, EPI_ROWBIAS, EPI_RESIDUAL, EPI_SILU, EPI_C2, EPI_ROWSTATS, EPI_SPLIT, EPI_FOLD,
               EPI_GEGLU, EPI_SINKS, EPI_OTHER, EPI_ANY, kV2Count);
        for (int i = 0; i < kLeanCount; i++) {
            const V2Entry& e = kLeanEntries[i].e;
            printf("lean %d %d %d %d %d %d %d %d %d %d %d %d %d\n", i, v2_index(e), e.bm, e.bn, e.nst, e.conv, e.spec, e.ln, e.nch, e.ks, e.wgn, e.wq, kLeanEntries[i].mask);
        }
        for (int i = 0; i < kV2Count; i++) {
            const V2Entry& e = kV2Entries[i];
            printf("v2 %d %d %d %d %d %d\n", i, e.bm, e.bn, e.ln, e.wgn, e.ks);
        }
    } else if (!strcmp(mode, "select")) {
        int entry, M, N, batch, splits, fold, bias, bias_f32, rowbias, residual, c2, rowstats, sinks, act, other, rs_np, force;
        long ldc, ldc2, rb_ld;
        unsigned long align_or;
        while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %ld %ld %ld %d %lu %d", &entry, &M, &N, &batch, &splits, &fold, &bias, &bias_f32, &rowbias, &residual, &c2, &rowstats,
                     &sinks, &act, &other, &ldc, &ldc2, &rb_ld, &rs_np, &align_or, &force) == 21) {
            EpiLaunch l;
            l.M = M; l.N = N; l.batch = batch; l.splits = splits; l.fold = fold != 0;
            l.bias = bias != 0; l.bias_f32 = bias_f32 != 0; l.rowbias = rowbias != 0; l.residual = residual != 0; l.c2 = c2 != 0; l.rowstats = rowstats != 0; l.sinks = sinks != 0;
            l.act = act; l.other = other != 0; l.ldc = ldc; l.ldc2 = ldc2; l.rb_ld = rb_ld; l.rs_np = rs_np; l.align_or = (uintptr_t)align_or;
            const bool in_range = entry >= 0 && entry < kV2Count;
            printf("%d %d %d\n", select_epi(entry, l, force != 0), epi_form(l), in_range ? (int)epi_whole(l, kV2Entries[entry].bm, kV2Entries[entry].bn) : 0);
        }
    } else {
        fprintf(stderr, "usage: %s list | select\n", argv[0]);
        return 2;
    }
    return 0;
}
