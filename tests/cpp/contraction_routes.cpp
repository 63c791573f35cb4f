// tests/test_contraction_routes_cpu.py: the instantiation lists and the request resolution of onnxstream_amd/csrc/osg_gemm_routes.h, printed for the Python side.
//   entries   one line per gemm2_kernel / conv3x3_kernel entry
//   rows      tune_row_ok over family 0-1 x cfg 0-63 x nst 0-8 x splits 0-65 x bn {0, 64, 80, 96, 128, 160}, one 0 / 1 each
//   resolve   resolve_v2 of every request (form bits, nch, cfg 0-7, nst 0-8, ks 1-2, fold, spec), resolve3 of every halo request
#include "osg_gemm_routes.h"
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace osg_mm;

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "entries")) {
        for (const V2Entry& e : kV2Entries)
            printf("v2 %d %d %d %d %d %d %d %d %d %d %d %d\n", e.bm, e.bn, e.nst, e.conv, e.spec, e.ln, e.nch, e.ks, e.wgn, e.wq, v2_tile(e), (int)v2_fold_capable(e));
        for (const V3Entry& e : kV3Entries) printf("v3 %d %d %d %d %d %d\n", e.w, e.bn, e.wgm, e.wgn, e.nlw, e.wq);
    } else if (!strcmp(mode, "rows")) {
        for (int family = 0; family < 2; family++)
            for (int cfg = 0; cfg < 64; cfg++)
                for (int nst = 0; nst <= 8; nst++)
                    for (int splits = 0; splits <= 65; splits++)
                        for (int bn : {0, 64, 80, 96, 128, 160}) putchar(tune_row_ok(family, cfg, nst, splits, bn) ? '1' : '0');
        putchar('\n');
    } else if (!strcmp(mode, "resolve")) {
        for (int fb = 0; fb < 64; fb++)   // form bits: conv 1, ln1 2, ln2 4, geglu 8, rowstats 16, w8 32
            for (int nch : {5, 10, 20}) {
                if (!(fb & 4) && nch != 5) continue;
                const V2Form f{(fb & 1) != 0, (fb & 2) != 0, (fb & 4) != 0, (fb & 8) != 0, (fb & 16) != 0, (fb & 32) != 0, nch};
                for (int cfg = 0; cfg < 8; cfg++)
                    for (int nst = 0; nst <= 8; nst++)
                        for (int ks = 1; ks <= 2; ks++)
                            for (int fold = 0; fold < 2; fold++)
                                for (int spec = 0; spec < 2; spec++) {
                                    const V2Route r = resolve_v2(V2Choice{cfg, nst, 2, ks, fold, spec}, f);
                                    printf("r %d %d %d %d %d %d %d %d %d\n", fb, nch, cfg, nst, ks, fold, spec, r.entry, (int)r.fold);
                                }
            }
        for (int w : {64, 32, 16, 8, 12})
            for (int bn : {0, 64, 80, 96, 128, 160})
                for (int nl : {0, 4, 8})
                    for (int w8 = 0; w8 < 2; w8++) printf("h %d %d %d %d %d\n", w, bn, nl, w8, resolve3(w, bn, nl, w8 != 0));
    }
    return 0;
}
