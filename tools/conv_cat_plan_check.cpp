// Stand-alone check of osg_conv3x3_cat_plan.h (no HIP, no GPU): build with the host sanitizers and run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I onnxstream_amd/csrc tools/conv_cat_plan_check.cpp -o conv_cat_plan_check && ./conv_cat_plan_check
// (`conv_cat_plan_check entries` prints the entry list of the header and checks nothing.)
// For every instantiation of osg_conv3x3_cat.hip x asked splits 1..5 x Cin2 / 64 in 1..40 x the slab counts of the nets (Cin / 64 in 1..40):
//   * the slices of cat_split / cat_slice cover every slab and every k-tile of the combined unit list exactly once, no slice starts behind the list's end,
//     and a slice's work stays less than one slab above the units per slice;
//   * the workgroup barriers the loader waves' path counts equal the math waves' path count, slice by slice;
//   * the LDS ring of the 1x1 phase fits 160 KiB, is at least 4 stages deep, and its counted waits fit the 6-bit vmcnt field.
#include <cstdio>
#include <string>
#include <vector>

#include "osg_conv3x3_cat_plan.h"

using namespace osg_mm;

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "entries") {   // the entry list, one "w bn wgm wgn nlw" line each (tests/test_conv_shortcut_gpu.py)
        for (const CatEntry& e : kCatEntries) printf("%d %d %d %d %d\n", e.w, e.bn, e.wgm, e.wgn, e.nlw);
        return 0;
    }
    long checked = 0;
    int bad = 0;
    for (const CatEntry& e : kCatEntries) {
        const int bst = cat_bst_bytes(e.bn, e.nlw);
        const int ns = cat_stages(bst), st = cat_stage_bytes(bst);
        const int lpu = kCatATileBytes / 1024 / e.nlw + bst / 1024 / e.nlw;
        if ((long)ns * st > kCatLdsBytes || ns < 4 || (ns - 2) * lpu > 63 || kCatATileBytes % (1024 * e.nlw)) {
            printf("entry W=%d BN=%d NLW=%d: ring of %d stages x %d bytes, %d loads per unit\n", e.w, e.bn, e.nlw, ns, st, lpu);
            bad++;
        }
        for (int slabs = 1; slabs <= 40; slabs++)
            for (int kt2 = 1; kt2 <= 40; kt2++)
                for (int asked = 1; asked <= 5; asked++) {
                    const CatSplit sp = cat_split(slabs, kt2, asked);
                    std::vector<int> slab_owner(slabs, 0), kt_owner(kt2, 0);
                    const int total = 9 * slabs + kt2;
                    if (sp.slices < 1 || sp.slices > asked || (sp.slices - 1) * sp.q >= total || sp.slices * sp.q < total) { printf("split %d %d %d: %d x %d\n", slabs, kt2, asked, sp.slices, sp.q); bad++; }
                    for (int z = 0; z < sp.slices; z++) {
                        const CatSlice s = cat_slice(slabs, kt2, sp.q, z);
                        if (s.slab_b < 0 || s.slab_e > slabs || s.slab_b > s.slab_e || s.kt_b < 0 || s.kt_e > kt2 || s.kt_b > s.kt_e) { printf("slice out of range\n"); bad++; continue; }
                        for (int j = s.slab_b; j < s.slab_e; j++) slab_owner[j]++;
                        for (int t = s.kt_b; t < s.kt_e; t++) kt_owner[t]++;
                        const int work = 9 * (s.slab_e - s.slab_b) + (s.kt_e - s.kt_b);
                        if (work > sp.q + 8) { printf("slice %d of (%d, %d, %d): %d units of %d\n", z, slabs, kt2, asked, work, sp.q); bad++; }
                        if (cat_barriers_loader(s) != cat_barriers_math(s)) { printf("barriers differ: slice %d of (%d, %d, %d)\n", z, slabs, kt2, asked); bad++; }
                        checked++;
                    }
                    for (int j = 0; j < slabs; j++) if (slab_owner[j] != 1) { printf("slab %d of (%d, %d, %d) has %d owners\n", j, slabs, kt2, asked, slab_owner[j]); bad++; }
                    for (int t = 0; t < kt2; t++) if (kt_owner[t] != 1) { printf("k-tile %d of (%d, %d, %d) has %d owners\n", t, slabs, kt2, asked, kt_owner[t]); bad++; }
                }
    }
    if (bad) { printf("FAILED: %d\n", bad); return 1; }
    printf("OK: %ld slices checked\n", checked);
    return 0;
}
