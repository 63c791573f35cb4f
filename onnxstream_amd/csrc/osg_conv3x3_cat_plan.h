// libosgpu: host-compilable arithmetic of the halo-reuse 3x3 convolution's second K segment (osg_conv3x3_kernel.h CAT = 1, osg_conv3x3_cat.hip): how the k-slices
// of a split divide the combined unit list, how the LDS is carved for the 1x1 phase, and how many workgroup barriers each role executes.  No HIP in here: the
// kernel, the launcher and tools/conv_cat_plan_check.cpp (a stand-alone program, built with the host sanitizers) read the same functions.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OSG_CAT_HD __host__ __device__
#else
#define OSG_CAT_HD
#endif

namespace osg_mm {

// ---- the instantiations of osg_conv3x3_cat.hip: (image width, output channels per tile, math waves as wgm x wgn, loader waves) -- the f16 combinations of the 3x3
// kernel's own entry list (8 loader waves where both rings stay deep enough).  One list: the unit instantiates it, tools/conv_cat_plan_check.cpp prints and checks
// it, tests/test_conv_shortcut_gpu.py reads the tool's print-out.
struct CatEntry { int w, bn, wgm, wgn, nlw; };
// clang-format off
inline constexpr CatEntry kCatEntries[] = {
    {64, 80, 4, 1, 4}, {64, 128, 2, 2, 4}, {64, 160, 2, 2, 4}, {64, 80, 4, 1, 8}, {64, 128, 2, 2, 8},
    {32, 80, 4, 1, 4}, {32, 128, 2, 2, 4}, {32, 160, 2, 2, 4}, {32, 80, 4, 1, 8}, {32, 128, 2, 2, 8}, {32, 160, 2, 2, 8},
    {16, 80, 4, 1, 4}, {16, 128, 2, 2, 4}, {16, 160, 2, 2, 4}, {16, 80, 4, 1, 8}, {16, 128, 2, 2, 8}, {16, 160, 2, 2, 8},
    {8, 80, 4, 1, 4},  {8, 128, 2, 2, 4},  {8, 160, 2, 2, 4},  {8, 80, 4, 1, 8},  {8, 128, 2, 2, 8},
};
// clang-format on
inline constexpr int kCatCount = sizeof(kCatEntries) / sizeof(kCatEntries[0]);
constexpr int cat_find(int w, int bn, int nlw) {
    for (int i = 0; i < kCatCount; i++)
        if (kCatEntries[i].w == w && kCatEntries[i].bn == bn && kCatEntries[i].nlw == nlw) return i;
    return -1;
}
// the entry a request runs (-1: an image width the kernel does not take): the rule of resolve3 (osg_gemm_routes.h)
constexpr int cat_resolve(int w, int bn, int loader_waves) {
    if (bn != 80 && bn != 160) bn = 128;
    const int e = loader_waves == 8 ? cat_find(w, bn, 8) : -1;
    return e >= 0 ? e : cat_find(w, bn, 4);
}
// one f16 weight stage of the 3x3 phase: whole rounds of the loader waves over the tile's 8-row, 1-KiB wave-loads (osg_conv3x3_kernel.h asserts Geo::BST_BYTES equals it)
OSG_CAT_HD constexpr int cat_bst_bytes(int bn, int nlw) { return ((bn + 7) / 8 + nlw - 1) / nlw * nlw * 1024; }

// ---- the combined unit list: slab j of the 3x3 part is the 9 tap units 9j .. 9j + 8, k-tile t of the 1x1 part is unit 9 * slabs + t.  Slice z owns the units
// [z * q, (z + 1) * q).  A slab is never cut (its patch is loaded once and read by all 9 taps): it belongs to the slice that owns its MIDDLE unit 9j + 4, so a
// slice carries at most ceil(q / 9) slabs: less than one slab more than q units.  A k-tile belongs to the slice that owns its unit.  Every slab and every k-tile has exactly one owner; a
// slice may hold slabs, k-tiles, both, or (q < 9) nothing at all -- it then stores a tile of zeros, like an empty slice of any other split.
struct CatSlice { int slab_b, slab_e, kt_b, kt_e; };
OSG_CAT_HD constexpr int cat_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
OSG_CAT_HD constexpr CatSlice cat_slice(int slabs, int kt2, int q, int zs) {
    const int ub = zs * q, ue = ub + q;
    return {cat_clamp((ub + 4) / 9, 0, slabs), cat_clamp((ue + 4) / 9, 0, slabs), cat_clamp(ub - 9 * slabs, 0, kt2), cat_clamp(ue - 9 * slabs, 0, kt2)};
}
// "ask for `asked` slices": {slices that run, units per slice}; no slice starts behind the end of the list
struct CatSplit { int slices, q; };
constexpr CatSplit cat_split(int slabs, int kt2, int asked) {
    const int total = 9 * slabs + kt2;
    const int a = asked < 1 ? 1 : asked;
    const int q = (total + a - 1) / a;
    return {(total + q - 1) / q, q};
}

// ---- workgroup barriers of one slice, per role.  Both roles: one behind the prologue of the 3x3 phase and one per (slab, tap) unit; where the slice holds k-tiles,
// one that separates the two carvings of the LDS, one behind the prologue of the 1x1 phase and one per k-tile; then one behind the loaders' last vmcnt(0).  (The barrier of the GroupNorm-statistics epilogue
// comes after the loader waves have left and is not counted here.)
constexpr int cat_barriers_loader(const CatSlice& s) {
    int n = 1;                                              // prologue of the 3x3 phase
    for (int slab = s.slab_b; slab < s.slab_e; slab++) n += 9;
    if (s.kt_b < s.kt_e) {
        n += 1;                                             // the math waves are done with the patches and the weight ring
        n += 1;                                             // prologue of the 1x1 phase
        for (int kt = s.kt_b; kt < s.kt_e; kt++) n += 1;
    }
    return n + 1;                                           // behind vmcnt(0): every DMA of the workgroup has landed
}
constexpr int cat_barriers_math(const CatSlice& s) {
    int n = 1 + 9 * (s.slab_e > s.slab_b ? s.slab_e - s.slab_b : 0);
    if (s.kt_e > s.kt_b) n += 2 + (s.kt_e - s.kt_b);
    return n + 1;                                           // the LDS is quiet: the epilogue (statistics staging) may reuse it
}

// ---- LDS of the 1x1 phase: a ring of stages, each the A tile (128 pixels x 64 channels of f16) followed by one weight stage of the 3x3 phase's size
constexpr int kCatLdsBytes = 160 * 1024;
constexpr int kCatATileBytes = 128 * 64 * 2;
OSG_CAT_HD constexpr int cat_stage_bytes(int bst_bytes) { return kCatATileBytes + bst_bytes; }
OSG_CAT_HD constexpr int cat_stages(int bst_bytes) {
    const int n = kCatLdsBytes / cat_stage_bytes(bst_bytes);
    return n > 8 ? 8 : n;
}

}  // namespace osg_mm
