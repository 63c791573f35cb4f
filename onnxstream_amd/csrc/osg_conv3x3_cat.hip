// libosgpu: the halo-reuse 3x3 convolution with a second K segment (osg_conv3x3_kernel.h, CAT = 1): out = f16(W (*) h + W2 . x2 + bias), one launch for a ResNet's
// conv2 and its 1x1 conv_shortcut.  The 3x3 part is the kernel of osg_conv3x3.hip; behind its last (slab, tap) unit the same workgroup walks Cin2 / 64 k-tiles of
// x2 [M][Cin2] against W2 [N][Cin2] into the same accumulators, and the epilogue runs once -- the shortcut's launch, the store and re-load of its output and one
// f16 rounding are gone.  f16 weights only.
#include "osg_conv3x3_kernel.h"

namespace {

// (the instantiations of this unit, kCatEntries, and the request -> entry rule live in osg_conv3x3_cat_plan.h: host tools and tests read the same list)
using CatLaunch = int (*)(osg_ctx*, GemmParams&, const CatArgs*);
template <size_t... I>
constexpr std::array<CatLaunch, kCatCount> cat_launchers(std::index_sequence<I...>) {
    return {launch3_any<kCatEntries[I].w, kCatEntries[I].bn, kCatEntries[I].wgm, kCatEntries[I].wgn, 0, kCatEntries[I].nlw, 0, 1>...};
}

}  // namespace

extern "C" int osg_conv3x3_cat_entries(void) { return kCatCount; }

// launch one configuration (reduce kernel included).  p: the 3x3 convolution as osg_conv3x3_prepare passed it; (x2, w2, Cin2): the second segment.  The k-slices
// divide the combined unit list (osg_conv3x3_cat_plan.h).
int osg_conv3x3_cat_launch(osg_ctx* ctx, GemmParams p, const void* x2, const void* w2, int Cin2, Halo3Choice ch) {
    static constexpr std::array<CatLaunch, kCatCount> table = cat_launchers(std::make_index_sequence<kCatCount>{});
    // A split of this launch is always finished by the reduce launch; ch.fold is not honoured.  The in-kernel fold (splitk_fold_acc) returned non-finite sums from
    // the 64-wide / 128-column / 8-loader-wave instantiation of this kernel on MI355X while every other instantiation folded correctly and the un-fused kernel folds at
    // the same register budget; the cause is not known, so no instantiation of this unit is trusted with it.
    const int entry = cat_resolve(p.W, ch.bn, ch.loaders);
    if (entry < 0) OSG_FAIL(ctx, "osg_conv2d_nhwc_cat: no kernel takes this image width");
    if (Cin2 <= 0 || Cin2 % 64) OSG_FAIL(ctx, "osg_conv2d_nhwc_cat: Cin2 must be a multiple of 64");
    if ((((uintptr_t)x2 | (uintptr_t)w2) & 15) != 0) OSG_FAIL(ctx, "osg_conv2d_nhwc_cat: the second operand pair must be 16-byte aligned");
    if ((double)p.M * Cin2 * 2.0 >= 2147483648.0 || (double)p.N * Cin2 * 2.0 >= 2147483648.0) OSG_FAIL(ctx, "osg_conv2d_nhwc_cat: the second operand pair must be smaller than 2 GiB each");
    const CatArgs cat{x2, w2, Cin2, (unsigned)((long)p.M * Cin2 * 2), (unsigned)((long)p.N * Cin2 * 2)};
    const CatSplit sp = cat_split(p.Cin / 64, Cin2 / 64, ch.splits);
    p.splits = sp.slices;
    p.k_per_split = sp.q;          // (units of the combined list per slice: conv3x3_body CAT)
    p.tickets = nullptr;
    p.fold_acc = 0;
    if (p.splits > 1) {
        if (osg_ensure_workspace(ctx, (size_t)p.splits * p.M * p.N * sizeof(float))) return 1;
        p.partial = (float*)ctx->ws;
    }
    p.n_major = (double)p.N * (p.K + Cin2) * 2.0 > (double)p.a_bytes_l + (double)p.M * Cin2 * 2.0;
    if (const int rc = table[entry](ctx, p, &cat)) return rc;
    osg_set_route(ctx, 4, entry, p.splits, p.fold_acc);
    if (p.splits > 1 && !p.fold_acc) return launch_splitk_reduce(ctx, p, 1);
    return 0;
}
