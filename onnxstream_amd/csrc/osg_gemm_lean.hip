// libosgpu: the lean epilogue variants of gemm2_kernel -- kLeanEntries of osg_gemm_epi.h, each an entry of kV2Entries compiled for the one form of fused epilogue a
// launch of the headline plan runs it with.  A translation unit of their own, beside the four that instantiate the entries themselves, so the build stays parallel.
#include "osg_gemm2.h"

namespace {
template <int I>
constexpr V2Launch lean_launcher() {
    constexpr V2Entry e = kLeanEntries[I].e;
    return launch_v2<e.bm, e.bn, e.nst, e.conv != 0, 0, e.spec, e.ln, e.nch, e.ks, e.wgn, e.wq, kLeanEntries[I].mask>;
}
template <size_t... I>
constexpr std::array<V2Launch, kLeanCount> lean_launchers(std::index_sequence<I...>) { return {lean_launcher<(int)I>()...}; }
}  // namespace

int osg_mm::launch_v2_lean(int lean, osg_ctx* ctx, GemmParams& p, int batch) {
    static constexpr std::array<V2Launch, kLeanCount> table = lean_launchers(std::make_index_sequence<kLeanCount>{});
    if (lean < 0 || lean >= kLeanCount) OSG_FAIL(ctx, "osg_gemm: no such lean epilogue variant");
    return table[lean](ctx, p, batch);
}
