// libosgpu: halo-reuse 3x3 / stride 1 / pad 1 convolution (the resnet convolutions: 55 % of an SD UNet pass).
//
// Measured on MI355X the implicit-GEMM kernel of osg_gemm.hip is bound by the per-CU L2->LDS path (~23 B/clk/CU), not by
// the MFMA pipe, and a 3x3 convolution run as a GEMM fetches every input pixel NINE times (once per filter tap).  Here a
// workgroup owns 128 consecutive output pixels (TH full rows of the image) x BN output channels and walks K as
// (64-channel slab) x (9 taps):
//   * the input PATCH of the slab -- (TH+2) x (W+2) pixels x 64 channels, zero halo supplied by the buffer descriptor's
//     bounds check -- is DMA'd into LDS ONCE and read by all 9 taps (A traffic / ~5);
//   * per (slab, tap) only the [BN][64] weight tile streams in: 4-deep LDS ring, counted vmcnt, ONE barrier per tap;
//   * the patch of the NEXT slab arrives piecewise during taps 0..4 of the current slab (double-buffered);
//   * both images are lane-linear 128-byte rows with the 16-byte chunk index XOR-swizzled by (row & 7) on the SOURCE address,
//     so every fragment read is a conflict-free ds_read_b128 (a fragment's 16 pixels are consecutive patch pixels);
//   * BN in {80, 128, 160}: 320 / 640 / 1280 output channels tile without padding; wave layouts 4x1 / 2x2 / 2x2.
// Arithmetic, accumulation order class and epilogue are those of the GEMM kernel (f16 operands, f32 accumulate on
// v_mfma_f32_16x16x32_f16, one RNE rounding): XnnPack::convolution, reference src/onnxstream.cpp:1292-1534.
#include "osg_conv3x3_kernel.h"

template <>
int osg_mm::launch3_unit<0>(int entry, osg_ctx* ctx, GemmParams& p) { return launch3_in_unit<0>(entry, ctx, p); }

// shape gate: -1 when the halo-reuse kernel does not take the shape (osg_gemm_select.h halo3_takes, OSG_CONV3X3_OFF, operands not 16-byte aligned); fills the
// buffer extents otherwise
int osg_conv3x3_prepare(osg_ctx* ctx, GemmParams& p) {
    static const bool off = getenv("OSG_CONV3X3_OFF") != nullptr;
    if (off || !halo3_takes(select_shape(p, 1))) return -1;
    if ((((uintptr_t)p.A | (uintptr_t)p.Bt) & 15) != 0) return -1;
    p.a_bytes = (unsigned)p.a_bytes_l;
    p.b_bytes = (unsigned)((long)p.N * p.K * (p.w8 ? 1 : 2));
    return 0;
}

// launch one configuration (reduce kernel included); p must have passed osg_conv3x3_prepare.  The request resolves to an instantiation first (osg_gemm_routes.h
// resolve3: 8 loader waves only where the ring stays deep enough, uint8 codes with 160 columns at W = 64 run 80), the split is sized for the tile that runs.
int osg_conv3x3_launch(osg_ctx* ctx, GemmParams p, Halo3Choice ch) {
    const int entry = resolve3(p.W, ch.bn, ch.loaders, p.w8 != 0);
    if (entry < 0) OSG_FAIL(ctx, "osg_conv3x3: no kernel takes this image width");
    const int bn = kV3Entries[entry].bn;
    const auto [slices, slabs_per] = split_slices(p.Cin / 64, ch.splits);
    p.splits = slices;
    p.k_per_split = slabs_per * 64;
    p.tickets = nullptr;
    p.fold_acc = 0;
    if (p.splits > 1) {
        size_t need = (size_t)p.splits * p.M * p.N * sizeof(float);
        if (ch.fold) need = std::max(need, osg_mm::splitk_fold_route(ctx, p, (long)((p.M + 127) / 128) * ((p.N + bn - 1) / bn), 128, bn));
        if (osg_ensure_workspace(ctx, need)) return 1;
        p.partial = (float*)ctx->ws;
    }
    p.n_major = (double)p.N * p.K * 2.0 > (double)p.a_bytes_l;
    if (const int rc = kV3Entries[entry].wq ? launch3_unit<1>(entry, ctx, p) : launch3_unit<0>(entry, ctx, p)) return rc;
    osg_set_route(ctx, 1, entry, p.splits, p.fold_acc);
    if (p.splits > 1 && !p.fold_acc) return launch_splitk_reduce(ctx, p, 1);
    return 0;
}

// the cost model's choice (osg_gemm_select.h model_halo3), then the per-call OSG_CONV3X3_* overrides
int osg_conv3x3_run(osg_ctx* ctx, GemmParams& p) {
    if (osg_conv3x3_prepare(ctx, p)) return -1;
    Halo3Choice ch = model_halo3(select_env(ctx), select_shape(p, 1));
    apply_knobs(kHalo3Knobs, &ch);
    return osg_conv3x3_launch(ctx, p, ch);
}
