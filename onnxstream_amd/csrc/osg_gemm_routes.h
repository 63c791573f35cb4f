// libosgpu: which instantiations of the contraction kernels exist, and what a launch request runs -- the one list and the one resolution that the cost model and
// the tuner (osg_gemm_select.h rank_v2), the tune-table loader (osg_ctx.hip), the launchers (osg_gemm.hip launch_v2_choice, osg_conv3x3.hip osg_conv3x3_launch) and the
// split-K fold sizing all read.  Host-only C++17 (no HIP): tests/cpp/contraction_routes.cpp compiles it with g++.
//
// A request names a tile, a ring depth and options; a form it asks for that has no instantiation runs the nearest one that does, by the fixed rules of resolve_v2 /
// resolve3 (the shipped tune table holds rows that depend on them: LayerNorm rows on tile 3 run 64 x 64, GEGLU-LayerNorm rows with nst 6 run a 2-stage ring).  The
// split-K workspace and the fold's ticket range are sized from the RESOLVED entry's tile.
#pragma once

namespace osg_mm {

// tiles of the direct-to-LDS kernel (tune cfg & 7): 0-3 the 128 / 64-row tiles of rounds 2-5, 4-7 the 160- / 80-column tiles of round 6 (measured candidates only)
inline constexpr int kV2BM[8] = {128, 128, 64, 64, 128, 128, 64, 64}, kV2BN[8] = {128, 64, 64, 128, 160, 80, 80, 160};

// one gemm2_kernel instantiation: its template arguments (MODE is 0 in every one)
struct V2Entry { int bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq; };

// clang-format off
inline constexpr V2Entry kV2Entries[] = {
    // f16, tiles 0-3 (osg_gemm.hip).                     BM   BN NST CONV SPEC LN NCH KS WGN WQ
    // plain GEMM and implicit-GEMM convolution
    {128, 128, 2, 0, 0, 0, 5, 1, 2, 0}, {128, 128, 4, 0, 0, 0, 5, 1, 2, 0}, {128, 128, 2, 1, 0, 0, 5, 1, 2, 0}, {128, 128, 4, 1, 0, 0, 5, 1, 2, 0},
    {128, 64, 2, 0, 0, 0, 5, 1, 2, 0},  {128, 64, 4, 0, 0, 0, 5, 1, 2, 0},  {128, 64, 6, 0, 0, 0, 5, 1, 2, 0},
    {128, 64, 2, 1, 0, 0, 5, 1, 2, 0},  {128, 64, 4, 1, 0, 0, 5, 1, 2, 0},  {128, 64, 6, 1, 0, 0, 5, 1, 2, 0},
    {64, 64, 2, 0, 0, 0, 5, 1, 2, 0},   {64, 64, 4, 0, 0, 0, 5, 1, 2, 0},   {64, 64, 6, 0, 0, 0, 5, 1, 2, 0},   {64, 64, 8, 0, 0, 0, 5, 1, 2, 0},
    {64, 64, 2, 1, 0, 0, 5, 1, 2, 0},   {64, 64, 4, 1, 0, 0, 5, 1, 2, 0},   {64, 64, 6, 1, 0, 0, 5, 1, 2, 0},   {64, 64, 8, 1, 0, 0, 5, 1, 2, 0},
    {64, 128, 2, 0, 0, 0, 5, 1, 2, 0},  {64, 128, 4, 0, 0, 0, 5, 1, 2, 0},  {64, 128, 6, 0, 0, 0, 5, 1, 2, 0},
    {64, 128, 2, 1, 0, 0, 5, 1, 2, 0},  {64, 128, 4, 1, 0, 0, 5, 1, 2, 0},  {64, 128, 6, 1, 0, 0, 5, 1, 2, 0},
    // KS = 2: two wave groups on alternating k-tiles
    {128, 64, 2, 0, 0, 0, 5, 2, 2, 0},  {64, 64, 2, 0, 0, 0, 5, 2, 2, 0},   {64, 64, 4, 0, 0, 0, 5, 2, 2, 0},
    {128, 64, 2, 1, 0, 0, 5, 2, 2, 0},  {64, 64, 2, 1, 0, 0, 5, 2, 2, 0},   {64, 64, 4, 1, 0, 0, 5, 2, 2, 0},
    {128, 64, 2, 0, 0, 2, 5, 2, 2, 0},  {64, 64, 2, 0, 0, 2, 5, 2, 2, 0},   {64, 64, 4, 0, 0, 2, 5, 2, 2, 0},
    {128, 64, 2, 0, 0, 2, 10, 2, 2, 0}, {64, 64, 2, 0, 0, 2, 10, 2, 2, 0},  {64, 64, 4, 0, 0, 2, 10, 2, 2, 0},
    {128, 64, 2, 0, 0, 2, 20, 2, 2, 0}, {64, 64, 2, 0, 0, 2, 20, 2, 2, 0},  {64, 64, 4, 0, 0, 2, 20, 2, 2, 0},
    // SPEC: four loader waves beside the four math waves
    {128, 128, 4, 0, 1, 0, 5, 1, 2, 0}, {128, 128, 4, 0, 1, 2, 5, 1, 2, 0}, {128, 128, 4, 0, 1, 2, 10, 1, 2, 0}, {128, 128, 4, 0, 1, 2, 20, 1, 2, 0},
    // LayerNorm folded in: LN = 1 row statistics beside the MFMAs, LN = 2 handed over by the producer of A (NCH: chunks of them)
    {128, 128, 2, 0, 0, 1, 5, 1, 2, 0}, {128, 128, 4, 0, 0, 1, 5, 1, 2, 0}, {128, 64, 2, 0, 0, 1, 5, 1, 2, 0},  {128, 64, 4, 0, 0, 1, 5, 1, 2, 0},
    {64, 64, 2, 0, 0, 1, 5, 1, 2, 0},   {64, 64, 4, 0, 0, 1, 5, 1, 2, 0},
    {128, 128, 2, 0, 0, 2, 5, 1, 2, 0}, {128, 128, 4, 0, 0, 2, 5, 1, 2, 0}, {128, 64, 2, 0, 0, 2, 5, 1, 2, 0},  {128, 64, 4, 0, 0, 2, 5, 1, 2, 0},
    {64, 64, 2, 0, 0, 2, 5, 1, 2, 0},   {64, 64, 4, 0, 0, 2, 5, 1, 2, 0},
    {128, 128, 2, 0, 0, 2, 10, 1, 2, 0}, {128, 128, 4, 0, 0, 2, 10, 1, 2, 0}, {128, 64, 2, 0, 0, 2, 10, 1, 2, 0}, {128, 64, 4, 0, 0, 2, 10, 1, 2, 0},
    {64, 64, 2, 0, 0, 2, 10, 1, 2, 0},  {64, 64, 4, 0, 0, 2, 10, 1, 2, 0},
    {128, 128, 2, 0, 0, 2, 20, 1, 2, 0}, {128, 128, 4, 0, 0, 2, 20, 1, 2, 0}, {128, 64, 2, 0, 0, 2, 20, 1, 2, 0}, {128, 64, 4, 0, 0, 2, 20, 1, 2, 0},
    {64, 64, 2, 0, 0, 2, 20, 1, 2, 0},  {64, 64, 4, 0, 0, 2, 20, 1, 2, 0},

    // f16, tiles 4-7 (osg_gemm_wide.hip): the waves as 4 x 1 on the 128 x 160 / 128 x 80 / 64 x 80 tiles, 2 x 2 on 64 x 160
    {128, 160, 2, 0, 0, 0, 5, 1, 1, 0}, {128, 160, 4, 0, 0, 0, 5, 1, 1, 0}, {128, 80, 2, 0, 0, 0, 5, 1, 1, 0},  {128, 80, 4, 0, 0, 0, 5, 1, 1, 0},
    {64, 80, 2, 0, 0, 0, 5, 1, 1, 0},   {64, 80, 4, 0, 0, 0, 5, 1, 1, 0},   {64, 80, 6, 0, 0, 0, 5, 1, 1, 0},
    {64, 160, 2, 0, 0, 0, 5, 1, 2, 0},  {64, 160, 4, 0, 0, 0, 5, 1, 2, 0},
    {128, 160, 4, 1, 0, 0, 5, 1, 1, 0}, {128, 80, 4, 1, 0, 0, 5, 1, 1, 0},  {64, 80, 4, 1, 0, 0, 5, 1, 1, 0},
    {128, 160, 4, 0, 1, 0, 5, 1, 1, 0}, {128, 160, 4, 0, 1, 2, 5, 1, 1, 0}, {128, 160, 4, 0, 1, 2, 10, 1, 1, 0}, {128, 160, 4, 0, 1, 2, 20, 1, 1, 0},
    {128, 160, 2, 0, 0, 2, 5, 1, 1, 0}, {128, 160, 4, 0, 0, 2, 5, 1, 1, 0}, {64, 160, 2, 0, 0, 2, 5, 1, 2, 0},  {64, 160, 4, 0, 0, 2, 5, 1, 2, 0},
    {128, 160, 2, 0, 0, 2, 10, 1, 1, 0}, {128, 160, 4, 0, 0, 2, 10, 1, 1, 0}, {64, 160, 2, 0, 0, 2, 10, 1, 2, 0}, {64, 160, 4, 0, 0, 2, 10, 1, 2, 0},
    {128, 160, 2, 0, 0, 2, 20, 1, 1, 0}, {128, 160, 4, 0, 0, 2, 20, 1, 1, 0}, {64, 160, 2, 0, 0, 2, 20, 1, 2, 0}, {64, 160, 4, 0, 0, 2, 20, 1, 2, 0},

    // uint8 weight codes, WQ = 1 (osg_gemm_w8.hip: GEMM; osg_gemm_w8_conv.hip: implicit-GEMM convolution)
    {128, 128, 2, 0, 0, 0, 5, 1, 2, 1}, {128, 128, 4, 0, 0, 0, 5, 1, 2, 1}, {128, 64, 2, 0, 0, 0, 5, 1, 2, 1},  {128, 64, 4, 0, 0, 0, 5, 1, 2, 1},
    {128, 64, 6, 0, 0, 0, 5, 1, 2, 1},  {64, 64, 2, 0, 0, 0, 5, 1, 2, 1},   {64, 64, 4, 0, 0, 0, 5, 1, 2, 1},   {64, 64, 8, 0, 0, 0, 5, 1, 2, 1},
    {64, 128, 2, 0, 0, 0, 5, 1, 2, 1},  {64, 128, 4, 0, 0, 0, 5, 1, 2, 1},  {128, 160, 2, 0, 0, 0, 5, 1, 1, 1}, {128, 160, 4, 0, 0, 0, 5, 1, 1, 1},
    {128, 80, 2, 0, 0, 0, 5, 1, 1, 1},  {128, 80, 4, 0, 0, 0, 5, 1, 1, 1},  {64, 80, 2, 0, 0, 0, 5, 1, 1, 1},   {64, 80, 4, 0, 0, 0, 5, 1, 1, 1},
    {64, 80, 6, 0, 0, 0, 5, 1, 1, 1},   {64, 160, 2, 0, 0, 0, 5, 1, 2, 1},  {64, 160, 4, 0, 0, 0, 5, 1, 2, 1},
    {128, 128, 2, 1, 0, 0, 5, 1, 2, 1}, {128, 128, 4, 1, 0, 0, 5, 1, 2, 1}, {128, 64, 2, 1, 0, 0, 5, 1, 2, 1},  {128, 64, 4, 1, 0, 0, 5, 1, 2, 1},
    {64, 64, 2, 1, 0, 0, 5, 1, 2, 1},   {64, 64, 4, 1, 0, 0, 5, 1, 2, 1},   {128, 160, 4, 1, 0, 0, 5, 1, 1, 1}, {128, 80, 4, 1, 0, 0, 5, 1, 1, 1},
    {64, 80, 4, 1, 0, 0, 5, 1, 1, 1},
};
// clang-format on
inline constexpr int kV2Count = sizeof(kV2Entries) / sizeof(kV2Entries[0]);

constexpr int v2_tile(const V2Entry& e) {
    for (int t = 0; t < 8; t++)
        if (kV2BM[t] == e.bm && kV2BN[t] == e.bn) return t;
    return -1;
}
// the translation unit that instantiates the entry (launch_v2_unit<U>): 0 osg_gemm.hip, 1 osg_gemm_wide.hip, 2 osg_gemm_w8.hip, 3 osg_gemm_w8_conv.hip
constexpr int v2_unit(const V2Entry& e) { return e.wq ? (e.conv ? 3 : 2) : (v2_tile(e) >= 4 ? 1 : 0); }
// can a split-K launch of the entry finish with splitk_fold_acc (the plain 256-thread kernel's protocol, on tiles of at most 10 accumulator quads per lane)?
// Otherwise the reduce launch finishes it.
constexpr bool v2_fold_capable(const V2Entry& e) {
    const int t = v2_tile(e);
    return e.ks == 1 && !e.spec && e.ln == 0 && t != 0 && t != 4 && t != 7;
}

// what a launch asks of a tile / ring / split-K choice (ks = 2: two wave groups; fold: split-K finished by splitk_fold_acc; spec: four loader waves)
struct V2Choice { int cfg, nst, splits, ks = 1, fold = 0, spec = 0; };
// ... and what it needs of an instantiation.  nch: the LN = 2 chunk count (v2_nch of the row-statistics slots).
struct V2Form { bool conv = false, ln1 = false, ln2 = false, geglu = false, rowstats = false, w8 = false; int nch = 5; };
constexpr int v2_nch(int rs_np) { return rs_np / 2 <= 5 ? 5 : rs_np / 2 <= 10 ? 10 : 20; }

// the entry that is (tile, nst, spec, ks) for this form as it stands, -1 if none.  GEGLU's value / gate pairs and the row statistics' 32-column slots need a
// wave's columns to be a multiple of 32 (not the 80-column waves of tiles 5-7).
constexpr int v2_find(const V2Form& f, int tile, int nst, int spec, int ks) {
    if (tile < 0 || tile > 7) return -1;
    const int ln = f.ln2 ? 2 : f.ln1 ? 1 : 0, nch = ln == 2 ? f.nch : 5;
    for (int i = 0; i < kV2Count; i++) {
        const V2Entry& e = kV2Entries[i];
        if (e.bm == kV2BM[tile] && e.bn == kV2BN[tile] && e.nst == nst && e.conv == (int)f.conv && e.spec == spec && e.ln == ln && e.nch == nch && e.ks == ks &&
            e.wq == (int)f.w8 && (!(f.geglu || f.rowstats) || (e.bn / e.wgn) % 32 == 0))
            return i;
    }
    return -1;
}
// does the cost model offer (tile, nst) for this form (rank_v2)?  The f16 tiles 0-3 at the rings of the plain GEMM (a folded-LayerNorm form then runs what
// resolve_v2 makes of it), the other tiles only with an instantiation of the form itself.
constexpr bool v2_holds(const V2Form& f, int tile, int nst) { return v2_find(!f.w8 && tile < 4 ? V2Form{} : f, tile, nst, 0, 1) >= 0; }

// the entry a request runs, and whether its split finishes in the kernel (entry -1: no kernel takes the form -- LayerNorm or row statistics with uint8 codes,
// LayerNorm in a convolution).  The fall-backs, as the launchers have always taken them:
//   uint8 codes: KS and spec ignored; a (tile, ring) the WQ = 1 set does not hold for the form runs the 128 x 128 / 64 x 64 tile (same BM) with 4 stages.
//   f16, tiles 4-7: spec where an entry has it, else without; a form they do not hold runs tile 0 / 2 (same BM) with ring 2 -> 2, else 4, no KS, no spec.
//   f16, tiles 0-3: LayerNorm on tile 3 runs tile 2; KS = 2 on tile 1 (2 stages) and tile 2 (>= 4 -> 4, else 2), not with LN = 1; spec where an entry has it;
//   then the ring asked for where the form has it, else 2 stages.
//   fold: asked for with KS = 1, on an entry that is fold-capable.
struct V2Route { int entry = -1; bool fold = false; };
constexpr V2Route resolve_v2(const V2Choice& ch, const V2Form& f) {
    if (ch.cfg < 0 || ch.cfg > 7) return {};
    int e = -1;
    if (f.w8) {
        if (f.ln1 || f.ln2 || f.rowstats) return {};
        e = v2_find(f, ch.cfg, ch.nst, 0, 1);
        if (e < 0) e = v2_find(f, kV2BM[ch.cfg] == 128 ? 0 : 2, 4, 0, 1);
    } else {
        int tile = ch.cfg, nst = ch.nst, ks = ch.ks, spec = ch.spec;
        if (tile >= 4) {
            if (spec) e = v2_find(f, tile, nst, 1, 1);
            if (e < 0) e = v2_find(f, tile, nst, 0, 1);
            if (e < 0) { tile = kV2BM[tile] == 128 ? 0 : 2; nst = nst == 2 ? 2 : 4; ks = 1; spec = 0; }
        }
        if (e < 0) {
            if ((f.ln1 || f.ln2) && tile == 3) tile = 2;
            if (ks == 2 && (tile == 1 || tile == 2) && !f.ln1) e = v2_find(f, tile, tile == 2 && nst >= 4 ? 4 : 2, 0, 2);
            if (e < 0 && spec) e = v2_find(f, tile, nst, 1, 1);
            if (e < 0) e = v2_find(f, tile, nst, 0, 1);
            if (e < 0) e = v2_find(f, tile, 2, 0, 1);
        }
    }
    return {e, e >= 0 && ch.fold && ch.ks == 1 && v2_fold_capable(kV2Entries[e])};
}

// one conv3x3_kernel instantiation (the halo-reuse 3x3 convolution): image width, output channels per tile, the math waves as wgm x wgn, loader waves, uint8 codes
struct V3Entry { int w, bn, wgm, wgn, nlw, wq; };
// clang-format off
inline constexpr V3Entry kV3Entries[] = {
    // f16 weights (osg_conv3x3.hip): 4 loader waves; 8 where the wider stages still leave a deep enough ring (Geo<W, BN, 8>::OK: not 160 columns at W = 64 / 8)
    {64, 80, 4, 1, 4, 0}, {64, 128, 2, 2, 4, 0}, {64, 160, 2, 2, 4, 0}, {64, 80, 4, 1, 8, 0}, {64, 128, 2, 2, 8, 0},
    {32, 80, 4, 1, 4, 0}, {32, 128, 2, 2, 4, 0}, {32, 160, 2, 2, 4, 0}, {32, 80, 4, 1, 8, 0}, {32, 128, 2, 2, 8, 0}, {32, 160, 2, 2, 8, 0},
    {16, 80, 4, 1, 4, 0}, {16, 128, 2, 2, 4, 0}, {16, 160, 2, 2, 4, 0}, {16, 80, 4, 1, 8, 0}, {16, 128, 2, 2, 8, 0}, {16, 160, 2, 2, 8, 0},
    {8, 80, 4, 1, 4, 0},  {8, 128, 2, 2, 4, 0},  {8, 160, 2, 2, 4, 0},  {8, 80, 4, 1, 8, 0},  {8, 128, 2, 2, 8, 0},
    // uint8 weight codes (osg_conv3x3_w8.hip): 4 loader waves; no 160 columns at W = 64 (one register short with the code registers of the B pipeline, and 128
    // tiles for 256 CUs at the only width it divides, 320)
    {64, 80, 4, 1, 4, 1}, {64, 128, 2, 2, 4, 1},
    {32, 80, 4, 1, 4, 1}, {32, 128, 2, 2, 4, 1}, {32, 160, 2, 2, 4, 1},
    {16, 80, 4, 1, 4, 1}, {16, 128, 2, 2, 4, 1}, {16, 160, 2, 2, 4, 1},
    {8, 80, 4, 1, 4, 1},  {8, 128, 2, 2, 4, 1},  {8, 160, 2, 2, 4, 1},
};
// clang-format on
inline constexpr int kV3Count = sizeof(kV3Entries) / sizeof(kV3Entries[0]);

// the translation unit that instantiates the entry (launch3_unit<U>): 0 osg_conv3x3.hip, 1 osg_conv3x3_w8.hip
constexpr int v3_unit(const V3Entry& e) { return e.wq; }
constexpr int v3_find(int w, int bn, int nlw, int wq) {
    for (int i = 0; i < kV3Count; i++)
        if (kV3Entries[i].w == w && kV3Entries[i].bn == bn && kV3Entries[i].nlw == nlw && kV3Entries[i].wq == wq) return i;
    return -1;
}
// the entry a halo-kernel request runs (-1: an image width it does not take): bn outside {80, 160} -> 128; uint8 codes with 160 columns at W = 64 -> 80; 8 loader
// waves where an f16 entry has them, else 4.  Every entry folds a split that asks for it.
constexpr int resolve3(int w, int bn, int loader_waves, bool w8) {
    if (bn != 80 && bn != 160) bn = 128;
    if (w8 && w == 64 && bn == 160) bn = 80;
    const int e = loader_waves == 8 && !w8 ? v3_find(w, bn, 8, 0) : -1;
    return e >= 0 ? e : v3_find(w, bn, 4, w8);
}

// a tune-table row's cfg: tile | KS = 2 << 3 | fold << 4 | spec << 5 (a halo-kernel row: fold << 4 only)
constexpr int tune_cfg(const V2Choice& c) { return c.cfg | (c.ks == 2 ? 8 : 0) | (c.fold ? 16 : 0) | (c.spec ? 32 : 0); }
constexpr V2Choice tune_choice(int cfg, int nst, int splits) { return V2Choice{cfg & 7, nst, splits, (cfg & 8) ? 2 : 1, (cfg >> 4) & 1, (cfg >> 5) & 1}; }
// does a row name a launchable configuration (osg_ctx.hip drops it otherwise)?  family 0 (gemm2_kernel): an entry of the plain GEMM as it stands, spec with one
// k-slice, fold on a fold-capable entry with 2-4 slices.  family 1 (halo kernel): a tile width of its entries, nst = loader waves (0: 4).
constexpr bool tune_row_ok(int family, int cfg, int nst, int splits, int bn) {
    if (splits < 1 || splits > 64) return false;
    if (family == 1) return (cfg == 0 || (cfg == 16 && splits <= 4 && splits >= 2)) && (nst == 0 || nst == 4 || nst == 8) && v3_find(8, bn, 4, 0) >= 0;
    if (family != 0 || (cfg & ~63)) return false;
    const V2Choice ch = tune_choice(cfg, nst, splits);
    const int e = v2_find(V2Form{}, ch.cfg, nst, ch.spec, ch.ks);
    return e >= 0 && (!ch.spec || splits == 1) && (!ch.fold || (v2_fold_capable(kV2Entries[e]) && splits <= 4 && splits >= 2));
}

}  // namespace osg_mm
