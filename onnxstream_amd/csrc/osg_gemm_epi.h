// libosgpu: the epilogue variant of a gemm2_kernel launch.  The fused epilogue decides bias type, per-image bias, residual, activation, second destination, row
// statistics, split-K slab and every store's bounds with uniform run-time branches; a launch walks that code once, cold.  The plan knows the form of
// every launch when it is built, so the forms the headline plan runs have instantiations whose EPI template argument names exactly what the epilogue contains:
// everything else is compiled out, and with it the element-wise fallback and the bounds of every load and store -- a lean variant runs only whole tiles with
// 8-byte aligned rows.  EPI_ANY is the kernel with every decision at run time, the code of every entry of kV2Entries.
// Host-only C++17 (no HIP, no getenv): the launcher (osg_gemm.hip launch_v2_choice) describes its launch in an EpiLaunch and passes the OSG_EPI_GENERIC switch in;
// tests/cpp/epilogue_select.cpp compiles this with g++.
#pragma once
#include "osg_gemm_routes.h"
#include <cstdint>

namespace osg_mm {

// what a launch's epilogue contains.  A lean mask is made of kEpiLeanBits only; the other bits describe launches that stay with EPI_ANY.
enum : int {
    EPI_BIAS16 = 1,        // f16 bias [N]
    EPI_BIAS32 = 2,        // f32 bias [N] (the c2 of a folded LayerNorm included)
    EPI_ROWBIAS = 4,       // per-image bias
    EPI_RESIDUAL = 8,
    EPI_SILU = 16,
    EPI_C2 = 32,           // second destination
    EPI_ROWSTATS = 64,     // row statistics of the rounded outputs (rs_out)
    EPI_SPLIT = 128,       // a k-slice of a split launch that the reduce launch finishes: f32 slab stores, nothing else
    EPI_FOLD = 256,        // a split finished in the kernel (splitk_fold_acc)
    EPI_GEGLU = 512,       // the pair-interleaved GEGLU epilogue: bias and nothing else beside it
    EPI_SINKS = 1024,      // GroupNorm statistics sinks
    EPI_OTHER = 2048,      // anything else a lean variant does not hold: another activation, a batch, the A/B switch that turns the operand prefetch off
};
constexpr int EPI_ANY = -1;
constexpr int kEpiLeanBits = EPI_BIAS16 | EPI_BIAS32 | EPI_ROWBIAS | EPI_RESIDUAL | EPI_SILU | EPI_C2 | EPI_ROWSTATS | EPI_SPLIT | EPI_GEGLU;

// what the selection reads of a launch (GemmParams and the batch count, osg_gemm_common.h epi_launch_of)
struct EpiLaunch {
    int M = 0, N = 0, batch = 1, splits = 1;
    bool fold = false;
    bool bias = false, bias_f32 = false, rowbias = false, residual = false, c2 = false, rowstats = false, sinks = false;
    int act = 0;                   // osg_act: 0 none, 1 SiLU, 3 GEGLU
    bool other = false;            // see EPI_OTHER
    long ldc = 0, ldc2 = 0, rb_ld = 0;   // element pitches (0: dense)
    int rs_np = 0;                 // row-statistics slots per row
    uintptr_t align_or = 0;        // C | C2 | residual | per-image bias | bias | row statistics, as addresses: their common alignment
};

// the form of the launch as a mask.  A k-slice that the reduce launch finishes stores its slab and reads no epilogue operand: its form is EPI_SPLIT alone.
constexpr int epi_form(const EpiLaunch& l) {
    if (l.other || l.batch != 1) return EPI_OTHER;
    if (l.splits > 1 && !l.fold) return EPI_SPLIT;
    int m = 0;
    if (l.splits > 1) m |= EPI_FOLD;
    if (l.bias) m |= l.bias_f32 ? EPI_BIAS32 : EPI_BIAS16;
    if (l.rowbias) m |= EPI_ROWBIAS;
    if (l.residual) m |= EPI_RESIDUAL;
    if (l.act == 1) m |= EPI_SILU;
    else if (l.act == 3) m |= EPI_GEGLU;
    else if (l.act != 0) m |= EPI_OTHER;
    if (l.c2) m |= EPI_C2;
    if (l.rowstats) m |= EPI_ROWSTATS;
    if (l.sinks) m |= EPI_SINKS;
    return m;
}
// the guarantee every lean variant carries: whole tiles, rows and operands 8-byte aligned (4 halves), every row-statistics slot inside the matrix
constexpr bool epi_whole(const EpiLaunch& l, int bm, int bn) {
    return l.M > 0 && l.N > 0 && l.M % bm == 0 && l.N % bn == 0 && (l.ldc & 3) == 0 && (l.ldc2 & 3) == 0 && (!l.rowbias || (l.rb_ld & 3) == 0) && (l.align_or & 7) == 0 &&
           (!l.rowstats || l.rs_np * 32 == l.N);
}

// one lean instantiation: an entry of kV2Entries (by its template arguments) and the mask it is compiled for
struct LeanEntry { V2Entry e; int mask; };
constexpr bool v2_same(const V2Entry& a, const V2Entry& b) {
    return a.bm == b.bm && a.bn == b.bn && a.nst == b.nst && a.conv == b.conv && a.spec == b.spec && a.ln == b.ln && a.nch == b.nch && a.ks == b.ks && a.wgn == b.wgn && a.wq == b.wq;
}
constexpr int v2_index(const V2Entry& e) {
    for (int i = 0; i < kV2Count; i++)
        if (v2_same(kV2Entries[i], e)) return i;
    return -1;
}
// can the kernel be compiled lean for (entry, mask)?  A mask of lean bits, one bias type at most; a folded-LayerNorm entry always has its f32 c2; row
// statistics and GEGLU's value / gate pairs need 32-column wave slots; a split slab stands alone and comes from a kernel that splits (no LayerNorm); GEGLU goes
// with a bias only.
constexpr bool lean_holds(const V2Entry& e, int mask) {
    if (mask == EPI_ANY || (mask & ~kEpiLeanBits)) return false;
    if ((mask & EPI_BIAS16) && (mask & EPI_BIAS32)) return false;
    if ((mask & EPI_SPLIT) && (mask != EPI_SPLIT || e.ln != 0)) return false;
    if (e.ln != 0 && !(mask & EPI_BIAS32)) return false;
    if ((mask & (EPI_ROWSTATS | EPI_GEGLU)) && (e.bn / e.wgn) % 32 != 0) return false;
    if ((mask & EPI_GEGLU) && (mask & ~(EPI_GEGLU | EPI_BIAS16 | EPI_BIAS32))) return false;
    return true;
}

// clang-format off
// The (entry, form) pairs the shipped SD 1.5 plan runs on whole tiles: 110 of the 120 gemm2_kernel launches of a pass (profiles/epilogue_forms_table.txt lists them by
// launches x instructions removed).  An entry by its template arguments: BM, BN, NST, CONV, SPEC, LN, NCH, KS, WGN, WQ.
inline constexpr LeanEntry kLeanEntries[] = {
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_RESIDUAL | EPI_ROWSTATS},     // to_out / ff.net.2 + residual, row statistics for the next LayerNorm
    {{64, 80, 4, 0, 0, 0, 5, 1, 1, 0}, EPI_BIAS16 | EPI_RESIDUAL},
    {{64, 64, 4, 0, 0, 2, 20, 1, 2, 0}, EPI_BIAS32},                                  // LayerNorm + merged q / k / v, to_q at 1280 channels
    {{64, 64, 4, 0, 0, 0, 5, 2, 2, 0}, EPI_BIAS16 | EPI_ROWSTATS},                    // proj_in
    {{64, 64, 2, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_ROWSTATS},
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_ROWSTATS},
    {{128, 128, 4, 0, 1, 2, 10, 1, 2, 0}, EPI_BIAS32},
    {{64, 64, 4, 0, 0, 2, 10, 1, 2, 0}, EPI_BIAS32},
    {{128, 64, 4, 0, 0, 2, 20, 1, 2, 0}, EPI_BIAS32},
    {{128, 64, 2, 0, 0, 2, 10, 1, 2, 0}, EPI_BIAS32 | EPI_GEGLU},                     // LayerNorm + GEGLU projection
    {{128, 160, 4, 0, 0, 2, 20, 1, 1, 0}, EPI_BIAS32 | EPI_GEGLU},
    {{128, 80, 4, 0, 0, 0, 5, 1, 1, 0}, EPI_SPLIT},
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_SPLIT},
    {{64, 80, 4, 0, 0, 0, 5, 1, 1, 0}, EPI_BIAS16},                                   // 1 x 1 shortcut convolutions
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16},
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_RESIDUAL},
    {{128, 80, 4, 0, 0, 0, 5, 1, 1, 0}, EPI_BIAS16},
    {{64, 80, 4, 0, 0, 0, 5, 1, 1, 0}, EPI_BIAS16 | EPI_RESIDUAL | EPI_C2},           // proj_out + residual, stored into its Concat slot too
    {{64, 64, 4, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_RESIDUAL | EPI_C2},
    {{64, 64, 6, 0, 0, 0, 5, 1, 2, 0}, EPI_BIAS16 | EPI_RESIDUAL | EPI_ROWSTATS},
    {{128, 64, 4, 0, 0, 2, 20, 1, 2, 0}, EPI_BIAS32 | EPI_GEGLU},
    {{64, 64, 4, 1, 0, 0, 5, 2, 2, 0}, EPI_BIAS16 | EPI_C2},                          // the stride-2 downsampling convolutions
    {{64, 64, 4, 1, 0, 0, 5, 2, 2, 0}, EPI_SPLIT},
    {{64, 128, 4, 1, 0, 0, 5, 1, 2, 0}, EPI_SPLIT},
};
// clang-format on
inline constexpr int kLeanCount = sizeof(kLeanEntries) / sizeof(kLeanEntries[0]);

constexpr bool lean_list_ok() {
    for (int i = 0; i < kLeanCount; i++) {
        if (v2_index(kLeanEntries[i].e) < 0 || !lean_holds(kLeanEntries[i].e, kLeanEntries[i].mask)) return false;
        for (int j = 0; j < i; j++)
            if (v2_same(kLeanEntries[i].e, kLeanEntries[j].e) && kLeanEntries[i].mask == kLeanEntries[j].mask) return false;
    }
    return true;
}
static_assert(lean_list_ok(), "kLeanEntries: every pair names an entry of kV2Entries and a mask the kernel compiles lean, once");

// the epilogue variant a launch of `entry` runs: the index in kLeanEntries of the instantiation compiled for exactly this form, when the launch meets the whole-tile
// guarantee; -1 = EPI_ANY (also with OSG_EPI_GENERIC=1: force_generic)
constexpr int select_epi(int entry, const EpiLaunch& l, bool force_generic) {
    if (force_generic || entry < 0 || entry >= kV2Count) return -1;
    const V2Entry& e = kV2Entries[entry];
    const int form = epi_form(l);
    if (!lean_holds(e, form) || !epi_whole(l, e.bm, e.bn)) return -1;
    for (int i = 0; i < kLeanCount; i++)
        if (kLeanEntries[i].mask == form && v2_same(kLeanEntries[i].e, e)) return i;
    return -1;
}

}  // namespace osg_mm
