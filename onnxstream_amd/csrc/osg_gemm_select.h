// libosgpu: what a contraction launch REQUESTS -- tile, ring, k-slices, fold, loader waves -- before osg_gemm_routes.h resolves the request to an instantiation.
// The cost models (rank_v2, rank_halo3), the deterministic default plan (model_choice, choose_v1: autotune off, what every parity test runs), the candidate
// lists a measured choice times (and whose first entry a frozen tune table falls back to), the split rule, the halo kernel's shape gate, the tune-table key and
// the conversions between a table row and a typed choice.  Host-only C++17: no HIP, no osg_ctx, no getenv -- the launchers (osg_gemm.hip, osg_conv3x3.hip) read
// the context and the environment into a SelectEnv and pass plain values in; tests/cpp/contraction_select.cpp compiles this with g++.
#pragma once
#include "osg_gemm_routes.h"
#include <algorithm>
#include <cmath>
#include <tuple>
#include <utility>
#include <vector>

// the measured-choice table's key and row (osg_tune.h: lookup / store / time_us)
namespace osg_tune {

struct Key {
    int kind;       // 0: GEMM, 1: 3x3/s1/p1 convolution (halo-reuse kernel and implicit GEMM compete), 2: other implicit-GEMM convolution
    int device;
    int M, N, K, batch;
    int H, W, Cin, KW, sh, sw;   // kind 0: H = lda, the rest 0
    // the form of the launch: act (bits 0-3) | residual << 4 | per-image bias << 5 | f32 bias << 6 | folded LayerNorm << 7 | handed-over row statistics << 8 |
    // row statistics produced << 9 | uint8 weight codes << 10
    int flags;
    bool operator<(const Key& o) const {
        return std::tie(kind, device, M, N, K, batch, H, W, Cin, KW, sh, sw, flags) <
               std::tie(o.kind, o.device, o.M, o.N, o.K, o.batch, o.H, o.W, o.Cin, o.KW, o.sh, o.sw, o.flags);
    }
};

struct Choice {
    int family;     // 0: gemm2 (cfg, nst, splits); 1: conv3x3 (bn, splits; nst = loader waves, cfg = fold << 4)
    int cfg, nst, splits, bn;
    float us;       // measured time of the winner
};

}  // namespace osg_tune

namespace osg_mm {

// everything the choice reads of the context and the environment
struct SelectEnv {
    int num_cu = 256;
    bool measured = false;   // the context's autotune flag: the wider candidate set of a measured choice
    int fold_mode = 1;       // OSG_SPLITK_FOLD: 0 = no folded candidates
    bool no_wide = false, no_spec = false, no_ks2 = false;   // OSG_TUNE_NO_WIDE / _NO_SPEC / _NO_KS2 (A/B runs)
};

// the shape of a launch, as GemmParams carries it (a GEMM: M, N, K, batch, lda; a convolution: M = images * Ho * Wo, N = Cout, K = KH * KW * Cin and the geometry)
struct SelectShape {
    int M = 0, N = 0, K = 0, batch = 1;
    long lda = 0;
    int H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, KW = 0, sh = 0, sw = 0, pt = 0, pl = 0;
    bool w8 = false;
};

// "ask for `asked` slices of `units` k-units, run no empty slice": {slices that run, units per slice}
constexpr std::pair<int, int> split_slices(int units, int asked) {
    const int per = (units + std::max(asked, 1) - 1) / std::max(asked, 1);
    return {(units + per - 1) / per, per};
}

// v2 tile / ring / split-K choice.  Measured on MI355X (tools/gemm_probe.py): the L2->LDS DMA path sustains ~23 B/clk per CU
// and bounds every configuration (a 128x128x64 k-tile moves 32 KiB for 515 MFMA cycles), so the model is: k-tile time =
// max(MFMA, bytes / 23) (+ ~450 exposed cycles when a block is alone on its CU), whole rounds of tiles over the CU slots,
// a fixed fill + epilogue per round, and the extra pass of a split-K reduce.
// every legal (tile, stages, splits) with its modelled cost in cycles, cheapest first
inline std::vector<std::pair<double, V2Choice>> rank_v2(const SelectEnv& env, int M, int N, int K, int batch, bool allow_split, V2Form form = V2Form{}) {
    const double cus = env.num_cu;
    const int kt = K / 64;
    std::vector<std::pair<double, V2Choice>> out;
    for (int c = 0; c < (env.measured ? (env.no_wide ? 4 : 8) : 3); c++)
        for (int nst = 8; nst >= 2; nst -= 2) {
            if (!v2_holds(form, c, nst)) continue;                            // (an instantiation for the form: osg_gemm_routes.h)
            // 6 / 8 stages (every tile of a short-K GEMM in flight at once): only as a measured candidate, only where the ring fits the LDS
            if ((nst == 6 || nst == 8) && !env.measured) continue;
            if (c >= 4 && N % 80 != 0) continue;              // (the 80 / 160-column tiles are for the widths they divide)
            const int bnp = (kV2BN[c] + 31) / 32 * 32;
            const double tiles = (double)((M + kV2BM[c] - 1) / kV2BM[c]) * ((N + kV2BN[c] - 1) / kV2BN[c]) * batch;
            const double mfma = kV2BM[c] * kV2BN[c] * 128.0 / 4069.0;
            const double tload = (kV2BM[c] * 128.0 + kV2BN[c] * (form.w8 ? 64.0 : 128.0)) / 23.0;
            const int smem = form.w8 ? nst * (kV2BM[c] * 128 + (kV2BN[c] + 63) / 64 * 64 * 64) : nst * (kV2BM[c] + bnp) * 128;
            if (smem > 160 * 1024) continue;
            const int bpc = std::min(4, 163840 / smem);
            for (int s = 1; s <= (allow_split ? 16 : 1); s++) {
                if (s > 1 && (kt / s < (env.measured ? 3 : 8))) break;   // measured choice: let shorter slices compete too
                const int kts = (kt + s - 1) / s;
                if (s > 1 && (kts * (s - 1) >= kt)) continue;   // an empty split
                const double blocks = tiles * s;
                const double rounds = std::ceil(blocks / (cus * bpc));
                const double conc = std::min((double)bpc, std::ceil(blocks / cus));
                const double tk = conc <= 1.0 ? std::max(mfma, tload) + 450.0 : conc * std::max(mfma, tload);
                double cost = rounds * (kts * tk + 3500.0);
                if (s > 1) cost += 9000.0 + (double)M * N * batch * s * 4.0 / 2000.0;   // reduce launch (measured ~4-7 us) + slab traffic
                out.push_back({cost, V2Choice{c, nst, s}});
                // (measured candidates only, round 6) the one-workgroup-per-CU tiles with their DMA requests issued by four LOADER waves: a wave that issues both
                // stalls ~70-100 cycles per request (the CU's address path takes 1 KiB per ~17 cycles and the four waves queue on it) with its MFMAs behind them
                if (env.measured && !env.no_spec && !env.no_wide && !form.w8 && (c == 0 || c == 4) && nst == 4 && s == 1 && !form.conv && !form.ln1) out.push_back({cost * 0.9995, V2Choice{c, nst, s, 1, 0, 1}});
                // KS = 2 (measured candidates only): the 64x64 tile with a 2- or 4-stage ring, the 128x64 tile with 2 stages (what the 160 KiB hold), >= 2 k-tiles per slice
                if (env.measured && !env.no_ks2 && !form.w8 && kts >= 2 && ((c == 2 && (nst == 2 || nst == 4)) || (c == 1 && nst == 2))) out.push_back({cost * 0.999, V2Choice{c, nst, s, 2}});
                // (measured candidates only) 2 .. 4 slices folded by the last arriver of each tile instead of a reduce launch: the tiles of at most 10 accumulator quads per lane
                if (env.measured && s >= 2 && s <= 4 && c != 0 && c != 4 && c != 7 && env.fold_mode != 0) out.push_back({cost * 1.0005, V2Choice{c, nst, s, 1, 1}});
            }
        }
    std::stable_sort(out.begin(), out.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    return out;
}

// GEGLU pairing / folded LayerNorm / row statistics live in the tile epilogue: such a launch runs one k-slice
constexpr bool v2_allows_split(const V2Form& f) { return !f.geglu && !f.ln1 && !f.ln2 && !f.rowstats; }

// The deterministic default: what a gemm2_kernel launch requests with autotune off and no override.  Two rules, kept apart on purpose -- every default plan and
// the parity tests' routes depend on each as it stands:
//   f16:    rank the PLAIN GEMM form with splits allowed, take the cheapest, THEN clamp to one k-slice for a form that cannot split.  (A GEGLU / LayerNorm /
//           row-statistics launch therefore runs the tile and ring that won WITH a split, on one slice -- not the cheapest unsplit candidate.)
//   uint8:  rank the form's conv / GEGLU / w8 bits (no LayerNorm, no row statistics: no uint8 kernel takes them) with the form's real split permission.
inline V2Choice model_choice(const SelectEnv& env, int M, int N, int K, int batch, const V2Form& form) {
    const bool allow_split = v2_allows_split(form);
    std::vector<std::pair<double, V2Choice>> r;
    if (form.w8) {
        V2Form f;
        f.conv = form.conv; f.geglu = form.geglu; f.w8 = true;
        r = rank_v2(env, M, N, K, batch, allow_split, f);
    } else
        r = rank_v2(env, M, N, K, batch, true);
    V2Choice ch = r.empty() ? V2Choice{0, 4, 1} : r[0].second;
    if (!allow_split) ch.splits = 1;
    return ch;
}

// does gemm2_kernel (the direct-to-LDS path) take the shape?  Otherwise the register-staged gemm_kernel runs it, by choose_v1.
constexpr bool v2_takes(const SelectShape& s, bool conv) { return s.K % 64 == 0 && (conv ? s.Cin % 64 == 0 : s.lda % 8 == 0); }

// the register-staged gemm_kernel's tile (0: 128x128x32, 1: 128x64x32, 2: 64x64x32) and the k-slices it asks for (of 32-deep k-tiles, through split_slices)
struct V1Choice { int cfg, splits; };
inline V1Choice choose_v1(int num_cu, int M, int N, int K, int batch) {
    auto tiles = [&](int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn) * batch; };
    const long cu = num_cu;
    int cfg;
    if (tiles(128, 128) >= cu && N % 128 == 0) cfg = 0;
    else if (tiles(128, 64) >= cu && M >= 128) cfg = 1;
    else cfg = 2;
    const int bm = cfg == 2 ? 64 : 128, bn = cfg == 0 ? 128 : 64;
    long t = tiles(bm, bn);
    int splits = 1;
    if (t < cu && K >= 1024) {
        splits = (int)((2 * cu + t - 1) / t);
        int max_splits = K / 256;
        if (splits > max_splits) splits = max_splits;
        if (splits > 32) splits = 32;
        if (splits < 1) splits = 1;
    }
    return {cfg, splits};
}

// the halo-reuse 3x3 kernel's request: output channels per tile, k-slices (of 64-channel slabs), loader waves, fold
struct Halo3Choice { int bn, splits, loaders = 4, fold = 0; };

// the geometric part of the halo kernel's shape gate (osg_conv3x3_prepare adds the switch and the operands' alignment): 3x3 / stride 1 / pad 1 at W in
// {8, 16, 32, 64}, whole 128-pixel tiles (TH rows of an image; at W = 8 two 8 x 8 images), 64-channel slabs, N % 4 == 0, operands under 2 GiB
constexpr bool halo3_takes(const SelectShape& s) {
    const int W = s.W, H = s.H;
    if (!(W == 64 || W == 32 || W == 16 || W == 8)) return false;
    if (s.Wo != W || s.Ho != H || s.sh != 1 || s.sw != 1 || s.pt != 1 || s.pl != 1 || s.KW != 3 || s.K != 9 * s.Cin) return false;
    if (s.Cin % 64 || s.N % 4) return false;
    const int TI = W == 8 ? 2 : 1, TH = 128 / (W * TI);
    if (H % TH) return false;
    if (W == 8 && H != 8) return false;
    if ((double)s.M * s.Cin * 2.0 >= 2147483648.0 || (double)s.N * s.K * 2.0 >= 2147483648.0) return false;   // (M = images * H * W here: the input's bytes)
    return true;
}

// Tile/split choice of the halo kernel.  Model (cycles, calibrated like rank_v2): a (slab, tap) unit costs
// max(MFMA, bytes / 23 B/clk) with bytes = the weight tile + 1/9 of the patch; whole rounds of tiles over the CUs.
// every legal (BN, splits) with its modelled cost in cycles, cheapest first (4 loader waves each: the measured choice tries 8 as well, conv3_candidates)
inline std::vector<std::pair<double, Halo3Choice>> rank_halo3(const SelectEnv& env, const SelectShape& p) {
    const int W = p.W;
    const int TI = W == 8 ? 2 : 1, TH = 128 / (W * TI);
    const double cus = env.num_cu;
    const int slabs = p.Cin / 64;
    const int mt = (p.M + 127) / 128;
    const int pp = TI * (TH + 2) * (W == 8 ? 16 : W + 2);
    std::vector<std::pair<double, Halo3Choice>> out;
    constexpr int bns[3] = {80, 128, 160};
    for (int bn : bns) {
        if (bn != 128 && p.N % bn) continue;
        const double tiles = (double)mt * ((p.N + bn - 1) / bn);
        const double mfma = 128.0 * bn * 128.0 / 4069.0;
        const double tload = (bn * (p.w8 ? 64.0 : 128.0) + pp * 128.0 / 9.0) / 23.0;
        for (int s = 1; s <= (env.measured ? 12 : 8); s++) {
            if (s > 1 && slabs / s < (env.measured ? 1 : 2)) break;   // measured choice: let finer splits compete too
            const int sl = (slabs + s - 1) / s;
            if (s > 1 && sl * (s - 1) >= slabs) continue;
            const double blocks = tiles * s;
            const double rounds = std::ceil(blocks / cus);
            double cost = rounds * (sl * 9.0 * (std::max(mfma, tload) + 250.0) + 6000.0);
            if (s > 1) cost += 9000.0 + (double)p.M * p.N * s * 4.0 / 2000.0;
            out.push_back({cost, Halo3Choice{bn, s}});
            // (measured candidates only) the same split finished inside the kernel by the last arriver of each tile (dearer than its twin: never ranked first)
            if (env.measured && s >= 2 && s <= 4 && env.fold_mode != 0) out.push_back({cost * 1.0005, Halo3Choice{bn, s, 4, 1}});
        }
    }
    std::stable_sort(out.begin(), out.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    return out;
}
// the halo kernel's default: the cheapest candidate
inline Halo3Choice model_halo3(const SelectEnv& env, const SelectShape& p) {
    const auto r = rank_halo3(env, p);
    return r.empty() ? Halo3Choice{128, 1} : r[0].second;
}

// ---- table rows <-> typed choices: the one place that knows a halo row keeps its loader waves in nst (0: 4) and its fold in cfg & 16
inline osg_tune::Choice tune_row(const V2Choice& c, float us = -1.f) { return {0, tune_cfg(c), c.nst, c.splits, 0, us}; }
inline osg_tune::Choice tune_row(const Halo3Choice& c, float us = -1.f) { return {1, c.fold ? 16 : 0, c.loaders, c.splits, c.bn, us}; }
inline V2Choice row_v2(const osg_tune::Choice& r) { return tune_choice(r.cfg, r.nst, r.splits); }
inline Halo3Choice row_halo3(const osg_tune::Choice& r) { return {r.bn, r.splits, r.nst == 8 ? 8 : 4, (r.cfg >> 4) & 1}; }

// ---- what a measured choice times, in this order (the first one is what a frozen table's miss, a launch under capture or one that consumes its own output runs)
struct Candidate { osg_tune::Choice row; double model; };   // model: the modelled cost in cycles
inline std::vector<Candidate> gemm_candidates(const SelectEnv& env, int M, int N, int K, int batch, const V2Form& form) {
    std::vector<Candidate> out;
    for (const auto& c : rank_v2(env, M, N, K, batch, v2_allows_split(form), form)) out.push_back({tune_row(c.second), c.first});
    return out;
}
// the 3x3 / stride 1 / pad 1 convolution: the halo kernel's (BN, splits) x loader waves {4, 8} (no_nl8, uint8 codes: 4 only), then the implicit-GEMM kernel's
// first 6 (tile, stages, splits)
inline std::vector<Candidate> conv3_candidates(const SelectEnv& env, const SelectShape& p, bool no_nl8) {
    std::vector<Candidate> out;
    for (const auto& c : rank_halo3(env, p))
        for (int nl : {4, 8}) {
            if (nl == 8 && (no_nl8 || p.w8)) continue;
            Halo3Choice h = c.second;
            h.loaders = nl;
            out.push_back({tune_row(h), c.first});
        }
    V2Form form;
    form.conv = true; form.w8 = p.w8;
    auto r2 = rank_v2(env, p.M, p.N, p.K, 1, true, form);
    if (r2.size() > 6) r2.resize(6);
    for (const auto& c : r2) out.push_back({tune_row(c.second), c.first});
    return out;
}

// ---- the table's key
struct KeyForm { int act = 0; bool residual = false, rowbias = false, bias_f32 = false, ln = false, rs_in = false, rs_out = false, w8 = false; };
inline osg_tune::Key tune_key(int kind, const SelectShape& s, const KeyForm& f) {
    osg_tune::Key k{};
    k.kind = kind; k.device = 0;   /* (one table for every MI355X of a node: ranks seeded from one file make identical choices) */ k.M = s.M; k.N = s.N; k.K = s.K; k.batch = s.batch;
    if (kind != 0) { k.H = s.H; k.W = s.W; k.Cin = s.Cin; k.KW = s.KW; k.sh = s.sh; k.sw = s.sw; }
    else k.H = (int)s.lda;
    k.flags = f.act | (f.residual ? 16 : 0) | (f.rowbias ? 32 : 0) | (f.bias_f32 ? 64 : 0) | (f.ln ? 128 : 0) | (f.rs_in ? 256 : 0) | (f.rs_out ? 512 : 0) | (f.w8 ? 1024 : 0);
    return k;
}

}  // namespace osg_mm
