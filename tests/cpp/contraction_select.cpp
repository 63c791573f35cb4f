// tests/test_contraction_select_cpu.py, tests/test_contraction_select_gpu.py: the launch choice of onnxstream_amd/csrc/osg_gemm_select.h, printed for the Python side.
//   plan NUM_CU FILE   FILE: one tune-table key per line (kind device M N K batch H W Cin KW sh sw flags).  Per key: the key; `model`: the deterministic default
//                      (autotune off) as a table row (family cfg nst splits bn), `route`: what osg_last_route reports for it (family, instantiation, k-slices);
//                      then one `c` line per candidate of the measured choice (autotune on, fold mode 1, no A/B switch), in the order they are timed
//   slices             split_slices of units 1-80 x asked 1-64
//   keys FILE          FILE: one call per line (kind M N K batch lda H W Cin KW sh sw act residual rowbias bias_f32 ln rs_in rs_out w8): its tune_key
//   halo               halo3_takes of a 3x3 / pad 1 convolution, Cin 64, over H, W in {4, 8, 12, 16, 24, 32, 64, 128} x stride {1, 2} x Cout {6, 8}
#include "osg_gemm_select.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

using namespace osg_mm;

static void print_row(const char* tag, const osg_tune::Choice& r) { printf("%s %d %d %d %d %d", tag, r.family, r.cfg, r.nst, r.splits, r.bn); }

// a 3x3 / stride 1 / pad 1 (kind 1) or k x k / pad k / 2 (kind 2) convolution's shape from its key
static SelectShape shape_of(const osg_tune::Key& k) {
    SelectShape s;
    s.M = k.M; s.N = k.N; s.K = k.K; s.batch = k.batch; s.w8 = (k.flags & 1024) != 0;
    if (k.kind == 0) { s.lda = k.H; return s; }
    const int kw = k.kind == 1 ? 3 : k.KW, st = k.kind == 1 ? 1 : k.sh;
    s.H = k.H; s.W = k.W; s.Cin = k.Cin; s.KW = kw; s.sh = s.sw = st; s.pt = s.pl = kw / 2;
    s.Ho = (k.H + 2 * (kw / 2) - kw) / st + 1; s.Wo = (k.W + 2 * (kw / 2) - kw) / st + 1;
    return s;
}

static V2Form form_of(const osg_tune::Key& k) {
    V2Form f;
    f.conv = k.kind != 0; f.ln1 = (k.flags & 128) && !(k.flags & 256); f.ln2 = (k.flags & 128) && (k.flags & 256); f.geglu = (k.flags & 15) == 3;
    f.rowstats = (k.flags & 512) != 0; f.w8 = (k.flags & 1024) != 0;
    f.nch = v2_nch(f.ln2 ? k.K / 32 : 0);
    return f;
}

static int plan(int num_cu, const char* path) {
    FILE* in = fopen(path, "r");
    if (!in) return 1;
    SelectEnv off, on;
    off.num_cu = on.num_cu = num_cu;
    on.measured = true;
    osg_tune::Key k{};
    while (fscanf(in, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &k.kind, &k.device, &k.M, &k.N, &k.K, &k.batch, &k.H, &k.W, &k.Cin, &k.KW, &k.sh, &k.sw, &k.flags) == 13) {
        printf("key %d %d %d %d %d %d %d %d %d %d %d %d %d\n", k.kind, k.device, k.M, k.N, k.K, k.batch, k.H, k.W, k.Cin, k.KW, k.sh, k.sw, k.flags);
        const SelectShape s = shape_of(k);
        const V2Form f = form_of(k);
        std::vector<Candidate> cands;
        if (k.kind == 1 && halo3_takes(s)) {
            const Halo3Choice h = model_halo3(off, s);
            print_row("model", tune_row(h));
            printf("\nroute 1 %d %d\n", resolve3(s.W, h.bn, h.loaders, s.w8), split_slices(s.Cin / 64, h.splits).first);
            cands = conv3_candidates(on, s, false);
        } else if (v2_takes(s, f.conv)) {
            const V2Choice ch = model_choice(off, s.M, s.N, s.K, s.batch, f);
            print_row("model", tune_row(ch));
            printf("\nroute 0 %d %d\n", resolve_v2(ch, f).entry, split_slices(s.K / 64, ch.splits).first);
            cands = gemm_candidates(on, s.M, s.N, s.K, s.batch, f);
        } else {   // the register-staged kernel: tile | vector loads << 2 | convolution << 3
            const V1Choice v = choose_v1(num_cu, s.M, s.N, s.K, s.batch);
            const bool vec = f.conv ? s.Cin % 8 == 0 : (s.K % 8 == 0 && s.lda % 8 == 0);
            printf("model 2 %d 0 %d 0\nroute 2 %d %d\n", v.cfg, v.splits, v.cfg | (vec ? 4 : 0) | (f.conv ? 8 : 0), split_slices((s.K + 31) / 32, v.splits).first);
        }
        for (const Candidate& c : cands) {
            print_row("c", c.row);
            printf(" %.1f\n", c.model);
        }
    }
    fclose(in);
    return 0;
}

static int keys(const char* path) {
    FILE* in = fopen(path, "r");
    if (!in) return 1;
    int kind, v[19];
    for (;;) {
        if (fscanf(in, "%d", &kind) != 1) break;
        for (int& x : v)
            if (fscanf(in, "%d", &x) != 1) { fclose(in); return 1; }
        SelectShape s;
        s.M = v[0]; s.N = v[1]; s.K = v[2]; s.batch = v[3]; s.lda = v[4]; s.H = v[5]; s.W = v[6]; s.Cin = v[7]; s.KW = v[8]; s.sh = v[9]; s.sw = v[10];
        KeyForm f;
        f.act = v[11]; f.residual = v[12]; f.rowbias = v[13]; f.bias_f32 = v[14]; f.ln = v[15]; f.rs_in = v[16]; f.rs_out = v[17]; f.w8 = v[18];
        const osg_tune::Key k = tune_key(kind, s, f);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", k.kind, k.device, k.M, k.N, k.K, k.batch, k.H, k.W, k.Cin, k.KW, k.sh, k.sw, k.flags);
    }
    fclose(in);
    return 0;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "plan") && argc == 4) return plan(atoi(argv[2]), argv[3]);
    if (!strcmp(mode, "keys") && argc == 3) return keys(argv[2]);
    if (!strcmp(mode, "slices")) {
        for (int units = 1; units <= 80; units++)
            for (int asked = 1; asked <= 64; asked++) printf("%d %d %d %d\n", units, asked, split_slices(units, asked).first, split_slices(units, asked).second);
        return 0;
    }
    if (!strcmp(mode, "halo")) {
        for (int h : {4, 8, 12, 16, 24, 32, 64, 128})
            for (int w : {4, 8, 12, 16, 24, 32, 64, 128})
                for (int st : {1, 2})
                    for (int n : {6, 8}) {
                        osg_tune::Key k{};
                        k.kind = 2; k.N = n; k.K = 9 * 64; k.batch = 1; k.H = h; k.W = w; k.Cin = 64; k.KW = 3; k.sh = k.sw = st;
                        SelectShape s = shape_of(k);
                        s.M = s.Ho * s.Wo;
                        printf("%d %d %d %d %d\n", h, w, st, n, (int)halo3_takes(s));
                    }
        return 0;
    }
    return 2;
}
