#!/usr/bin/env python3
"""profiles/epilogue_forms_ab.txt from the result files of one A/B/C series (the method of profiles/kernarg_preload_ab.txt):
A = the parent commit's libosgpu.so (OSGPU_LIB), B = this tree, C = this tree with OSG_EPI_GENERIC=1 (every launch runs its entry's EPI_ANY instantiation).

  DIR/r<round>_<A|B|C>.json   the JSON line of `bench.py --gpus 1 --steps 20 --warmup 5 --cpu-passes 0 --windows 5`, each run its own process, A, B, C alternating
  DIR/dump_compare.txt        (optional) the comparison of `--dump-outputs` between A and B
  TRACES/timeline_<A|B|C>.txt (optional) tools/graph_trace.py of one `rocprofv3 --kernel-trace -- python bench.py --steps 10 --warmup 5 --windows 0` run per library

    python tools/epilogue_forms_ab.py DIR [TRACES] [-o profiles/epilogue_forms_ab.txt]
"""
import argparse
import glob
import json
import os
import re
import statistics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGS = ("ms_per_step", "ms_per_step_window_median", "unet_device_ms_per_step")


def find(o, key):
    if isinstance(o, dict):
        if key in o:
            return o[key]
        o = list(o.values())
    if isinstance(o, list):
        for v in o:
            r = find(v, key)
            if r is not None:
                return r
    return None


def family(name):
    for f in ("gemm2_kernel", "conv3x3_kernel", "attn2_kernel", "gn_slab_kernel", "tblock_tail_kernel", "splitk_reduce", "conv_cin4", "kv_pack"):
        if f in name:
            return f
    return "other"


def timeline(path):
    """[(duration us, kernel name)] per position of the replayed pass, and the header lines"""
    rows, head = [], []
    for l in open(path):
        if l.startswith("#"):
            head.append(l.rstrip())
            continue
        f = l.rstrip("\n").split("\t")
        if len(f) >= 4:
            rows.append((float(f[1]), f[3]))
    return rows, head


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("traces", nargs="?")
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "epilogue_forms_ab.txt"))
    a = ap.parse_args()
    runs = {}
    for p in sorted(glob.glob(os.path.join(a.dir, "r*_[ABC].json"))):
        m = re.search(r"r(\d+)_([ABC])\.json$", p)
        j = json.loads(open(p).read().strip().splitlines()[-1])
        runs[(int(m.group(1)), m.group(2))] = [find(j, k) for k in FIGS]
    out = ["# Epilogue variants per launch form: A = parent library, B = this tree, C = this tree with OSG_EPI_GENERIC=1 (same library, every launch on its EPI_ANY instantiation)",
           "# Every run: bench.py --gpus 1 --steps 20 --warmup 5 --cpu-passes 0 --windows 5, its own process under its own time limit; A, B, C alternating, six rounds in one GPU call.",
           "# The figure is unet_device_ms_per_step (HIP events around the replayed graph); a gain needs every B below every A AND mean A - B >= 3 x the largest A-to-A difference.",
           "# round\tlibrary\t" + "\t".join(FIGS)]
    for (r, lib), v in sorted(runs.items()):
        out.append(f"{r}\t{lib}\t" + "\t".join("nan" if x is None else f"{x:.4f}" for x in v))
    verdicts = {}
    for k, fig in enumerate(FIGS):
        s = {lib: [v[k] for (r, l), v in sorted(runs.items()) if l == lib and v[k] is not None] for lib in "ABC"}
        if not all(s.values()):
            continue
        A, B, C = s["A"], s["B"], s["C"]
        spread = max(A) - min(A)
        gain = statistics.mean(A) - statistics.mean(B)
        below = max(B) < min(A)
        ratio = gain / spread if spread > 0 else float("inf")
        verdicts[fig] = (below, ratio, gain)
        out.append(f"# {fig}: " + "  ".join(f"{lib} {statistics.mean(x):.4f} ({min(x):.4f} .. {max(x):.4f})" for lib, x in (("A", A), ("B", B), ("C", C))))
        out.append(f"#   every B below every A: {'yes' if below else 'NO'};  mean A - B = {gain:+.4f} ms ({100 * gain / statistics.mean(A):+.2f} %), largest A-to-A difference {spread:.4f} ms, "
                   f"ratio {ratio:.1f} (a gain needs >= 3);  mean C - A = {statistics.mean(C) - statistics.mean(A):+.4f} ms, C within A's range: "
                   f"{'yes' if min(A) - spread <= statistics.mean(C) <= max(A) + spread else 'NO'}")
    if "unet_device_ms_per_step" in verdicts:
        below, ratio, gain = verdicts["unet_device_ms_per_step"]
        out.append(f"# VERDICT (unet_device_ms_per_step): {'a gain' if below and ratio >= 3 else 'NOT a gain by the criterion'}: every B below every A {'holds' if below else 'fails'}, "
                   f"mean A - B = {gain:+.4f} ms = {ratio:.1f} x the largest A-to-A difference")
    cmp_file = os.path.join(a.dir, "dump_compare.txt")
    if os.path.exists(cmp_file):
        out.append("# ---- bench.py --dump-outputs, A against B (same seeds)")
        out += ["# " + l.rstrip() for l in open(cmp_file)]
    if a.traces and all(os.path.exists(os.path.join(a.traces, f"timeline_{lib}.txt")) for lib in "ABC"):
        out.append("# ---- per-family totals of one replayed UNet pass (rocprofv3 --kernel-trace, tracing only, of bench.py --steps 10 --warmup 5 --windows 0; one run per library;")
        out.append("#      median per position over the replayed passes, tools/graph_trace.py)")
        tl = {lib: timeline(os.path.join(a.traces, f"timeline_{lib}.txt")) for lib in "ABC"}
        for lib in "ABC":
            rows, head = tl[lib]
            out.append(f"# {'parent (A)' if lib == 'A' else 'this tree (B)' if lib == 'B' else 'this tree, OSG_EPI_GENERIC=1 (C)'}: {head[0].lstrip('# ') if head else ''}")
            fam = {}
            for d, n in rows:
                e = fam.setdefault(family(n), [0, 0.0])
                e[0] += 1
                e[1] += d
            for f, (cnt, us) in sorted(fam.items(), key=lambda kv: -kv[1][1]):
                out.append(f"{f:<22} {cnt:>4} dispatches {us:>10.1f} us per pass {us / cnt:>8.2f} us each")
        ra, rb, rc = tl["A"][0], tl["B"][0], tl["C"][0]
        if len(ra) == len(rb) == len(rc):
            lean = [(x, y, z) for x, y, z in zip(ra, rb, rc) if "gemm2_kernel" in y[1] and not re.search(r", -1>", y[1]) and re.search(r"gemm2_kernel<(?:[^,>]*,){11}", y[1])]
            rest = [(x, y, z) for x, y, z in zip(ra, rb, rc) if "gemm2_kernel" in y[1] and (x, y, z) not in lean]
            out.append("# ---- gemm2_kernel dispatches position by position (the same plan in all three)")
            for what, grp in (("on a lean instantiation in B", lean), ("on EPI_ANY in B", rest)):
                if grp:
                    sa, sb, sc = (sum(t[k][0] for t in grp) for k in range(3))
                    slower = sum(1 for x, y, _ in grp if y[0] > x[0])
                    out.append(f"# {len(grp):>3} dispatches {what}: A {sa:.1f} us, B {sb:.1f} us ({(sb - sa) / len(grp):+.3f} us each), C {sc:.1f} us ({(sc - sa) / len(grp):+.3f} us each); "
                               f"B slower than A at {slower} positions")
            out.append("# position\tA us\tB us\tC us\tB - A\tkernel in B")
            for i, (x, y, z) in enumerate(zip(ra, rb, rc)):
                if "gemm2_kernel" in y[1]:
                    out.append(f"{i}\t{x[0]:.2f}\t{y[0]:.2f}\t{z[0]:.2f}\t{y[0] - x[0]:+.2f}\t{y[1][:100]}")
    open(a.out, "w").write("\n".join(out) + "\n")
    print("\n".join(l for l in out if l.startswith("#"))[:6000])


if __name__ == "__main__":
    main()
