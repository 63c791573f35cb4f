#!/usr/bin/env python3
"""profiles/epilogue_forms_table.txt: for every (entry of kV2Entries, form of fused epilogue) pair the shipped SD 1.5 plan launches, the launches per UNet pass and
what the pair's code looks like outside its k loop -- the code a workgroup walks once per launch (tools/isa_phases.py) -- in the entry's
EPI_ANY instantiation and, where kLeanEntries (onnxstream_amd/csrc/osg_gemm_epi.h) holds the pair, in its lean instantiation.

Two inputs:
  * the launch log of one benchmark run -- `OSG_EPI_LOG=1 python bench.py --gpus 1 --steps 2 --warmup 1 --cpu-passes 0 --windows 0 2> LOG`: one `[epi]` line per
    gemm2_kernel launch; the first run of lines with capturing=1 is the captured UNet pass, the second the VAE decoder (once per image).  The forms depend on
    what the planner hands each launch at run time (second destinations, statistics sinks, pitches, alignment), which is why they are read from a run of the plan
    and not from the tune table's keys;
  * the built libosgpu.so, disassembled here (no GPU).

Columns: instructions and branch instructions OUTSIDE the innermost MFMA loop.  A lean instantiation holds the path its form executes and nothing else, so its
figures are the instructions / branches on the executed path; `removed` is what EPI_ANY carries beyond that (skipped over by taken branches or never reached).

    python tools/epilogue_forms_table.py LOG [-o profiles/epilogue_forms_table.txt]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_loops as il            # noqa: E402
import kernel_resources as kr     # noqa: E402

BITS = ("bias16", "bias32", "rowbias", "residual", "silu", "c2", "rowstats", "split", "fold", "geglu", "sinks", "other")


def form_name(mask):
    return "+".join(n for k, n in enumerate(BITS) if mask >> k & 1) or "plain"


def driver(src, *modes):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "drv")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"), os.path.join(REPO, "tests", "cpp", src), "-o", exe], check=True)
        return [subprocess.run([exe, m], stdout=subprocess.PIPE, text=True, check=True).stdout for m in modes]


def kernels(lib):
    """{(bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, epi): (instructions, instructions outside the k loop, branches outside it)} of every gemm2_kernel"""
    out = {}
    blob = open(lib, "rb").read()
    for _, obj in kr.code_objects(blob):
        if not obj.startswith(b"\x7fELF"):
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            lines = subprocess.run([il.OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout.split("\n")
        for name, i, e in il.functions(lines):
            m = re.search(r"gemm2_kernel<([^>]*)>", name)
            if not m or "q8_" in name:
                continue
            a = [{"false": 0, "true": 1}.get(t.strip(), t.strip()) for t in m.group(1).split(",")]
            a = [int(t) for t in a]
            if len(a) == 11:
                a.append(-1)
            key = tuple(a[:4] + a[5:])                 # (MODE is 0 everywhere)
            body = lines[i:e]
            base = int(re.match(r"^([0-9a-f]+) <", body[0]).group(1), 16)
            ins = []
            for l in body:
                mm = re.match(r"\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):", l)
                if mm:
                    ins.append((int(mm.group(3), 16) - base, mm.group(1), l))
            a2i = {ad: k for k, (ad, _, _) in enumerate(ins)}
            loop = None
            for k, (ad, op, l) in enumerate(ins):
                if op.startswith("s_cbranch") or op == "s_branch":
                    t = re.search(r"<[^>]*\+0x([0-9a-f]+)>", l)
                    if t and int(t.group(1), 16) <= ad and int(t.group(1), 16) in a2i:
                        s = a2i[int(t.group(1), 16)]
                        if any(o.startswith("v_mfma") for (_, o, _) in ins[s:k + 1]) and (loop is None or k - s < loop[1] - loop[0]):
                            loop = (s, k)
            inside = set(range(loop[0], loop[1] + 1)) if loop else set()
            outside = [op for k, (_, op, _) in enumerate(ins) if k not in inside]
            out[key] = (len(ins), len(outside), sum(1 for op in outside if op.startswith("s_cbranch") or op == "s_branch"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "epilogue_forms_table.txt"))
    ap.add_argument("--lib", default=os.path.join(REPO, "onnxstream_amd", "libosgpu.so"))
    a = ap.parse_args()
    entries_txt, = driver("contraction_routes.cpp", "entries")
    v2 = [tuple(map(int, l.split()[1:11])) for l in entries_txt.splitlines() if l.startswith("v2 ")]
    lean_txt, = driver("epilogue_select.cpp", "list")
    lean = {}
    for l in lean_txt.splitlines():
        f = l.split()
        if f[0] == "lean":
            lean[(int(f[2]), int(f[13]))] = int(f[1])
    rows = [dict((k, int(v)) for k, v in re.findall(r"(\w+)=(-?\d+)", l)) for l in open(a.log) if l.startswith("[epi]")]
    runs, prev = [], 0
    for r in rows:
        if r["capturing"] and not prev:
            runs.append([])
        if r["capturing"]:
            runs[-1].append(r)
        prev = r["capturing"]
    if not runs:
        raise SystemExit("no captured launches in the log")
    code = kernels(a.lib)
    out = ["# (entry, epilogue form) pairs of the shipped SD 1.5 plan: launches per pass and the code outside the k loop -- tools/epilogue_forms_table.py (see its docstring)",
           "# entry = index in kV2Entries, BMxBN-nNST and its options; form = what the launch's fused epilogue contains (osg_gemm_epi.h epi_form); whole = the launches of the pair that",
           "# run whole tiles with 8-byte aligned rows (only those take a lean instantiation); lean = index in kLeanEntries (-: the pair stays with EPI_ANY)",
           "# any / lean: instructions (branch instructions) outside the innermost MFMA loop of the EPI_ANY / the lean instantiation; removed = any - lean; weight = launches x removed"]
    for title, run in (("UNet pass", runs[0]),) + ((("VAE decoder (once per image)", runs[1]),) if len(runs) > 1 else ()):
        pairs = collections.OrderedDict()
        for r in run:
            p = pairs.setdefault((r["entry"], r["form"]), dict(n=0, nwhole=0, shapes=set()))
            p["n"] += 1
            p["nwhole"] += 1 if r["whole"] else 0
            p["shapes"].add((r["M"], r["N"], r["K"], r["splits"]))
        table = []
        for (entry, form), p in pairs.items():
            e = v2[entry]
            any_ = code.get(e + (-1,))
            li = lean.get((entry, form))
            ln = code.get(e + (form,)) if li is not None else None
            removed = any_[1] - ln[1] if any_ and ln else None
            table.append((-(p["n"] * removed) if removed is not None else 1, -p["n"], entry, form, p, e, any_, li, ln, removed))
        table.sort(key=lambda t: t[:4])
        total = sum(p["n"] for p in pairs.values())
        covered = sum(t[4]["nwhole"] for t in table if t[7] is not None)
        out.append(f"# ---- {title}: {total} gemm2_kernel launches, {len(pairs)} pairs; {covered} launches ({100.0 * covered / total:.1f} %) run a lean instantiation")
        out.append(f"# {'entry':<34} {'form':<28} {'launches':>8} {'whole':>5} {'lean':>4} {'any':>12} {'lean':>12} {'removed':>7} {'weight':>7}  shapes M x N x K (k-slices)")
        for _, _, entry, form, p, e, any_, li, ln, removed in table:
            name = f"{entry:3d} {e[0]}x{e[1]}-n{e[2]}" + ("-conv" if e[3] else "") + ("-spec" if e[4] else "") + (f"-ln{e[5]}-nch{e[6]}" if e[5] else "") + ("-ks2" if e[7] == 2 else "")
            fa = f"{any_[1]} ({any_[2]})" if any_ else "?"
            fl = f"{ln[1]} ({ln[2]})" if ln else "-"
            shapes = ", ".join(f"{m}x{n}x{k}" + (f" ({s})" if s > 1 else "") for m, n, k, s in sorted(p["shapes"]))
            out.append(f"{name:<36} {form_name(form):<28} {p['n']:>8} {p['nwhole']:>5} {li if li is not None else '-':>4} {fa:>12} {fl:>12} "
                       f"{removed if removed is not None else '-':>7} {p['n'] * removed if removed is not None else '-':>7}  {shapes}")
    open(a.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))


if __name__ == "__main__":
    main()
