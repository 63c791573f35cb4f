"""Print the measured figures of the per-operator lowering table (tests/op_cases.py) on the device: per case, over fusion {0, 2} x {1, 3} pushes x every
sample and output, the largest distance in f16 ulps to the float64 restatement, for the "reduce" cases the largest error / bound, and err16 to the
reference's fp16 output where tests/golden/op_cases.npz has one.  profiles/op_lowering_table.txt is this tool's output on an MI355X.

    python tools/op_lowering_table.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import op_cases as oc  # noqa: E402

print(f"{'case':44s} {'class':11s} {'ulps':>4s} {'err/bound':>9s} {'err16':>9s}  failures")
for c in oc.device_cases():
    ulps, ratio, e16, fails = 0, None, None, []
    for fusion in (0, 2):
        for pushes in (1, 3):
            got = oc.run_case(c, pushes, fusion)
            for o in c.outs:
                for k, g in enumerate(got[o]):
                    fig, bad = oc.figures(c, o, g, k)
                    fails += [f"f{fusion} p{pushes} s{k} {o}: {b}" for b in bad]
                    ulps = max(ulps, fig.get("ulps", 0))
                    if "ratio" in fig:
                        ratio = max(ratio or 0.0, fig["ratio"])
                    gold = oc.golden(c, o) if k == 0 else None
                    if gold and g.shape == gold[0].shape:
                        e16 = max(e16 or 0.0, oc.err16(g, *gold))
    print(f"{c.name:44s} {c.cls:11s} {ulps:4d} {'-' if ratio is None else f'{ratio:9.3f}':>9s} {'-' if e16 is None else f'{e16:9.2e}':>9s}  {'; '.join(fails)}", flush=True)
