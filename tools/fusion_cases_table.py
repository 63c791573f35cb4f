"""Write profiles/fusion_cases_table.txt: the table of tests/fusion_cases.py run on the device -- per case and fusion level the err16 against
tests/golden/fusion_cases.npz (max|got - ref16| / max|ref32|, worst output) and the largest distance in f16 ulps to the float64 restatement, then the level 2 step
list.  Where a class rule applies to `out` at a level (fusion_cases' `rule`), its error / bound follows the rule's name (the elementwise rule is the ulps figure).  The
figures that tests/test_fusion_cases_gpu.py asserts on; "exception" marks a figure held by fusion_cases.EXCEPTIONS, "<--" one that the test would refuse.

    python tools/fusion_cases_table.py [OUT]"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fusion_cases as fc  # noqa: E402


def main(out):
    from onnxstream_amd.bindings import OnnxStreamError
    lines = ["# tools/fusion_cases_table.py: per case and fusion level, err16 = max|got - ref16| / max|ref32| against tests/golden/fusion_cases.npz (worst output)",
             "# and the largest distance in f16 ulps to the float64 restatement; then the level 2 plan.  One pushed sample.", ""]
    for c in fc.planned():
        cells, steps = [], None
        for level in fc.LEVELS:
            try:
                got, kinds, what = fc.run(c, level)
            except OnnxStreamError as e:
                if "memory access" in str(e) or "hipError" in str(e):
                    raise SystemExit(f"{c.name}: the device reported a fault, nothing more is launched: {e}")
                cells.append(f"L{level} REFUSED {e}")
                continue
            e16, ulps, bad, rule = 0.0, 0, [], ""
            for o in c.outs:
                if not got[o]:
                    bad.append(f"{o}: None")
                    continue
                fig, b = fc.check_output(c, level, o, got[o][0])
                bad += [f"{o}: {x}" for x in b]
                e16, ulps = max(e16, fig.get("err16", 0.0)), max(ulps, fig.get("ulps", 0))
                if "ratio" in fig:
                    rule = f" {c.rule} {fig['ratio']:.2f}"
            cells.append(f"L{level} err16 {e16:.2e} ulps {ulps:3d}{rule}" + ("  exception" if e16 > 1e-3 and not bad else "") + (f"  <-- {'; '.join(bad)}" if bad else ""))
            if level == 2:
                steps = kinds
                if kinds != c.plan:
                    cells[-1] += f"  <-- plan, expected {c.plan}"
        lines.append(f"{c.name:48s} {c.pass_:20s} {c.expect:8s} " + " | ".join(cells))
        lines.append(f"{'':48s} level 2: {' '.join(steps or [])}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(fc.planned())} cases -> {out}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "fusion_cases_table.txt"))
