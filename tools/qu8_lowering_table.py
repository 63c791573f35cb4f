"""Print the uint8 lowering table (tests/qu8_cases.py) as run on the device: per planned case and fusion level the launches of one pass and the number of
codes compared with the interpreter (four passes; at level 0 every intermediate as well), all bit for bit -- the checks are those of
tests/test_qu8_lowering_gpu.py, a failure is printed in the last column.  profiles/qu8_lowering_table.txt is this tool's output on an MI355X.

    python tools/qu8_lowering_table.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import qu8_cases as qcs  # noqa: E402
import test_qu8_lowering_gpu as tg  # noqa: E402

lines = ["# python tools/qu8_lowering_table.py on an MI355X (gfx950): per planned case of tests/qu8_cases.py and fusion level, the launches of one pass and the codes",
         "# compared bit for bit with the interpreter over the four passes A, A, 0.37 A + 0.2, A (level 0: every intermediate too); ref: the reference's stored output holds the case",
         f"{'case':44s} {'expect':8s} {'ref':3s} {'launches 0':>10s} {'codes 0':>8s} {'launches 1':>10s} {'codes 1':>8s}  failures"]
print("\n".join(lines), flush=True)
for c in qcs.planned():
    fig, fails = [], []
    for level in qcs.LEVELS:
        try:
            fig += list(tg.check_case(c, level))
        except AssertionError as e:
            fig += [-1, -1]
            fails.append(f"level {level}: {str(e)[:160]}")
    lines.append(f"{c.name:44s} {c.expect or '-':8s} {'no' if c.name in qcs.REF_REFUSES else 'yes':3s} {fig[0]:10d} {fig[1]:8d} {fig[2]:10d} {fig[3]:8d}  {'; '.join(fails)}".rstrip())
    print(lines[-1], flush=True)
open(os.path.join(REPO, "profiles", "qu8_lowering_table.txt"), "w").write("\n".join(lines) + "\n")
