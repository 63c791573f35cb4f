#!/usr/bin/env python3
"""profiles/tuned_rows_table.txt from the result lines of tests/test_tuned_rows.py: one line per row of the shipped tune table -- the route osg_last_route
reported, the k-slices and workgroups of the launch, the worst |got - want| / bound over every output element, the share of elements more than one f16 ulp from the
correctly rounded float64 result, the host seconds of the row (operands, launch, reference, comparison).

    OSA_TUNED_ROWS_DIR=<dir> python -m pytest -m gpu tests/test_tuned_rows.py        # keeps <dir>/<group>.jsonl
    python tools/tuned_rows_table.py <dir> [-o profiles/tuned_rows_table.txt]
"""
import argparse
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("-o", "--out", default=os.path.join(REPO, "profiles", "tuned_rows_table.txt"))
    a = ap.parse_args()
    import tuned_rows as tr
    recs, misses = {}, {}
    for path in sorted(glob.glob(os.path.join(a.dir, "*.jsonl"))):
        for text in open(path).read().splitlines():
            x = json.loads(text)
            if "line" in x:
                recs[x["line"]] = x
            else:
                misses[x["group"]] = x["misses"]
    rows = tr.rows()
    group = {r.line: g for g in tr.GROUPS for r in tr.group_rows(g)}
    ok = sum(1 for r in rows if recs.get(r.line, {}).get("ok"))
    out = [f"# every row of onnxstream_amd/tune/mi355x.txt at its own shape against float64 (tests/test_tuned_rows.py): {ok} of {len(rows)} rows pass",
           "# route = osg_last_route (family, entry, k-slices, fold, reduce kernel); ref = b brute-force / s structured reference; worst = max |got - want| / bound;",
           "# far = share of elements more than one f16 ulp from the correctly rounded result; s = host seconds of the row; a fold row's relaunch is bit-equal",
           "# tune-table misses per group: " + (", ".join(f"{g} {misses[g]}" for g in tr.GROUPS if g in misses) or "none recorded"),
           f"# {'row':<44} {'group':<13} {'route':<18} {'slices':>6} {'workgroups':>10} ref {'worst':>6} {'far':>8} {'s':>6}  result"]
    for r in rows:
        x = recs.get(r.line)
        if x is None:
            out.append(f"{r.id:<46} {group[r.line]:<13} not run")
            continue
        route = x.get("route") or x.get("expected") or []
        res = "ok" + (", relaunch bit-equal" if x.get("relaunch") else "") if x["ok"] else "FAILED: " + x.get("error", "")[:160]
        out.append(f"{r.id:<46} {group[r.line]:<13} {','.join(map(str, route)):<18} {route[2] if route else '':>6} {x.get('workgroups', ''):>10} "
                   f"{'s' if x.get('structured') else 'b':>3} {x.get('worst', float('nan')):>6.3f} {x.get('far', float('nan')):>8.5f} {x['seconds']:>6.1f}  {res}")
    secs = {g: sum(recs[r.line]["seconds"] for r in tr.group_rows(g) if r.line in recs) for g in tr.GROUPS}
    out.append("# seconds per group: " + ", ".join(f"{g} {s:.0f}" for g, s in secs.items()))
    open(a.out, "w").write("\n".join(out) + "\n")
    print(f"{a.out}: {ok} of {len(rows)} rows pass; seconds per group {secs}")


if __name__ == "__main__":
    main()
