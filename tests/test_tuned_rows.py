"""-m gpu: every row of the shipped tune table (onnxstream_amd/tune/mi355x.txt, the plan bench.py times) launched at its own shape through the public entry
point and compared element by element with float64 -- the launches tests/test_contraction_instantiations.py does not reach: thousands of workgroups, several
rounds of tiles per CU, the XCD-chunked tile walk, up to 360 k-tiles, ragged split-K, the in-kernel fold at full size.  tests/tuned_rows.py holds the decoding, the
expected routes and the references.

The table is process-wide and read once, so the rows run in child processes (tests/tuned_rows_worker.py), one per group of tuned_rows.GROUPS, each with
OSG_TUNE_CACHE = a copy of the table, OSG_TUNE_FROZEN = 1 and a time limit of its own.  Per row the child asserts that osg_last_route is the row's own choice,
checks every element, launches a fold row twice (same bits); per group osg_tune_misses() == 0: every launch found the row it was built from.  One case per
table line reads its own result line.  A child that times out, aborts or reports a device error ends its group: its remaining rows fail as not run, and
no further child is started (the remaining groups skip).

Seconds per group on an MI355X host with 16 threads (the float64 reference dominates: 0.1 to 5.3 s per row, 0.55 s on average, per row in
profiles/tuned_rows_table.txt) and the limits, 3 to 4 x and never under 45 s (a child's start costs a few seconds): LIMITS.  OSA_TUNED_ROWS_DIR keeps the
result lines for tools/tuned_rows_table.py."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import tuned_rows as tr

pytestmark = pytest.mark.gpu
ROWS = tr.rows()
# group: (seconds measured, limit)
LIMITS = {"sd15-unet": (13, 60), "sd15-decoder": (16, 60), "sdxl": (34, 120), "decoder-1024": (24, 90), "p4-unet": (20, 75), "p4-decoder": (31, 100),
          "w8a16": (9, 45)}
_results = {}
_ended = []          # the group whose child timed out, aborted or lost the device: nothing else is started


def group_of(r):
    return next(g for g, (lo, hi) in tr.GROUPS.items() if lo <= r.line <= hi)


def results_of(group, tmp_path_factory):
    if group in _results:
        return _results[group]
    if _ended:
        pytest.skip(f"the child of group {_ended[0]} did not finish: no further rows are launched")
    keep = os.environ.get("OSA_TUNED_ROWS_DIR")
    d = keep or str(tmp_path_factory.mktemp("tuned_rows"))
    os.makedirs(d, exist_ok=True)
    table, lines = os.path.join(d, f"{group}.tune.txt"), os.path.join(d, f"{group}.jsonl")
    shutil.copy(tr.TABLE, table)
    if os.path.exists(lines):
        os.remove(lines)
    env = dict(os.environ, OSG_TUNE_CACHE=table, OSG_TUNE_FROZEN="1")
    for k in list(env):
        if k.startswith(("OSG_GEMM_", "OSG_CONV3X3_", "OSG_SPLITK_")):      # (the per-process developer knobs would bypass the table)
            del env[k]
    try:
        rc = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_rows_worker.py"), group, lines], env=env,
                            timeout=LIMITS[group][1]).returncode
        status = "finished" if rc == 0 else f"exit status {rc}"
    except subprocess.TimeoutExpired:
        status = f"timed out after {LIMITS[group][1]} s"
    recs = [json.loads(x) for x in open(lines).read().splitlines()] if os.path.exists(lines) else []
    res = {"status": status, "rows": {x["line"]: x for x in recs if "line" in x}, "misses": next((x["misses"] for x in recs if "misses" in x), None)}
    assert open(table).read() == open(tr.TABLE).read(), "the frozen table was written to"
    if status != "finished":
        _ended.append(group)
    _results[group] = res
    return res


@pytest.mark.parametrize("r", ROWS, ids=[r.id for r in ROWS])
def test_tuned_row(r, tmp_path_factory):
    res = results_of(group_of(r), tmp_path_factory)
    rec = res["rows"].get(r.line)
    assert rec is not None, f"{r.id}: not run (its group's child: {res['status']})"
    print(json.dumps(rec))
    assert rec["ok"], rec.get("error")
    assert tuple(rec["route"]) == tr.expected_route(r).route and rec["worst"] <= 1.0 and rec["far"] <= tr.ci.FAR
    assert not r.fold or rec.get("relaunch") == "bit-equal"


@pytest.mark.parametrize("group", list(tr.GROUPS))
def test_every_launch_of_the_group_found_its_row(group, tmp_path_factory):
    res = results_of(group, tmp_path_factory)
    assert res["status"] == "finished", res["status"]
    assert res["misses"] == 0, f"{res['misses']} shapes missed the table: a row is unreachable from the call it describes"
