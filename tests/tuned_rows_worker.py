"""The child process of tests/test_tuned_rows.py: python tuned_rows_worker.py GROUP RESULTS.  The tune table is process-wide and read once, so the parent
starts this with OSG_TUNE_CACHE = a copy of the shipped table and OSG_TUNE_FROZEN = 1.  One context with autotune on; the rows of the group in table order,
each: operands, the launch through the public entry point, osg_last_route against the expected route, every element against float64; a fold row is launched
again and must give the same bits (the tickets were restored).  One JSON line per row is appended to RESULTS as the row finishes, a last line holds
osg_tune_misses().  A failed comparison is recorded and the walk goes on; an error of the device ends it (exit status 3): the rows left are not run."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(group, results):
    import numpy as np

    import tuned_rows as tr
    from onnxstream_amd import osgpu
    assert os.environ.get("OSG_TUNE_CACHE") and os.environ.get("OSG_TUNE_FROZEN") == "1", "the parent sets the table and freezes it"
    gpu = osgpu.Gpu(0)
    gpu._ck(gpu.lib.osg_set_autotune(gpu.ctx, 1))
    status = 0
    with open(results, "a") as out:
        for r in tr.group_rows(group):
            t0 = time.time()
            rec = {"line": r.line, "id": r.id, "ok": False}
            case = got = again = None
            try:
                case = tr.Case(r)
                e = case.route
                rec.update(expected=list(e.route), workgroups=e.workgroups, structured=case.structured)
                got, route = case.launch(gpu)
                rec["route"] = list(route)
                assert tuple(route) == e.route, f"{r.id}: osg_last_route {tuple(route)}, the row's choice is {e.route}"
                rec["worst"], rec["far"] = case.compare(got)
                if e.route[3]:
                    again, route = case.launch(gpu)
                    assert tuple(route) == e.route, f"{r.id}: second launch ran {tuple(route)}"
                    assert np.array_equal(again.view(np.uint16), got.view(np.uint16)), f"{r.id}: the second launch of the fold differs from the first"
                    rec["relaunch"] = "bit-equal"
                rec["ok"] = True
            except AssertionError as err:
                rec["error"] = str(err)[:600]
            except osgpu.OsgError as err:
                rec["error"] = f"device error, the walk ends here: {err}"[:600]
                status = 3
            rec["seconds"] = round(time.time() - t0, 2)
            out.write(json.dumps(rec) + "\n")
            out.flush()
            if status:
                return status
        out.write(json.dumps({"group": group, "misses": int(gpu.lib.osg_tune_misses())}) + "\n")
    gpu.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
