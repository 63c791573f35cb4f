"""-m gpu: the launch choice of onnxstream_amd/csrc/osg_gemm_select.h as the launchers apply it.

* Default routes.  No override variable, autotune off: each public entry point must run what the driver (tests/cpp/contraction_select.cpp) computes for the
  device's own CU count -- model_choice / model_halo3 / choose_v1 resolved through resolve_v2 / resolve3, the k-slices of split_slices -- and its output is
  compared with float64 by the operands, references and bounds of tests/tuned_rows.py and tests/test_contraction_instantiations.py.
* The measuring path, in a child process with an empty OSG_TUNE_CACHE (tests/select_measure_worker.py): the first launch of a shape appends exactly one row, a
  launchable one out of the driver's candidate list for the shape; the second launch misses nothing and runs the route the row names.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import select_measure_worker as worker
import test_contraction_select_cpu as sel
import tuned_rows as tr
from test_shipped_artifacts_cpu import _launchable
from test_tblock_tail_float64 import num_cu      # (torch's count of the device's CUs; 256, the MI355X, where torch sees no device)

pytestmark = pytest.mark.gpu
ci = tr.ci
GEGLU, F32BIAS, LN, RS_OUT, W8 = sel.GEGLU, sel.F32BIAS, sel.LN, sel.RS_OUT, sel.W8

# (name, how it is launched, key)
CASES = [("gemm-64x64x64", "row", sel.gemm_key(64, 64, 64)),
         ("gemm-64x320x2560-split", "row", sel.gemm_key(64, 320, 2560)),
         ("gemm-256x1280x320", "row", sel.gemm_key(256, 1280, 320)),
         ("gemm-64x320x72-register-staged", "v1", sel.gemm_key(64, 320, 72)),
         ("gemm-geglu-64x640x1280", "row", sel.gemm_key(64, 640, 1280, GEGLU)),
         ("gemm-ln-64x320x1280", "row", sel.gemm_key(64, 320, 1280, LN | F32BIAS)),
         ("gemm-rowstats-64x320x1280", "row", sel.gemm_key(64, 320, 1280, RS_OUT)),
         ("gemm-w8-64x320x2560", "row", sel.gemm_key(64, 320, 2560, W8)),
         ("gemm-w8-geglu-64x640x1280", "row", sel.gemm_key(64, 640, 1280, W8 | GEGLU)),
         ("conv3x3-8x8-1280-to-320-halo-split", "row", sel.halo_key(8, 1280)),
         ("conv3x3-16x16-64-to-320-halo-one-slab", "row", sel.halo_key(16, 64)),
         ("conv3x3-stride2-16x16-64-to-64-implicit-gemm", "row", (2, 0, 64, 64, 576, 1, 16, 16, 64, 3, 2, 2, 0)),
         ("conv1x1-8x8-320-to-320-gemm-path", "conv1x1", sel.gemm_key(64, 320, 320)),
         ("conv3x3-w8-8x8-1280-to-320-halo", "row", sel.halo_key(8, 1280, flags=W8))]


@pytest.fixture(scope="module")
def plans():
    """the driver's plan of every key this module launches, for the device's CU count"""
    cus = num_cu()
    keys = [c[2] for c in CASES] + [k for k in worker.KEYS]
    return {r["key"]: r for r in sel.parse_plan(sel.plan(cus, keys))}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_default_route_is_the_models_choice(gpu, plans, case, monkeypatch):
    name, how, key = case
    ci.knobs(monkeypatch)
    gpu._ck(gpu.lib.osg_set_autotune(gpu.ctx, 0))
    rec = plans[key]
    line = 2 * (CASES.index(case) + 1)
    if how == "v1":
        assert rec["model"][0] == ci.GEMM_V1
        M, N, K = key[2:5]
        rng = np.random.default_rng(line)
        a, w, bias, res = ci.rnd(rng, (M, K)), ci.rnd(rng, (N, K), K ** -0.5), ci.rnd(rng, (N,), 0.1), ci.rnd(rng, (M, N))
        got, route = ci.gemm(gpu, a, w, bias, res, ci.ACT_NONE)
        assert route == (*rec["route"], 0, ci.reduce_kernel(rec["route"][2], 0, N)), (route, rec)
        ci.check(got, *ci.contraction(a, w, bias, res), name)
        return
    row = tr.Row(line, *key, *rec["model"])
    want = tr.expected_route(row)
    assert want.route[:3] == rec["route"] and want.route[3] == 0, (want.route, rec)      # (the Python restatement and the driver agree before anything is launched)
    c = tr.Case(row)
    if how == "conv1x1":      # the GEMM over the pixels, entered through the convolution
        n, k = key[3], key[4]
        got, route = ci.conv(gpu, c.a.reshape(1, 8, 8, k), c.w.reshape(n, 1, 1, k), c.bias, None, None, ci.ACT_NONE, 1, 0)
    else:
        got, route = c.launch(gpu)
    assert tuple(route) == want.route, f"{name}: osg_last_route {tuple(route)}, the model's choice {rec['model']} runs {want.route}"
    worst, far = c.compare(got)
    print(f"{name}: model {rec['model']} route {want.route} worst {worst:.3f} x the bound, {far:.4f} more than one ulp off")


def test_a_measured_choice_goes_to_the_table_once_and_is_reused(plans, tmp_path):
    cache, results = tmp_path / "tune.txt", tmp_path / "launches.jsonl"
    cache.write_text("")
    env = {k: v for k, v in os.environ.items() if not k.startswith(("OSG_GEMM_", "OSG_CONV3X3_", "OSG_SPLITK_", "OSG_TUNE_"))}
    env["OSG_TUNE_CACHE"] = str(cache)
    done = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "select_measure_worker.py"), str(results)], env=env, timeout=150)
    assert done.returncode == 0, f"the child ended with status {done.returncode}"
    recs = [json.loads(x) for x in results.read_text().splitlines()]
    assert [(r["launch"], tuple(r["key"])) for r in recs] == [(n, k) for n in (1, 2) for k in worker.KEYS]
    rows = {}
    for i, r in enumerate(recs[:len(worker.KEYS)]):
        key = tuple(r["key"])
        assert len(r["table"]) == i + 1 and r["misses"] == i + 1, f"{key}: the first launch stores one row ({len(r['table'])} lines, {r['misses']} misses)"
        f = r["table"][-1].split()
        assert tuple(map(int, f[:13])) == key and float(f[18]) > 0, r["table"][-1]
        choice = tuple(map(int, f[13:18]))
        assert _launchable(*choice), f"{key}: the stored row {choice} names no launchable configuration"
        assert choice in plans[key]["cands"], f"{key}: the stored row {choice} is none of the {len(plans[key]['cands'])} candidates"
        rows[key] = tr.Row(i + 1, *key, *choice)
    for r in recs:
        key = tuple(r["key"])
        assert tuple(r["route"]) == tr.expected_route(rows[key]).route, f"{key}, launch {r['launch']}: ran {r['route']}, the stored row is {rows[key]}"
        assert r["worst"] <= 1.0 and r["far"] <= ci.FAR
        if r["launch"] == 2:
            assert r["misses"] == len(worker.KEYS) and len(r["table"]) == len(worker.KEYS), f"{key}: the second launch missed or stored again"
