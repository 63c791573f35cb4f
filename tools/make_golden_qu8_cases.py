"""Generate tests/golden/qu8_cases.npz: for every case of tests/qu8_cases.py the range-data text (from the case's float64 restatement over its samples, in the
reference's text format), and for every case the reference accepts (oracle/_ref, `make -C oracle ref`) its dequantised value of every named tensor of sample 0 with
scale and zero point -- the reference run with m_use_uint8_arithmetic, every op output kept raw (oracle/qu8_check.run_u8_all), one thread.  Data only: the graphs and
inputs are re-emitted from the table's seeds and are not stored.

Prints two lists for the table: REFUSED (the reference's message: qu8_cases.REF_REFUSES, restatement-only cases) and DIFFERS (reference and interpreter disagree:
qu8_cases.REF_DIFFERS, which must be empty -- where they disagree the reference is right).

    python tools/make_golden_qu8_cases.py"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import qu8_cases as qcs  # noqa: E402


def run_reference(case, text):
    """tensor name -> (dequantised fp32 in the logical layout, scale, zero point) of sample 0, every activation the reference kept; raises with the reference's refusal"""
    from oracle import qu8_check as qc
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        case.emit(d)
        ops, vals = qc.run_u8_all(d, case.sample(0), text)
    prod = {qc.tname(o): op["type"] for op in ops for o in op["outputs"]}
    out = {}
    for n, v in vals.items():
        if v["dtype"] != 1:
            continue
        codes = v["data"].transpose(0, 3, 1, 2) if prod.get(n) == "Conv" else v["data"]          # (a Conv's output is kept channels-last)
        out[n] = (qcs.deq(np.ascontiguousarray(codes), v["scale"], v["zp"]), np.float32(v["scale"]), int(v["zp"]))
    return out


def compare(case, ref, want):
    """-> what differs between the reference's tensors and the interpreter's (empty: nothing)"""
    bad = []
    for n in case.intermediates():
        if n not in ref:
            bad.append(f"{n}: not kept by the reference")
            continue
        codes, s, z = want[n]
        r = ref[n]
        if r[0].shape != codes.shape:
            bad.append(f"{n}: shape {r[0].shape} / {codes.shape}")
        elif np.float32(s) != r[1] or z != r[2]:
            bad.append(f"{n}: parameters ({r[1]!r}, {r[2]}) / ({s!r}, {z})")
        elif not np.array_equal(qcs.deq(codes, s, z), r[0]):
            bad.append(f"{n}: {int((qcs.deq(codes, s, z) != r[0]).sum())} of {codes.size} values differ")
    return bad


if __name__ == "__main__":
    from onnxstream_amd.bindings import OnnxStreamError
    from oracle import ref as oref
    assert oref.available(), "build the oracle first: make -C oracle ref"
    store, index, blob, refused, differs = {}, [], [], {}, {}
    for c in qcs.CASES:
        store["ranges|" + c.name] = np.asarray(c.computed_range_text())
    qcs._GOLDEN = ({k.split("|", 1)[1]: str(v) for k, v in store.items()}, {})
    for c in qcs.planned():
        try:
            ref = run_reference(c, qcs.range_text(c))
        except (OnnxStreamError, RuntimeError, AssertionError) as e:
            refused[c.name] = str(e)
            continue
        bad = compare(c, ref, qcs.want(c, 0))
        if bad:
            differs[c.name] = bad
        for n in c.intermediates():
            if n in ref:
                index.append((f"{c.name}|{n}", list(ref[n][0].shape), float(ref[n][1]), ref[n][2]))
                blob.append(ref[n][0].reshape(-1))
    path = os.path.join(REPO, "tests", "golden", "qu8_cases.npz")
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index).encode(), np.uint8), ref=np.concatenate(blob).astype(np.float32), **store)
    print(f"{len(index)} tensors of {len(qcs.planned()) - len(refused)} cases, range data of {len(qcs.CASES)} -> {path} ({os.path.getsize(path)} bytes)")
    for n, msg in refused.items():
        print(f"REFUSED {n}: {msg}")
    for n, bad in differs.items():
        print(f"DIFFERS {n}: {bad}")
