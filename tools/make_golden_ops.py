"""Generate tests/golden/op_cases.npz from the reference (oracle/_ref, `make -C oracle ref`): every case of tests/op_cases.py that reaches the device, one pushed
sample, with fp16 arithmetic (`<case>|<output>|ref16`, stored as f16 where that is lossless) and fp32 arithmetic (`...|ref32`).  The graphs and inputs are re-emitted from the table's seeds and are not
stored.  Cases the reference refuses are printed with its message: they go into op_cases.REF_REFUSES (restatement-only).

    python tools/make_golden_ops.py"""
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import op_cases as oc  # noqa: E402


def run_reference(case, fp16):
    """output name -> fp32 array of sample 0; raises OnnxStreamError with the reference's refusal"""
    from onnxstream_amd.bindings import Model
    from onnxstream_amd.synth.graph import DirSink
    from oracle import ref as oref
    with tempfile.TemporaryDirectory() as d:
        d += "/"
        oc.emit(case, DirSink(d))
        m = Model(oref.REF_LIB, 1, "ram+nocache")
        try:
            if case.dynamic:
                m.set_support_dynamic_shapes(True)
            if case.upcast:
                m.set_upcast_substrings(case.upcast)
            m.read_file(d + "model.txt")
            m.set_use_fp16_arithmetic(False)          # inputs enter as fp32 through model_add_tensor
            for name, arr in case.sample(0).items():
                m.add_tensor(name, arr)
            m.set_use_fp16_arithmetic(fp16)
            m.run()
            out = {}
            for o in case.outs:
                got = m.get_tensor(o)
                assert got is not None, (case.name, o)
                out[o] = got[0]
        finally:
            m.close()
    return out


if __name__ == "__main__":
    from onnxstream_amd.bindings import OnnxStreamError
    from oracle import ref as oref
    assert oref.available(), "build the oracle first: make -C oracle ref"
    data, refused = {}, {}
    for c in oc.device_cases():
        try:
            o16, o32 = run_reference(c, True), run_reference(c, False)
        except OnnxStreamError as e:
            refused[c.name] = str(e)
            continue
        want = c.want(0)
        for o in c.outs:
            h = o16[o].astype(np.float16)           # (the fp16 path's outputs are f16 values: kept as f16 where that loses nothing)
            data[f"{c.name}|{o}|ref16"] = h if np.array_equal(oc.bits(h.astype(np.float32)), oc.bits(o16[o])) else o16[o]
            data[f"{c.name}|{o}|ref32"] = o32[o]
            w = want[o].astype(np.float16).astype(np.float32)
            if o16[o].shape != w.shape:
                print(f"SHAPE {c.name} {o}: reference {o16[o].shape} restatement {w.shape}")
            elif c.cls == "move" and not np.array_equal(oc.bits(w), oc.bits(o16[o])):
                print(f"VALUE {c.name} {o}: the restatement is not the reference's output bit for bit")
            elif c.cls != "move":
                err = float(np.abs(w.astype(np.float64) - o16[o]).max()) / max(float(np.abs(o32[o]).max()), 1e-30)
                if err > 1e-3:
                    print(f"VALUE {c.name} {o}: |restatement - ref16| / max|ref32| = {err:.2e}")
    path = os.path.join(REPO, "tests", "golden", "op_cases.npz")
    np.savez_compressed(path, **data)
    print(f"{len(data) // 2} outputs of {len(oc.device_cases()) - len(refused)} cases -> {path} ({os.path.getsize(path)} bytes)")
    for n, msg in refused.items():
        print(f"REFUSED {n}: {msg}")
