"""Generate tests/golden/fusion_cases.npz from the reference (oracle/_ref, `make -C oracle ref`): every case of tests/fusion_cases.py that plans, one pushed sample: the
outputs of the fp16-arithmetic run as f16 values and max|output| of the fp32-arithmetic run, the extra outputs of a case included, packed as fusion_cases.load_golden reads them.  The reference
runs each graph as written, op by op: none of its own rewrites is switched on (the upcast substrings of a case are, they are part of its graph's meaning).  The graphs
and inputs are re-emitted from the table's seeds and are not stored.  Cases the reference refuses are printed with its message: they go into fusion_cases.REF_REFUSES
(restatement-only).

    python tools/make_golden_fusion.py"""
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import fusion_cases as fc  # noqa: E402
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
            if case.upcast:
                m.set_upcast_substrings(case.upcast)
            for name in case.extra_outs:
                m.add_extra_output(name)
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
    index, blob, maxes, refused = [], [], [], {}
    for c in fc.planned():
        try:
            o16, o32 = run_reference(c, True), run_reference(c, False)
        except OnnxStreamError as e:
            refused[c.name] = str(e)
            continue
        want = c.want(0)
        for o in c.outs:
            h = o16[o].astype(np.float16)
            assert np.array_equal(oc.bits(h.astype(np.float32)), oc.bits(o16[o])), (c.name, o, "the fp16 path's output is not made of f16 values")
            index.append((f"{c.name}|{o}", list(h.shape)))
            blob.append(h.reshape(-1)[::fc.golden_stride(h.size)])
            maxes.append(np.abs(o32[o]).max())
            w = want[o].astype(np.float16).astype(np.float32)
            if o16[o].shape != w.shape:
                print(f"SHAPE {c.name} {o}: reference {o16[o].shape} restatement {w.shape}")
                continue
            e16 = oc.err16(w, o16[o], o32[o])
            if e16 > 1e-3:
                print(f"VALUE {c.name} {o}: |restatement - ref16| / max|ref32| = {e16:.2e}")
    path = os.path.join(REPO, "tests", "golden", "fusion_cases.npz")
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index).encode(), np.uint8), ref16=np.concatenate(blob), ref32max=np.asarray(maxes, np.float32))
    print(f"{len(index)} outputs of {len(fc.planned()) - len(refused)} cases -> {path} ({os.path.getsize(path)} bytes)")
    for n, msg in refused.items():
        print(f"REFUSED {n}: {msg}")
