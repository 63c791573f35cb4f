"""No GPU: the hot kernels of the built libosgpu.so ask for their leading scalar parameters to be preloaded into user SGPRs.

gfx950 delivers up to 14 dwords of kernel arguments in scalar registers at wave start, but only leading scalar / pointer parameters: a by-value struct is not
preloaded, and a kernel that takes its arguments as one declares a preload length of 0.  The contraction, attention and transformer-tail kernels therefore take
what their first memory requests depend on as flat parameters in front of their struct, and the build passes the flag that asks for the preload
(onnxstream_amd/build.py).  Read from the library itself: the length each kernel descriptor declares (tools/kernel_resources.py preload_lengths) against the dword
count of the kernel's leading scalar parameters in the code object's metadata.
"""
import os
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 14        # 16 user SGPRs less the two of the argument-segment pointer
FAMILIES = ("gemm2_kernel", "conv3x3_kernel", "attn2_kernel", "tblock_tail_kernel", "gn_slab_kernel", "splitk_reduce4_kernel")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None, reason="needs llvm-readelf and c++filt")
def test_hot_kernels_declare_their_leading_parameters_preloaded():
    from onnxstream_amd import build as b
    if not os.path.exists(b.LIB_GPU):
        import __graft_entry__ as ge
        ge.build()
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources as kr
    blob = open(b.LIB_GPU, "rb").read()
    rows, declared = [], {}
    for _, obj in kr.code_objects(blob):
        if obj.startswith(b"\x7fELF"):
            rows += list(kr.kernels_of(obj))
            declared.update(kr.preload_lengths(obj))
    names = kr.demangle([r["name"] for r in rows])
    seen = {f: 0 for f in FAMILIES}
    for r, n in zip(rows, names):
        # (a name c++filt could not demangle -- binutils does not know the mangling of _Float16 -- still holds the length-prefixed identifier and its template list)
        fam = next((f for f in FAMILIES if n.split("<")[0].split("::")[-1].split()[-1] == f or f"{len(f)}{f}I" in n), None)
        if fam is None:
            continue
        seen[fam] += 1
        assert r["name"] in declared, f"{n}: no kernel descriptor"
        assert 0 < r["lead"] <= BUDGET, f"{n}: {r['lead']} dwords of leading scalar parameters"
        assert declared[r["name"]] == r["lead"], f"{n}: declares {declared[r['name']]} dwords preloaded, its leading scalar parameters are {r['lead']}"
    for fam, k in seen.items():
        assert k > 0, f"no {fam} in the library"
