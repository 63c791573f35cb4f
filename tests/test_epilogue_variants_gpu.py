"""-m gpu: every lean epilogue variant of gemm2_kernel (kLeanEntries, onnxstream_amd/csrc/osg_gemm_epi.h) on the smallest shapes at which it can go wrong.

Per variant, with the form's own operands (f16 or f32 bias, per-image bias, residual, SiLU or GEGLU, second destination, row statistics out, handed-over LayerNorm slots),
every output between guard bands:
  * one tile: M = BM, N = BN, K = 64 (NST + 1) -- the ring wraps once;
  * a 2 x 2 tile grid: M = 2 BM, N = 2 BN;
  * rows per image = BM / 2 wherever the launch goes through a convolution entry point: with a per-image bias one tile spans two images;
  * the fallback: M = BM + 16 (through a convolution entry point: images of 16 rows) must run the entry's EPI_ANY instantiation and be correct.
Every element is compared bit for bit with the same launch under OSG_EPI_GENERIC=1 and against float64 with the bounds and the ulp rule of
tests/test_contraction_instantiations.py (imported).  osg_last_epilogue must name the variant (or -1 where EPI_ANY has to run).

K where 64 (NST + 1) cannot reach the entry: an implicit-GEMM convolution has K = 9 Cin, Cin % 64 == 0 -- Cin = 64, 9 k-tiles (>= NST + 1 for every ring);
a handed-over LayerNorm entry is chosen by its chunk count -- K = 320 / 576 / 1216 for NCH = 5 / 10 / 20, as in test_contraction_instantiations; a split slab
variant runs two k-slices of NST + 1 k-tiles each.
"""
import os
import subprocess
import tempfile
from functools import lru_cache

import numpy as np
import pytest

import test_contraction_instantiations as ci
from test_contraction_instantiations import (ACT_GEGLU, ACT_NONE, ACT_SILU, GEMM2, K_LN2, OSG_F16, Out, act_apply, bias_dtype, check, check_rowstats, contraction, dev, f16,
                                             f32, f64, geglu_logical, im2col, knobs, ln_reference, ptr, rnd)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIT_NAMES = ("BIAS16", "BIAS32", "ROWBIAS", "RESIDUAL", "SILU", "C2", "ROWSTATS", "SPLIT", "FOLD", "GEGLU")
RAN = set()


@lru_cache(maxsize=None)
def lean_table():
    """(bits, [lean entries]) from tests/cpp/epilogue_select.cpp"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "epilogue_select")
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"), os.path.join(REPO, "tests", "cpp", "epilogue_select.cpp"), "-o", exe],
                       check=True)
        out = subprocess.run([exe, "list"], stdout=subprocess.PIPE, text=True, check=True).stdout
    bits, lean = {}, []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "bits":
            bits = dict(zip(BIT_NAMES, map(int, f[1:11])))
        elif f[0] == "lean":
            i, entry, bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, mask = map(int, f[1:])
            lean.append(dict(i=i, entry=entry, bm=bm, bn=bn, nst=nst, conv=conv, spec=spec, ln=ln, nch=nch, ks=ks, wgn=wgn, wq=wq, mask=mask))
    return bits, lean


def lean_id(x):
    bits, _ = lean_table()
    return ci.v2_id(x) + "-" + ("+".join(n.lower() for n in BIT_NAMES if x["mask"] & bits[n]) or "plain")


def lean_params():
    return [pytest.param(x["i"], id=lean_id(x)) for x in lean_table()[1]]


def activated(pre, E, act):
    if act == ACT_GEGLU:
        return act_apply(geglu_logical(pre), geglu_logical(E), act)
    return act_apply(pre, E, act)


def run_form(gpu, x, M, N, seed, rpi=None):
    """one launch of the variant's entry with exactly its form at M x N; returns ({name: output array}, (want, E) float64, osg_last_route, osg_last_epilogue)"""
    B, _ = lean_table()
    mask, bm = x["mask"], x["bm"]
    rng = np.random.default_rng(seed)
    has = {n: bool(mask & B[n]) for n in BIT_NAMES}
    split = has["SPLIT"]
    act = ACT_SILU if has["SILU"] else ACT_GEGLU if has["GEGLU"] else ACT_NONE
    bias_t = f32 if has["BIAS32"] else f16
    with_bias = has["BIAS16"] or has["BIAS32"] or split        # (a k-slice's form ignores the operands: the reduce launch adds them)
    rpi = rpi or bm // 2                                       # rows per image of the convolution entry points
    outs = {}
    if x["ln"]:
        assert not (has["ROWBIAS"] or has["C2"] or has["ROWSTATS"] or split), "osg_gemm_ln reaches no such form"
        K = K_LN2[x["nch"]] if x["ln"] == 2 else 64 * (x["nst"] + 1)
        xs, w = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5)
        gamma, beta, bias = (1.0 + rnd(rng, (K,), 0.1, f32)).astype(f16), rnd(rng, (K,), 0.1), rnd(rng, (N,), 0.1)
        res = rnd(rng, (M, N)) if has["RESIDUAL"] else None
        got, route, (wf, c1, c2) = ci.gemm_ln(gpu, xs, w, gamma, beta, bias, res, act, x["ln"] == 2)
        outs["y"] = got
        want = activated(*ln_reference(xs, wf, c1, c2, 1e-5, res), act)
        return outs, want, route, gpu.last_epilogue()
    if x["conv"]:
        K, cin = 9 * 64, 64
    else:
        K = 64 * (x["nst"] + 1) * (2 if split else 1)
        cin = K
    bias = rnd(rng, (N,), 0.1, bias_t) if with_bias else None
    res = rnd(rng, (M, N)) if has["RESIDUAL"] or split else None
    through_conv = x["conv"] or has["ROWBIAS"] or has["C2"]
    if not through_conv:
        a, w = rnd(rng, (M, K)), rnd(rng, (N, K), K ** -0.5)
        if has["ROWSTATS"]:
            got, rs, route = ci.gemm_rowstats(gpu, a, w, bias, res, act)
            outs["rowstats"] = rs
        else:
            got, route = ci.gemm(gpu, a, w, bias, res, act)
        outs["y"] = got
        return outs, activated(*contraction(a, w, bias, res), act), route, gpu.last_epilogue()
    assert not (has["ROWSTATS"] or has["GEGLU"]), "no convolution entry point emits row statistics or takes GEGLU"
    assert M % rpi == 0
    imgs, ho, wo = M // rpi, rpi // 8, 8
    if x["conv"]:
        xin, w = rnd(rng, (imgs, 2 * ho, 2 * wo, cin)), rnd(rng, (N, 3, 3, cin), K ** -0.5)
        geo = (imgs, 2 * ho, 2 * wo, cin, N, 3, 3, 2, 2, 1, 1, 1, 1, act)
        a = im2col(xin.astype(f64), 3, 2, 1)[0]
    else:
        xin, w = rnd(rng, (imgs, ho, wo, cin)), rnd(rng, (N, 1, 1, cin), K ** -0.5)
        geo = (imgs, ho, wo, cin, N, 1, 1, 1, 1, 0, 0, 0, 0, act)
        a = xin.reshape(M, K)
    ib = rnd(rng, (imgs, N), 0.5) if has["ROWBIAS"] else None
    out = Out(gpu, M, N)
    out2 = Out(gpu, M, N, ld=N + 24, col=12) if has["C2"] else None          # (the second destination as a column view: the gap must stay untouched)
    dx, dw, db, dr, di = keep = dev(gpu, xin, w, bias, res, ib)
    gpu._ck(gpu.lib.osg_conv2d_nhwc_v(gpu.ctx, OSG_F16, dx.ptr, dw.ptr, ptr(db), bias_dtype(bias), ptr(di), N if ib is not None else 0, ptr(dr), out.ptr, 0,
                                      out2.ptr if out2 else None, N + 24 if out2 else 0, *geo))
    route, epi = gpu.last_route(), gpu.last_epilogue()
    outs["y"] = out.read()
    if out2:
        outs["y2"] = out2.read()
    del keep
    rowbias = np.repeat(ib, rpi, axis=0) if ib is not None else None
    return outs, act_apply(*contraction(a, w.reshape(N, K), bias, res, rowbias), act), route, epi


def run_pair(gpu, monkeypatch, x, M, N, seed, want_lean, rpi=None):
    """the launch as selected and under OSG_EPI_GENERIC=1: bit-equal, correct against float64, the variants reported"""
    _, _, req = ci.table()
    B, _ = lean_table()
    cfg, nst, ks, spec = req[x["entry"]]
    split = bool(x["mask"] & B["SPLIT"])
    knobs(monkeypatch, OSG_GEMM_CFG=cfg, OSG_GEMM_NST=nst, OSG_GEMM_KS=ks, OSG_GEMM_SPEC=spec, OSG_GEMM_SPLITS=2 if split else 1, OSG_GEMM_FOLD=0)
    monkeypatch.delenv("OSG_EPI_GENERIC", raising=False)
    outs, (want, E), route, epi = run_form(gpu, x, M, N, seed, rpi)
    monkeypatch.setenv("OSG_EPI_GENERIC", "1")
    outs_g, _, route_g, epi_g = run_form(gpu, x, M, N, seed, rpi)
    monkeypatch.delenv("OSG_EPI_GENERIC", raising=False)
    what = f"{lean_id(x)} at {M} x {N}"
    assert route[:2] == (GEMM2, x["entry"]) and route[2] == (2 if split else 1) and route == route_g, (what, route, route_g)
    assert epi_g == (-1, -1), (what, epi_g)
    assert epi == ((x["i"], x["mask"]) if want_lean else (-1, -1)), (what, epi)
    assert outs.keys() == outs_g.keys()
    for k in outs:
        assert np.array_equal(outs[k].view(np.uint8), outs_g[k].view(np.uint8)), f"{what}: {k} differs from the OSG_EPI_GENERIC=1 launch"
    check(outs["y"], want, E, what)
    if "y2" in outs:
        assert np.array_equal(outs["y2"].view(np.uint16), outs["y"].view(np.uint16)), f"{what}: the second destination differs from the first"
    if "rowstats" in outs:
        check_rowstats(outs["y"], outs["rowstats"], what)


@pytest.mark.parametrize("i", lean_params())
def test_lean_variant(gpu, i, monkeypatch):
    x = lean_table()[1][i]
    bm, bn = x["bm"], x["bn"]
    run_pair(gpu, monkeypatch, x, bm, bn, 1000 + i, True)              # one tile
    run_pair(gpu, monkeypatch, x, 2 * bm, 2 * bn, 2000 + i, True)      # 2 x 2 tiles
    RAN.add(i)


@pytest.mark.parametrize("i", lean_params())
def test_ragged_rows_fall_back_to_the_generic_epilogue(gpu, i, monkeypatch):
    x = lean_table()[1][i]
    run_pair(gpu, monkeypatch, x, x["bm"] + 16, x["bn"], 3000 + i, False, rpi=16)     # (through a convolution entry point: images of 16 rows)


def test_every_lean_variant_ran(gpu, monkeypatch):
    """names any lean instantiation that no case above ran (run on its own, it runs the one-tile case of each itself)"""
    _, lean = lean_table()
    missing = []
    for x in lean:
        if x["i"] in RAN:
            continue
        try:
            run_pair(gpu, monkeypatch, x, x["bm"], x["bn"], 1000 + x["i"], True)
        except AssertionError as err:
            missing.append(f"{lean_id(x)}: {str(err)[:200]}")
    assert not missing, "lean instantiations no case ran: " + "; ".join(missing)
