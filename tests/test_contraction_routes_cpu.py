"""CPU: the instantiation lists of the contraction kernels and the resolution of a launch request onto them (onnxstream_amd/csrc/osg_gemm_routes.h -- what the
launchers, the cost model, the tuner, the tune-table loader and the split-K fold sizing all read), through a g++-built driver (tests/cpp/contraction_routes.cpp)."""
import os
import subprocess
import sys
import tempfile
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_shipped_artifacts_cpu import _launchable, _rows  # noqa: E402  (the loader's rule, restated there)

TILES = [(128, 128), (128, 64), (64, 64), (64, 128), (128, 160), (128, 80), (64, 80), (64, 160)]
CONV, LN1, LN2, GEGLU, ROWSTATS, W8 = 1, 2, 4, 8, 16, 32      # form bits of the driver


@pytest.fixture(scope="module")
def routes():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "routes")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"),
                        os.path.join(REPO, "tests", "cpp", "contraction_routes.cpp"), "-o", exe], check=True)
        out = {m: subprocess.run([exe, m], stdout=subprocess.PIPE, text=True, check=True).stdout for m in ("entries", "rows", "resolve")}
    v2, v3 = [], []
    for line in out["entries"].splitlines():
        f = line.split()
        if f[0] == "v2":
            bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, tile, fold = map(int, f[1:])
            v2.append(dict(bm=bm, bn=bn, tile=tile, nst=nst, conv=conv, spec=spec, ln=ln, nch=nch, ks=ks, wgn=wgn, wq=wq, fold_capable=fold))
        else:
            w, bn, wgm, wgn, nlw, wq = map(int, f[1:])
            v3.append(dict(w=w, bn=bn, wgm=wgm, wgn=wgn, nlw=nlw, wq=wq))
    res, halo = {}, {}
    for line in out["resolve"].splitlines():
        f = line.split()
        if f[0] == "r":
            *key, entry, fold = map(int, f[1:])
            res[tuple(key)] = (entry, fold)
        else:
            w, bn, nl, w8, entry = map(int, f[1:])
            halo[(w, bn, nl, w8)] = entry
    return SimpleNamespace(v2=v2, v3=v3, rows=out["rows"].strip(), res=res, halo=halo)


def run(r, form, cfg, nst, ks=1, fold=0, spec=0, nch=5):
    """(the entry the request runs, or None; whether the split folds)"""
    entry, f = r.res[(form, nch if form & LN2 else 5, cfg, nst, ks, fold, spec)]
    return (r.v2[entry] if entry >= 0 else None), bool(f)


def at(r, form, cfg, nst, **kw):
    """(tile, nst, ks, spec, ln) of the entry a request runs"""
    e, _ = run(r, form, cfg, nst, **kw)
    return None if e is None else (e["tile"], e["nst"], e["ks"], e["spec"], e["ln"])


def test_the_row_rule_is_the_loaders(routes):
    want = "".join("1" if _launchable(fam, cfg, nst, s, bn) else "0" for fam in (0, 1) for cfg in range(64) for nst in range(9) for s in range(66)
                   for bn in (0, 64, 80, 96, 128, 160))
    assert routes.rows == want


def test_each_instantiation_is_listed_once(routes):
    assert len({tuple(e.values()) for e in routes.v2}) == len(routes.v2) and len({tuple(e.values()) for e in routes.v3}) == len(routes.v3)
    for e in routes.v2:
        assert e["tile"] >= 0 and e["wgn"] == (1 if e["tile"] in (4, 5, 6) else 2), e
        assert not e["wq"] or (e["ln"] == 0 and e["spec"] == 0 and e["ks"] == 1), e
        assert e["fold_capable"] == (e["ks"] == 1 and not e["spec"] and e["ln"] == 0 and e["tile"] not in (0, 4, 7)), e
    for e in routes.v3:
        assert (e["wgm"], e["wgn"]) == ((4, 1) if e["bn"] == 80 else (2, 2)) and (e["nlw"] == 4 or not e["wq"]), e


def test_every_request_names_an_entry_unless_no_kernel_takes_its_form(routes):
    for (form, nch, cfg, nst, ks, fold, spec), (entry, f) in routes.res.items():
        error_form = bool(form & (LN1 | LN2)) and bool(form & (W8 | CONV)) or (form & W8 and form & ROWSTATS)
        assert (entry < 0) == bool(error_form), (form, cfg, nst, ks, fold, spec)
        if entry < 0:
            continue
        e = routes.v2[entry]
        assert e["wq"] == bool(form & W8) and e["conv"] == bool(form & CONV) and e["ln"] == (2 if form & LN2 else 1 if form & LN1 else 0)
        assert e["nch"] == (nch if form & LN2 else 5)
        # the fold applies exactly where it is asked for with KS = 1 and the entry that runs can take it -- and then the route is sized with that entry's tile
        assert f == (fold == 1 and ks == 1 and e["fold_capable"] == 1), (form, cfg, nst, ks, fold, spec)


def test_f16_tiles_4_to_7(routes):
    r = routes
    for tile, back in ((4, 0), (5, 0), (6, 2), (7, 2)):
        assert at(r, LN1, tile, 4) == (back, 4, 1, 0, 1)                                 # LN = 1: the round-2 tiles only
        assert at(r, 0, tile, 8) == (back, 4, 1, 0, 0) and at(r, 0, tile, 3) == (back, 4, 1, 0, 0)
        assert at(r, 0, tile, 8, ks=2) == (back, 4, 1, 0, 0)                            # (the fall-back takes no KS = 2 ...)
        assert at(r, LN1, tile, 4, spec=1) == (back, 4, 1, 0, 1)                        # (... and no spec)
        assert at(r, 0, tile, 2) == (tile, 2, 1, 0, 0) and at(r, 0, tile, 4) == (tile, 4, 1, 0, 0)
        assert at(r, 0, tile, 4, ks=2) == (tile, 4, 1, 0, 0)
    for form in (GEGLU, ROWSTATS):
        assert at(r, form, 4, 4) == (4, 4, 1, 0, 0)
        assert at(r, form, 5, 4) == (0, 4, 1, 0, 0) and at(r, form, 6, 2) == (2, 2, 1, 0, 0) and at(r, form, 7, 4) == (2, 4, 1, 0, 0)
    assert [at(r, CONV, t, 4) for t in (4, 5, 6, 7)] == [(4, 4, 1, 0, 0), (5, 4, 1, 0, 0), (6, 4, 1, 0, 0), (2, 4, 1, 0, 0)]
    assert at(r, CONV, 5, 2) == (0, 2, 1, 0, 0) and at(r, CONV, 6, 6) == (2, 4, 1, 0, 0)
    assert at(r, CONV | LN2, 4, 4) is None                                              # (a convolution has no LayerNorm form)
    assert at(r, LN2, 4, 2) == (4, 2, 1, 0, 2) and at(r, LN2, 7, 4) == (7, 4, 1, 0, 2)
    assert at(r, LN2, 5, 4) == (0, 4, 1, 0, 2) and at(r, LN2, 6, 4) == (2, 4, 1, 0, 2)
    assert at(r, 0, 6, 6) == (6, 6, 1, 0, 0) and at(r, 0, 6, 8) == (2, 4, 1, 0, 0) and at(r, 0, 4, 6) == (0, 4, 1, 0, 0)
    # spec: tile 4, 4 stages, no convolution
    assert at(r, 0, 4, 4, spec=1) == (4, 4, 1, 1, 0) and at(r, LN2, 4, 4, spec=1, nch=10) == (4, 4, 1, 1, 2)
    assert at(r, 0, 4, 2, spec=1) == (4, 2, 1, 0, 0) and at(r, CONV, 4, 4, spec=1) == (4, 4, 1, 0, 0) and at(r, 0, 5, 4, spec=1) == (5, 4, 1, 0, 0)


def test_f16_tiles_0_to_3(routes):
    r = routes
    assert at(r, LN1, 3, 4) == (2, 4, 1, 0, 1) and at(r, LN2, 3, 6) == (2, 2, 1, 0, 2)   # LayerNorm on tile 3 runs 64 x 64
    # KS = 2: tile 1 with 2 stages, tile 2 with >= 4 -> 4 else 2; never with LN = 1
    assert [at(r, 0, 1, n, ks=2) for n in (2, 4, 6)] == [(1, 2, 2, 0, 0)] * 3
    assert [at(r, 0, 2, n, ks=2) for n in (2, 3, 4, 6, 8)] == [(2, 2, 2, 0, 0)] * 2 + [(2, 4, 2, 0, 0)] * 3
    assert at(r, CONV, 2, 4, ks=2) == (2, 4, 2, 0, 0) and at(r, LN2, 1, 4, ks=2) == (1, 2, 2, 0, 2)
    assert at(r, LN1, 2, 4, ks=2) == (2, 4, 1, 0, 1) and at(r, 0, 0, 4, ks=2) == (0, 4, 1, 0, 0) and at(r, 0, 3, 4, ks=2) == (3, 4, 1, 0, 0)
    # spec: tile 0, 4 stages, no convolution, not LN = 1
    assert at(r, 0, 0, 4, spec=1) == (0, 4, 1, 1, 0) and at(r, LN2, 0, 4, spec=1) == (0, 4, 1, 1, 2)
    assert at(r, LN1, 0, 4, spec=1) == (0, 4, 1, 0, 1) and at(r, CONV, 0, 4, spec=1) == (0, 4, 1, 0, 0)
    assert at(r, 0, 0, 2, spec=1) == (0, 2, 1, 0, 0) and at(r, 0, 1, 4, spec=1) == (1, 4, 1, 0, 0)
    # the LN forms: 4 stages -> 4, anything else -> 2; NCH 5 / 10 / 20 as the form says
    for form in (LN1, LN2, LN2 | GEGLU):
        for tile in (0, 1, 2):
            assert [at(r, form, tile, n)[1] for n in (0, 2, 3, 4, 6, 8)] == [2, 2, 2, 4, 2, 2]
    assert [run(r, LN2, 1, 4, nch=n)[0]["nch"] for n in (5, 10, 20)] == [5, 10, 20]
    # plain rings
    for form in (0, CONV, GEGLU, ROWSTATS):
        assert [at(r, form, 0, n)[1] for n in (2, 4, 6, 8, 0)] == [2, 4, 2, 2, 2]
        for tile in (1, 3):
            assert [at(r, form, tile, n)[1] for n in (2, 4, 6, 8, 5)] == [2, 4, 6, 2, 2]
        assert [at(r, form, 2, n)[1] for n in (2, 4, 6, 8, 5)] == [2, 4, 6, 8, 2]


def test_uint8_codes(routes):
    r = routes
    assert at(r, W8, 2, 4, ks=2) == (2, 4, 1, 0, 0) and at(r, W8, 0, 4, spec=1) == (0, 4, 1, 0, 0)   # KS and spec ignored
    assert at(r, W8, 2, 8) == (2, 8, 1, 0, 0) and at(r, W8, 6, 6) == (6, 6, 1, 0, 0)
    assert at(r, W8, 0, 6) == (0, 4, 1, 0, 0) and at(r, W8, 4, 6) == (0, 4, 1, 0, 0) and at(r, W8, 7, 8) == (2, 4, 1, 0, 0)
    assert at(r, W8 | CONV, 3, 2) == (2, 4, 1, 0, 0) and at(r, W8 | CONV, 7, 4) == (2, 4, 1, 0, 0) and at(r, W8 | CONV, 5, 2) == (0, 4, 1, 0, 0)
    assert at(r, W8 | CONV, 1, 2) == (1, 2, 1, 0, 0) and at(r, W8 | CONV, 6, 4) == (6, 4, 1, 0, 0)
    assert at(r, W8 | GEGLU, 4, 2) == (4, 2, 1, 0, 0) and [at(r, W8 | GEGLU, t, 2) for t in (5, 6, 7)] == [(0, 4, 1, 0, 0), (2, 4, 1, 0, 0), (2, 4, 1, 0, 0)]
    for form in (W8 | LN1, W8 | LN2, W8 | ROWSTATS):
        assert at(r, form, 0, 4) is None


def test_the_fold_is_sized_for_the_tile_that_runs(routes):
    """the cases where the launchers fell back to another tile after sizing the fold for the one asked for"""
    r = routes
    e, fold = run(r, CONV, 6, 2, fold=1)          # f16 convolution: no 64 x 80 tile with 2 stages -> 64 x 64
    assert (e["bm"], e["bn"], e["nst"], fold) == (64, 64, 2, True)
    e, fold = run(r, W8 | CONV, 6, 2, fold=1)     # uint8 codes: -> 64 x 64 with 4 stages
    assert (e["bm"], e["bn"], e["nst"], fold) == (64, 64, 4, True)
    e, fold = run(r, W8 | CONV, 5, 2, fold=1)     # -> 128 x 128: no fold there
    assert (e["bm"], e["bn"], fold) == (128, 128, False)
    assert run(r, 0, 6, 4, fold=1)[1] and not run(r, 0, 6, 4, ks=2, fold=1)[1] and not run(r, LN2, 6, 4, fold=1)[1] and not run(r, 0, 0, 4, fold=1)[1]


def test_halo_kernel(routes):
    h = lambda w, bn, nl, w8: None if routes.halo[(w, bn, nl, w8)] < 0 else routes.v3[routes.halo[(w, bn, nl, w8)]]
    for w in (64, 32, 16, 8):
        for bn in (0, 64, 96, 128):
            assert h(w, bn, 4, 0)["bn"] == 128 and h(w, bn, 4, 1)["bn"] == 128
        for nl in (0, 4, 8):
            assert h(w, 80, nl, 1)["nlw"] == 4 and h(w, 80, nl, 0)["nlw"] == (8 if nl == 8 else 4)
        assert h(w, 160, 8, 0)["nlw"] == (4 if w in (64, 8) else 8)        # (where the wider stages leave the ring too short: 4 loader waves)
        assert h(w, 160, 4, 1)["bn"] == (80 if w == 64 else 160)          # (uint8 codes, 64-pixel rows: the 80-column tile)
        assert all(e["wq"] == w8 for (ww, _, _, w8), i in routes.halo.items() if ww == w for e in [routes.v3[i]])
    assert h(12, 128, 4, 0) is None


def test_every_shipped_tune_row_resolves_with_the_form_its_key_encodes(routes):
    tile3_ln = 0
    for ln, v, _ in _rows():
        kind, K, W, flags = v[0], v[4], v[7], v[12]
        family, cfg, nst, splits, bn = v[13:18]
        w8 = 1 if flags & 1024 else 0
        if family == 1:
            assert routes.halo[(W, bn, nst, w8)] >= 0, f"line {ln}"
            continue
        form = (CONV if kind != 0 else 0) | (W8 if w8 else 0) | (GEGLU if (flags & 15) == 3 else 0) | (ROWSTATS if flags & 512 else 0)
        if flags & 128:
            form |= LN2 if flags & 256 else LN1
        nch = (5 if K // 64 <= 5 else 10 if K // 64 <= 10 else 20)
        e, fold = run(routes, form, cfg & 7, nst, ks=2 if cfg & 8 else 1, fold=(cfg >> 4) & 1, spec=(cfg >> 5) & 1, nch=nch)
        assert e is not None, f"line {ln}: no kernel takes the row"
        assert fold == bool(cfg & 16), f"line {ln}: a folded row whose entry cannot fold"
        if form & (LN1 | LN2) and cfg & 7 == 3:
            assert (e["bm"], e["bn"]) == (64, 64), f"line {ln}"
            tile3_ln += 1
    assert tile3_ln >= 1      # (rows the tuner stored for LayerNorm shapes on tile 3: they have always run the 64 x 64 tile)
