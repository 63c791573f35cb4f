"""tests/tuned_rows.py on the host: every row of the shipped tune table decodes to a call, resolves under its own form and is legal for it; the structured
references of the large rows equal the brute-force float64 reference; and the comparison the device test makes would catch a dropped k-tile -- a numpy
emulation of the declared arithmetic passes it, the same emulation with one k-tile missing, or with the remainder slice one tile short, fails it."""
import os
import re

import numpy as np
import pytest

import test_contraction_instantiations as ci
import tuned_rows as tr

ROWS = tr.rows()
BY_LINE = {r.line: r for r in ROWS}


def test_the_table_has_250_rows_in_the_groups_the_device_test_runs():
    assert len(ROWS) == 250
    covered = sorted(r.line for g in tr.GROUPS for r in tr.group_rows(g))
    assert covered == [r.line for r in ROWS], "the groups of tuned_rows.GROUPS do not cover every table line exactly once"
    text = open(os.path.join(ci.REPO, "onnxstream_amd", "csrc", "osg_common.h")).read()
    assert int(re.search(r"kTickets = 1 << (\d+)", text).group(1)) == tr.K_TICKETS.bit_length() - 1


@pytest.mark.parametrize("r", ROWS, ids=[r.id for r in ROWS])
def test_row_decodes_resolves_and_is_legal_for_its_form(r):
    r.check_decodes()
    e = tr.check_legal(r)
    assert e.route[1] >= 0 and e.route[2] >= 1 and e.workgroups >= 1
    # the split as written runs as written: no slice of a shipped row is empty
    assert e.route[2] == r.splits, f"table line {r.line}: {r.splits} k-slices asked, {e.route[2]} run"


def test_the_regime_the_table_launches():
    """what the issue counts: the launches the instantiation module never reaches are in the table (a changed table moves these figures knowingly)"""
    e = {r.line: tr.expected_route(r) for r in ROWS}
    v2 = [r for r in ROWS if r.family == 0]
    assert sum(1 for r in v2 if e[r.line].workgroups > 256) >= 80
    assert max(e[r.line].workgroups for r in ROWS) >= 32768
    assert max(r.K for r in ROWS) == 23040
    assert sum(1 for r in ROWS if r.fold) >= 16
    assert sum(1 for r in ROWS if r.family == 1) >= 70
    assert sum(1 for r in ROWS if r.rows * r.K * 8 > tr.LIMIT) >= 30      # rows that need the structured reference


# ---- structured reference == brute force ---------------------------------------------------------------------------------------------------------------
def synthetic(line, **kw):
    base = dict(line=line, kind=0, device=0, M=1, N=1, K=64, batch=1, H=0, W=0, Cin=0, KW=0, sh=0, sw=0, flags=0, family=0, cfg=2, nst=4, splits=1, bn=0)
    base.update(kw)
    if base["kind"] == 0:
        base["H"] = base["K"]
    return tr.Row(**base)


STRUCTURED = [
    # GEMM: 5 periods of 131 rows and a bit, 3 k-slices (markers in each), bias + residual; SiLU with an f32 bias; GEGLU; uint8 codes with vectors; a batch
    synthetic(901, M=700, N=48, K=576, flags=16, splits=3),
    synthetic(902, M=4500, N=24, K=320, flags=64 | 1, splits=1),
    synthetic(903, M=600, N=64, K=256, flags=3),
    synthetic(905, M=650, N=40, K=256, flags=1024 | 16, splits=2),
    synthetic(904, M=300, N=20, K=128, batch=3),
    # convolutions 3 x 3: several periods in h and w, every border, 2 images, per-image bias + residual; stride 2 (odd and even sizes); uint8 codes; 5 x 5
    synthetic(911, kind=1, M=2 * 32 * 32, N=24, K=9 * 64, H=32, W=32, Cin=64, KW=3, sh=1, sw=1, flags=32 | 16, family=1, cfg=0, nst=4, splits=1, bn=80),
    synthetic(912, kind=2, M=2 * 19 * 21, N=20, K=9 * 64, H=37, W=41, Cin=64, KW=3, sh=2, sw=2, flags=1),
    synthetic(913, kind=2, M=1 * 20 * 20, N=20, K=9 * 64, H=40, W=40, Cin=64, KW=3, sh=2, sw=2, flags=64),
    synthetic(915, kind=2, M=1 * 70 * 70, N=12, K=9 * 64, H=70, W=70, Cin=64, KW=3, sh=1, sw=1, flags=1024 | 32),
    synthetic(914, kind=2, M=1 * 23 * 23, N=8, K=25 * 64, H=23, W=23, Cin=64, KW=5, sh=1, sw=1, flags=0),
]


@pytest.mark.parametrize("r", STRUCTURED, ids=[r.id for r in STRUCTURED])
def test_structured_reference_equals_brute_force(r):
    """the same operands through both references: want and the bound (hence S) agree to 1e-12 relative; the markers tell rows apart"""
    if r.conv:
        assert r.M == r.images * r.Ho * r.Wo, (r.Ho, r.Wo)
    s = tr.Case(r, structured=True)
    b = tr.Case(r, structured=True)
    b.structured = False                                      # the same operand arrays, the brute-force products
    if r.conv:
        assert s.x.shape[1] > 2 * s.Ph and s.x.shape[2] > 2 * s.Pw, "several periods"
        assert not np.array_equal(s.x[0, :s.Ph], s.x[0, s.Ph:2 * s.Ph]), "the markers break the period"
    else:
        assert r.rows >= 2 * s.P and len({c for c, _ in s.mcols}) >= 3
        assert len(np.unique(s.a[:min(r.rows, 4096)], axis=0)) == min(r.rows, 4096), "two of 4096 consecutive rows are equal"
        per = -(-s.route.ktiles // s.route.route[2]) * 64
        assert len({c // per for c, _ in s.mcols}) == s.route.route[2] or s.route.route[2] > 3, "a k-slice without a marker column"
    for (r0, r1, n0, n1) in [(0, r.rows, 0, r.N), (r.rows // 3, r.rows // 3 + 57, 0, r.N)]:
        ws, es, *_ = s.reference(r0, r1, n0, n1)
        wb, eb, *_ = b.reference(r0, r1, n0, n1)
        scale = np.abs(wb).max()
        assert np.abs(ws - wb).max() <= 1e-12 * scale, np.abs(ws - wb).max() / scale
        assert np.abs(es - eb).max() <= 1e-12 * np.abs(eb).max()


def test_column_chunks_of_a_wide_weight_cover_the_output(monkeypatch):
    """the reference of a very wide weight is formed in column chunks: shrink CHUNK and compare with one block"""
    r = synthetic(921, M=70, N=200, K=128, flags=16 | 1)
    c = tr.Case(r)
    whole, _, _, _ = c.reference(0, r.rows, 0, r.N)
    monkeypatch.setattr(tr, "CHUNK", 128 * 40)
    blocks = c.chunks()
    assert len({(n0, n1) for _, _, n0, n1 in blocks}) > 1 and len({(r0, r1) for r0, r1, _, _ in blocks}) > 1
    got = np.full(whole.shape, np.nan)
    for r0, r1, n0, n1 in blocks:
        got[r0:r1, n0:n1] = c.reference(r0, r1, n0, n1)[0]
    assert np.array_equal(got, whole)


# ---- the comparison catches what it is for ---------------------------------------------------------------------------------------------------------------
# reduced copies of table rows (same form, K and choice; fewer rows and columns): a GEMM in 4 slices of 80 k-tiles, a GEGLU row with the LayerNorm folded in, the halo kernel with 10 slabs in
# 4 slices (3, 3, 3, 1) and with 40 slabs in 8, the stride-2 convolution with 180 k-tiles in 12 slices, a uint8 row with per-column vectors, a structured row
EMULATED = [(30, dict(M=96, N=64)), (17, dict(M=64, N=128)), (22, dict(hw=16, images=1, N=40)), (231, dict(hw=8, images=3, N=32)),
            (33, dict(hw=16, images=1, N=32)), (221, dict(M=80, N=48)), (110, dict(M=64, N=40))]


@pytest.mark.parametrize("line,size", EMULATED, ids=[f"L{n:03d}" for n, _ in EMULATED])
def test_emulated_arithmetic_passes_and_a_dropped_k_tile_fails(line, size):
    r = tr.reduced(BY_LINE[line], **size)
    r.check_decodes() if not r.conv else None
    c = tr.Case(r)
    units = c.route.ktiles * (9 if r.family == 1 else 1)
    worst, far = c.compare(c.emulate())
    assert worst <= 1.0 and far <= ci.FAR
    # one k-tile out of up to 360 missing: test_fullsize's 2.4e-3 of the output's maximum does not see it, the per-element bound does
    for kw in (dict(drop_tile=units // 2), dict(short_last=True)):
        bad = c.emulate(**kw)
        with pytest.raises(AssertionError, match="outside the bound"):
            c.compare(bad)


def test_emulated_structured_row_passes_and_a_dropped_k_tile_fails():
    """the structured operands through the same comparison (a reduced copy of the 1024 x 1024 decoder's widest convolution and of its attention projection)"""
    for line, size in ((138, dict(hw=24, images=1, N=32)), (136, dict(M=300, N=32))):
        r = tr.reduced(BY_LINE[line], **size)
        c = tr.Case(r, structured=True)
        c.compare(c.emulate())
        with pytest.raises(AssertionError, match="outside the bound"):
            c.compare(c.emulate(drop_tile=1))
