"""CPU: which epilogue variant a gemm2_kernel launch runs (onnxstream_amd/csrc/osg_gemm_epi.h select_epi), through a g++-built stand-alone driver
(tests/cpp/epilogue_select.cpp) compiled with -fsanitize=address,undefined.

For every lean instantiation of kLeanEntries: a launch that meets its conditions gets it; a launch with any one condition broken -- M one row short of a tile
multiple, N four columns short, an output pitch or an operand of 4-byte alignment, a feature outside the mask, OSG_EPI_GENERIC=1 -- does not; and over every
entry x every form, no lean instantiation is ever selected for a form other than the one it is compiled for."""
import itertools
import os
import subprocess
import tempfile
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("entry", "M", "N", "batch", "splits", "fold", "bias", "bias_f32", "rowbias", "residual", "c2", "rowstats", "sinks", "act", "other", "ldc", "ldc2", "rb_ld",
          "rs_np", "align_or", "force")
BIT_NAMES = ("BIAS16", "BIAS32", "ROWBIAS", "RESIDUAL", "SILU", "C2", "ROWSTATS", "SPLIT", "FOLD", "GEGLU", "SINKS", "OTHER")


@pytest.fixture(scope="module")
def epi():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "epilogue_select")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "onnxstream_amd", "csrc"), os.path.join(REPO, "tests", "cpp", "epilogue_select.cpp"), "-o", exe], check=True)
        listing = subprocess.run([exe, "list"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert listing.returncode == 0 and not listing.stderr, listing.stderr

        def select(launches):
            text = "".join(" ".join(str(int(l[f])) for f in FIELDS) + "\n" for l in launches)
            r = subprocess.run([exe, "select"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0 and not r.stderr, r.stderr          # (a sanitizer report goes to stderr and ends the program)
            rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
            assert len(rows) == len(launches)
            return rows

        bits, lean, v2 = {}, [], []
        for line in listing.stdout.splitlines():
            f = line.split()
            if f[0] == "bits":
                bits = dict(zip(BIT_NAMES, map(int, f[1:13])))
                bits["ANY"] = int(f[14])
            elif f[0] == "lean":
                i, entry, bm, bn, nst, conv, spec, ln, nch, ks, wgn, wq, mask = map(int, f[1:])
                assert i == len(lean)
                lean.append(SimpleNamespace(i=i, entry=entry, bm=bm, bn=bn, ln=ln, wgn=wgn, ks=ks, mask=mask))
            elif f[0] == "v2":
                i, bm, bn, ln, wgn, ks = map(int, f[1:])
                v2.append(SimpleNamespace(i=i, bm=bm, bn=bn, ln=ln, wgn=wgn, ks=ks))
        yield SimpleNamespace(bits=bits, lean=lean, v2=v2, select=select)


def launch_of(B, entry, bm, bn, mask, tiles=2):
    """a launch of `entry` whose form is exactly `mask`, on whole tiles with aligned rows"""
    M, N = tiles * bm, tiles * bn
    split = bool(mask & B["SPLIT"])
    return dict(entry=entry, M=M, N=N, batch=1, splits=2 if split else 1, fold=0,
                bias=bool(mask & (B["BIAS16"] | B["BIAS32"])) or split, bias_f32=bool(mask & B["BIAS32"]), rowbias=bool(mask & B["ROWBIAS"]),
                residual=bool(mask & B["RESIDUAL"]), c2=bool(mask & B["C2"]), rowstats=bool(mask & B["ROWSTATS"]), sinks=0,
                act=1 if mask & B["SILU"] else 3 if mask & B["GEGLU"] else 0, other=0,
                ldc=0, ldc2=N + 64 if mask & B["C2"] else 0, rb_ld=N if mask & B["ROWBIAS"] else 0, rs_np=N // 32 if mask & B["ROWSTATS"] else 0, align_or=0x7f0000001000 | 8, force=0)


def form_of(B, l):
    """epi_form, restated"""
    if l["other"] or l["batch"] != 1:
        return B["OTHER"]
    if l["splits"] > 1 and not l["fold"]:
        return B["SPLIT"]
    m = B["FOLD"] if l["splits"] > 1 else 0
    if l["bias"]:
        m |= B["BIAS32"] if l["bias_f32"] else B["BIAS16"]
    for f, b in (("rowbias", "ROWBIAS"), ("residual", "RESIDUAL"), ("c2", "C2"), ("rowstats", "ROWSTATS"), ("sinks", "SINKS")):
        if l[f]:
            m |= B[b]
    m |= {0: 0, 1: B["SILU"], 3: B["GEGLU"]}.get(l["act"], B["OTHER"])
    return m


def test_the_list_is_well_formed(epi):
    B = epi.bits
    lean_bits = B["BIAS16"] | B["BIAS32"] | B["ROWBIAS"] | B["RESIDUAL"] | B["SILU"] | B["C2"] | B["ROWSTATS"] | B["SPLIT"] | B["GEGLU"]
    assert 0 < len(epi.lean) <= 40
    assert len({(x.entry, x.mask) for x in epi.lean}) == len(epi.lean)
    for x in epi.lean:
        assert 0 <= x.entry < len(epi.v2) and x.mask != B["ANY"] and not (x.mask & ~lean_bits), vars(x)
        assert not (x.mask & B["BIAS16"] and x.mask & B["BIAS32"])
        assert not (x.mask & B["SPLIT"]) or x.mask == B["SPLIT"]
        assert x.ln == 0 or x.mask & B["BIAS32"]                 # (a folded LayerNorm always adds its f32 c2)
        assert not (x.mask & (B["ROWSTATS"] | B["GEGLU"])) or (x.bn // x.wgn) % 32 == 0
        assert not (x.mask & B["GEGLU"]) or not (x.mask & ~(B["GEGLU"] | B["BIAS16"] | B["BIAS32"]))


def test_each_lean_instantiation_is_selected_for_its_own_launch_only(epi):
    B = epi.bits
    for x in epi.lean:
        good = launch_of(B, x.entry, x.bm, x.bn, x.mask)
        one_tile = launch_of(B, x.entry, x.bm, x.bn, x.mask, tiles=1)
        broken = {
            "M one row short": dict(good, M=good["M"] - 1),
            "M 16 rows over": dict(good, M=x.bm + 16),
            "N four columns short": dict(good, N=good["N"] - 4, rs_np=(good["N"] - 4) // 32 if good["rowstats"] else 0),
            "output pitch of 4-byte alignment": dict(good, ldc=good["N"] + 2),
            "an operand of 4-byte alignment": dict(good, align_or=good["align_or"] | 4),
            "OSG_EPI_GENERIC=1": dict(good, force=1),
            "a batch": dict(good, batch=2),
            "operand prefetch switched off": dict(good, other=1),
            "statistics sinks": dict(good, sinks=1),
            "sigmoid": dict(good, act=2),
            "fold": dict(good, splits=2, fold=1),
        }
        if good["c2"]:
            broken["second pitch of 4-byte alignment"] = dict(good, ldc2=good["ldc2"] + 2)
        if good["rowbias"]:
            broken["per-image bias pitch of 4-byte alignment"] = dict(good, rb_ld=good["rb_ld"] + 2)
        if good["rowstats"]:
            broken["a row-statistics slot short"] = dict(good, rs_np=good["rs_np"] - 1)
        if x.mask & B["SPLIT"]:
            for k in ("statistics sinks", "sigmoid"):   # (a k-slice stores its slab whatever the reduce launch adds: still this variant)
                del broken[k]
        names = list(broken)
        got = epi.select([good, one_tile] + [broken[k] for k in names])
        assert got[0] == (x.i, x.mask, 1), (vars(x), got[0])
        assert got[1] == (x.i, x.mask, 1), (vars(x), got[1])
        for k, g in zip(names, got[2:]):
            assert g[0] == -1, (vars(x), k, g)
        # a feature outside the mask: never this variant; another one only if that one is compiled for exactly the new form
        if not x.mask & B["SPLIT"]:
            extra = []
            for f in ("rowbias", "residual", "c2", "rowstats"):
                if not good[f]:
                    extra.append(dict(good, **{f: 1}, ldc2=good["N"], rb_ld=good["N"], rs_np=good["N"] // 32))
            extra += [dict(good, act=a) for a in (0, 1, 3) if a != good["act"]]
            extra.append(dict(good, bias=1, bias_f32=0 if good["bias_f32"] else 1))
            extra.append(dict(good, bias=0 if good["bias"] else 1))
            extra.append(dict(good, splits=2))
            for l, g in zip(extra, epi.select(extra)):
                assert g[0] != x.i, (vars(x), l)
                assert g[1] == form_of(B, l)
                if g[0] >= 0:
                    assert epi.lean[g[0]].entry == x.entry and epi.lean[g[0]].mask == g[1], (vars(x), l, g)


def test_no_lean_mask_is_selected_for_a_form_it_does_not_hold(epi):
    """every entry of kV2Entries x every form: a selected variant is compiled for that entry and exactly that form, and every (entry, form) the list holds is found"""
    B = epi.bits
    launches = []
    for e in epi.v2:
        for bias, rowbias, residual, c2, rowstats, sinks, act, split in itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2, 3), (0, 1, 2)):
            N = 2 * e.bn
            launches.append(dict(entry=e.i, M=2 * e.bm, N=N, batch=1, splits=1 if split == 0 else 2, fold=split == 2, bias=bias != 0, bias_f32=bias == 2, rowbias=rowbias,
                                 residual=residual, c2=c2, rowstats=rowstats, sinks=sinks, act=act, other=0, ldc=0, ldc2=N if c2 else 0, rb_ld=N, rs_np=N // 32, align_or=16, force=0))
    launches += [dict(launches[0], entry=-1), dict(launches[0], entry=len(epi.v2))]
    got = epi.select(launches)
    held = {(x.entry, x.mask): x.i for x in epi.lean}
    found = set()
    for l, g in zip(launches, got):
        form = form_of(B, l)
        assert g[1] == form, (l, g)
        want = held.get((l["entry"], form), -1)
        if want >= 0 and form & B["ROWSTATS"] and l["N"] % 32:
            want = -1
        assert g[0] == want, (l, g, want)
        if g[0] >= 0:
            found.add(g[0])
    assert found == set(range(len(epi.lean)))
