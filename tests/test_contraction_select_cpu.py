"""CPU: what a contraction launch requests (onnxstream_amd/csrc/osg_gemm_select.h -- the cost models, the deterministic default plan, the candidates of a
measured choice, the split rule, the halo kernel's shape gate, the tune-table key), through a g++-built driver (tests/cpp/contraction_select.cpp).

* Golden (tests/golden/contraction_select.txt): for 256 CUs, every distinct key of the shipped tune table and the EXTRA shapes, each with its default
  (autotune off) and the ordered candidate list of a measured choice -- whole for the EXTRA shapes with short lists, as number, digest and head for the table's (summary()).
  Recorded when the functions moved into the header, text unchanged; any edit of the header must reproduce it byte for byte.
* split_slices against slices() of test_contraction_instantiations.py, tune_key against the call tuned_rows.py derives from each table row, halo3_takes
  against the halo predicate of Row.check_decodes: comparisons with the Python that already restates them.
"""
import atexit
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
from functools import lru_cache

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import tuned_rows as tr  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "contraction_select.txt")
GEGLU, F32BIAS, LN, RS_IN, RS_OUT, W8 = 3, 64, 128, 256, 512, 1024


def gemm_key(M, N, K, flags=0):
    return (0, 0, M, N, K, 1, K, 0, 0, 0, 0, 0, flags)


def halo_key(hw, cin, cout=320, flags=0):
    return (1, 0, hw * hw, cout, 9 * cin, 1, hw, hw, cin, 3, 1, 1, flags)


# where the quirks of the default bite: the forms that cannot split at M = 64 with K = 1280 / 2560 (the f16 rule ranks them WITH splits, then clamps), the same
# with uint8 codes where a kernel takes the form (GEGLU), N no multiple of 80, one k-tile, the halo kernel with one slab (no split) and with 20
EXTRA = [gemm_key(64, 640, K, GEGLU) for K in (1280, 2560)] + [gemm_key(64, 320, K, LN | F32BIAS) for K in (1280, 2560)] + \
        [gemm_key(64, 320, 1280, LN | RS_IN | F32BIAS)] + [gemm_key(64, 320, K, RS_OUT) for K in (1280, 2560)] + \
        [gemm_key(64, 640, K, W8 | GEGLU) for K in (1280, 2560)] + [gemm_key(64, 320, 2560, W8)] + \
        [gemm_key(64, 200, 1280), gemm_key(4096, 328, 320), gemm_key(64, 320, 64), gemm_key(4096, 320, 64)] + \
        [halo_key(hw, cin) for hw in (8, 16, 32, 64) for cin in (64, 1280)] + [halo_key(8, 1280, flags=W8)]


def golden_keys():
    keys = []
    for r in tr.rows():
        k = (r.kind, r.device, r.M, r.N, r.K, r.batch, r.H, r.W, r.Cin, r.KW, r.sh, r.sw, r.flags)
        if k not in keys:
            keys.append(k)
    return keys + [k for k in EXTRA if k not in keys]


@lru_cache(maxsize=None)
def driver():
    d = tempfile.mkdtemp(prefix="osg_select_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "select")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "onnxstream_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "contraction_select.cpp"), "-o", exe], check=True)
    return exe


def run(*args, lines=None):
    """the driver's output in a mode; lines: the rows of its input file"""
    with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
        if lines is not None:
            f.write("".join(" ".join(map(str, x)) + "\n" for x in lines))
            f.flush()
            args = args + (f.name,)
        return subprocess.run([driver(), *args], stdout=subprocess.PIPE, text=True, check=True).stdout


def plan(num_cu, keys):
    return run("plan", str(num_cu), lines=keys)


def parse_plan(text):
    """[{key, model: (family, cfg, nst, splits, bn), route: (family, instantiation, k-slices), cands: [(family, cfg, nst, splits, bn)]}]"""
    out = []
    for line in text.splitlines():
        tag, *f = line.split()
        if tag == "key":
            out.append(dict(key=tuple(map(int, f)), cands=[]))
        elif tag == "c":
            out[-1]["cands"].append(tuple(map(int, f[:5])))
        else:
            out[-1][tag] = tuple(map(int, f))
    return out


WHOLE = 40


def tok(c):
    """a table row's choice (family, cfg, nst, splits, bn) as one word"""
    return ".".join(map(str, c))


def summary(text):
    """the driver's plan as the golden keeps it, one line per key: the key, the default, its route, the candidates' number, the SHA-1 (12 digits) of the whole
    ordered list and its first three; an EXTRA key with at most WHOLE candidates is followed by the whole list.  (The whole lists of the table's keys are 20 000 words: the digest pins
    them, order included, and a mismatch names the key -- the driver's plan mode prints the list to look at.)"""
    out = []
    for r in parse_plan(text):
        words = [tok(c) for c in r["cands"]]
        out.append(f"key {' '.join(map(str, r['key']))} : model {tok(r['model'])} route {tok(r['route'])} : {len(words)} candidates "
                   f"{hashlib.sha1(' '.join(words).encode()).hexdigest()[:12]} first {' '.join(words[:3])}")
        if r["key"] in EXTRA and len(words) <= WHOLE:
            out.append("    all " + " ".join(words))
    return "\n".join(out) + "\n"


@lru_cache(maxsize=None)
def live():
    return plan(256, golden_keys())


def test_the_default_plan_and_the_candidates_are_the_recorded_ones():
    got, want = summary(live()).splitlines(), open(GOLDEN).read().splitlines()
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} lines differ; line {bad[0][0] + 1}: got {bad[0][1][:300]!r}, recorded {bad[0][2][:300]!r}"
    assert len(got) == len(want)


def test_the_recorded_plan_covers_what_it_should():
    recs = parse_plan(live())        # (the recorded plan: the test above)
    assert [r["key"] for r in recs] == golden_keys()
    for r in recs:
        assert r["cands"] and r["model"][0] == r["route"][0] and r["route"][1] >= 0, r["key"]
        flags = r["key"][12]
        if r["key"][0] == 0 and ((flags & 15) == GEGLU or flags & (LN | RS_OUT)):
            assert r["model"][3] == 1 and all(c[3] == 1 for c in r["cands"]), r["key"]           # one k-slice, default and measured
        if flags & W8:
            assert all(not (c[0] == 0 and c[1] & (8 | 32)) and not (c[0] == 1 and c[2] == 8) for c in r["cands"]), r["key"]      # no KS = 2, no loader-wave form
        assert all(c[0] == 0 for c in r["cands"]) or r["key"][0] == 1, r["key"]                   # the halo kernel competes for kind 1 only
    # the f16 rule: ranked with splits, then clamped -- the GEGLU launch takes the tile and ring of the plain GEMM's SPLIT winner
    by_key = {r["key"]: r for r in recs}
    plain = parse_plan(plan(256, [gemm_key(64, 640, 2560)]))[0]
    assert plain["model"][3] > 1 and by_key[gemm_key(64, 640, 2560, GEGLU)]["model"][:3] == plain["model"][:3]
    # one slab: nothing to split
    assert all(c[3] == 1 for c in by_key[halo_key(16, 64)]["cands"] if c[0] == 1) and by_key[halo_key(8, 1280)]["model"][3] > 1


def test_the_split_rule_is_the_one_the_tests_restate():
    for line in run("slices").splitlines():
        units, asked, s, per = map(int, line.split())
        assert s == tr.ci.slices(units, asked) and per == -(-units // asked) and (s - 1) * per < units <= s * per, line


def test_the_key_of_each_table_row_follows_from_the_call_it_describes():
    rows = tr.rows()
    calls = [(r.kind, r.M, r.N, r.K, r.batch, r.K if not r.conv else 0, r.H if r.conv else 0, r.W if r.conv else 0, r.Cin if r.conv else 0, r.k if r.conv else 0,
              r.stride if r.conv else 0, r.stride if r.conv else 0, r.act, int(r.residual), int(r.rowbias), int(r.bias_f32), int(r.ln), int(r.rs_in), int(r.rs_out),
              int(r.w8)) for r in rows]
    got = [tuple(map(int, x.split())) for x in run("keys", lines=calls).splitlines()]
    assert len(got) == len(rows)
    for r, k in zip(rows, got):
        r.check_decodes()
        assert k == (r.kind, r.device, r.M, r.N, r.K, r.batch, r.H, r.W, r.Cin, r.KW, r.sh, r.sw, r.flags), f"table line {r.line}: tune_key gives {k}"


def test_the_halo_gate_is_the_one_the_table_rows_are_checked_with():
    seen = set()
    for line in run("halo").splitlines():
        h, w, stride, n, takes = map(int, line.split())
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1

        def row(kind):
            return tr.Row(0, kind, 0, ho * wo, n, 576, 1, h, w, 64, 3, stride, stride, 0, 0, 2, 4, 1, 0)
        row(1 if takes else 2).check_decodes()          # (its assertion: kind 1 exactly where the halo predicate holds)
        if stride == 1:
            with pytest.raises(AssertionError, match="osg_conv3x3_prepare"):
                row(2 if takes else 1).check_decodes()
        else:
            assert not takes
        seen.add(takes)
    assert seen == {0, 1}
