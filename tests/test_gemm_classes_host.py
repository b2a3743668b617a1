"""CPU checks behind tests/test_gpu_gemm_classes.py: tests/gemm_classes_ref.py restates the constants and the rules that are
in the text of csrc/gemm.hip and ops.py today, every case of TILE_CASES, SKINNY_CASES, BIG_CASES, PANEL_CASES and SPLIT_CASES
is in the class it claims, their union reaches all 25 kernel instances (4 tile64 + 2 skinny + 4 big + 14 panel + the
split-K reduce) and every derived flag both ways, the exact inputs have one fp32 answer in three summation orders, the
real-valued bound leaves room for a correct fp32 evaluation in three orders, and eleven wrong kernels are caught on every
path they can occur on.  A failure on the GPU can then not be blamed on the case table, the inputs or the bound.

Where the GEMM shapes of tests/test_gpu_ops.py and tests/test_gpu_configs.py land (the gap this closes).  OLDER below
lists every call of those two files with the instance the restatement gives it, and test_where_the_older_shapes_land
regenerates the table and the sentences after it:
  test_gemm_layouts        7 shapes x 4 layouts on tile64 (323^3 is 9 big tiles of the 160 the big kernel wants), but
                           (8192,32,416) NN on skinny<1>
  test_gemm_epilogues      (150,45,37) NN: tile64<0,0>, the only shape the six epilogues met
  test_gemm_split_k_...    (48,32,4096) TN, split 2, 7, 64: tile64<1,0> + reduce, EPI_NONE, no slice with a K tail
  test_gemm_tall_skinny    skinny<1> and skinny<2>: none/relu/cross, K in {1, 8, 17, 32, 80, 129, 192, 741}
  test_gpu_configs         big<0,0> once at (3000,1001,200) with none/bias/relu/add; big<1,0> and big<1,1> only at M or
                           K = 16384; big<0,1> never; panel MAXB 3 and 7 only, M a multiple of 64, K in {323, 835, 96, 33}
Never before: a slice with a K tail, a request that collapses to one slice (the one request that shrank is split_k_for's 56
at D = 323: 54 slices of 304); panel MAXB 1, 2, 4, 5, 6; a partial row block, K < 16, K = 16 or K = 32 on the panel
kernel.  (That the reduce met no epilogue and the big kernel no cross, sigmoid, tanh or aux is in the text of those tests,
not in their shapes.)
"""
import os
import re

import numpy as np
import pytest

from tests import gemm_classes_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explicit-tf2-recommendation_amd")
C = GR.C


@pytest.fixture(scope="module")
def text():
    with open(os.path.join(PKG, "csrc", "gemm.hip")) as f:
        return f.read()


@pytest.fixture(scope="module")
def ops_text():
    with open(os.path.join(PKG, "ops.py")) as f:
        return f.read()


def _one(pattern, text, what, count=1):
    found = re.findall(pattern, text)
    assert len(found) == count and len(set(found)) == 1, "%s found %d times as %s, the tests expect %d identical" % (
        what, len(found), sorted(set(found)), count)
    return found[0]


def _ints(t):
    return tuple(int(v) for v in t)


# ---- the restatement is the source's ---------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source(text, ops_text):
    got = {}
    got["BM"], got["BN"], got["BK"] = _ints(_one(
        r"constexpr int BM = (\d+), BN = (\d+), BK = (\d+), PAD = 1;", text, "the tile64 constants"))
    got["LM"], got["LN"], got["LK"] = _ints(_one(
        r"constexpr int LM = (\d+), LN = (\d+), LK = (\d+), LPAD = 4;", text, "the big constants"))
    got["PNB"] = int(_one(r"constexpr int PNB = (\d+), PPAD = 4;", text, "PNB"))
    got["PMt"], got["PKt"] = _ints(_one(r"constexpr int PMt = (\d+), PKt = (\d+);", text, "the panel instance"))
    e1, e2, got["BIG_MIN"] = _ints(_one(
        r"const bool big = M > (\d+) && N > (\d+) && ceil_div64\(M, LM\) \* ceil_div64\(N, LN\) \* split_k >= (\d+);",
        text, "the big rule"))
    got["SKINNY_N"], got["SKINNY_M"] = _ints(_one(
        r"if \(!transA && !transB && N <= (\d+) && M >= (\d+) && split_k == 1\) \{", text, "the skinny rule"))
    got["SKINNY_NT1"] = int(_one(r"\n    if \(N <= (\d+)\)\n      hipLaunchKernelGGL\(\(gemm_f32_skinny_kernel<1>\)", text,
                                 "the NT rule"))
    got["SKINNY_ROWS"] = int(_one(r"dim3 grid\(\(unsigned\)ceil_div64\(M, (\d+)\)\);", text, "the skinny grid"))
    assert _one(r"const int64_t m0 = \(int64_t\)blockIdx\.x \* (\d+);", text, "the skinny row block") == "32"
    e3, a, b, got["PANEL_MAX_COLS"], got["PANEL_MAX_K"], rows, got["PANEL_MIN_WG"] = _ints(_one(
        r"const bool panel_fwd = !transA && split_k == 1 && N > (\d+) &&\s+"
        r"\(\(ncol_panels == 1 && M >= (\d+) \* (\d+)\) \|\|\s+"
        r"\(ncol_panels > 1 && ncol_panels <= (\d+) && K <= (\d+) && ceil_div64\(M, (\d+)\) \* ncol_panels >= (\d+)\)\);",
        text, "the panel rule"))
    got["PANEL_ROWS"] = a * b
    assert rows == got["PMt"], "the panel rule counts workgroups of another height than the kernel's"
    o1, o2 = _ints(_one(r"t = 128 if \(M > (\d+) and N > (\d+)\) else 64 ", ops_text, "split_k_for's tile rule"))
    assert len({e1, e2, e3, o1, o2}) == 1, "the five uses of the edge 64 differ: %s" % ((e1, e2, e3, o1, o2),)
    got["EDGE"] = e1
    assert "t = %d if (M > %d and N > %d) else %d " % (got["LM"], o1, o2, got["BM"]) in ops_text
    got["SK_MAX_TILES"], got["SK_MIN_K"] = _ints(_one(r"if tiles >= (\d+) or K < (\d+):\n        return 1", ops_text,
                                                     "split_k_for's early return"))
    got["SK_SLOTS_FEW"], got["SK_FEW"], got["SK_SLOTS"] = _ints(_one(
        r"slots = (\d+) if tiles < (\d+) else (\d+)\n", ops_text, "split_k_for's slots"))
    got["SK_MAX"], got["SK_MIN_DEPTH"] = _ints(_one(
        r"split = max\(1, min\((\d+), slots // max\(tiles, 1\), K // (\d+)\)\)", ops_text, "split_k_for's split"))
    cmin, mb = _ints(_one(r"cap = max\((\d+), \((\d+) << 20\) // max\(1, 4 \* M \* N\)\)", ops_text, "split_k_for's cap"))
    got["SK_CAP_MIN"], got["SK_WS_BYTES"] = cmin, mb << 20
    for field in GR.Consts._fields:
        assert got[field] == getattr(C, field), "the source has %s = %s, gemm_classes_ref.C.%s = %s" % (
            field, got[field], field, getattr(C, field))


def test_rules_are_the_ones_in_the_source(text, ops_text):
    for line in (
            "  if (M == 0 || N == 0) return REC_OK;\n  if (split_k < 1) split_k = 1;\n"
            "  if (split_k > 1 && !workspace) return REC_E_WORKSPACE;",
            "    kchunk = ((ceil_div64(K, split_k) + BK - 1) / BK) * BK;\n    if (kchunk < BK) kchunk = BK;\n"
            "    split_k = (int)ceil_div64(K, kchunk);\n    if (split_k < 1) split_k = 1;",
            "float* ws = split_k > 1 ? workspace : nullptr;",
            "const int64_t ncol_panels = N <= PNB * 32 ? 1 : ceil_div64(N, PNB * 32);",
            "const int64_t ncp = ncol_panels == 1 ? 0 : ((ceil_div64(N, ncol_panels) + 31) / 32) * 32;",
            "const int maxb = (int)ceil_div64(ceil_div64(ncp > 0 ? ncp : N, 32), 4);",
            "constexpr int PMt = 64, PKt = 16;",
            "if (transB) { PANEL_MB(0, 1); } else { PANEL_MB(0, 0); }",
            "const int psplit = 1;",
            "const int64_t kper = ((((K + 15) >> 4) + 3) >> 2) << 4;",
            "for (int64_t k0 = k_begin; k0 < k_end; k0 += 32) {",
            "if (gx + 3 < X && gk < k_end) {",
            "const int64_t Kfull = (K / PKt) * PKt;",
            "for (; z + 4 <= split; z += 4) {",
            "float acc = (a0 + a1) + (a2 + a3);",
            "float v = (part[0][r][c] + part[1][r][c]) + (part[2][r][c] + part[3][r][c]);"):
        assert line in text, "gemm.hip no longer holds: " + line
    # the order of the branches: skinny, panel, big, tile64
    at = [text.index(s) for s in ("gemm_f32_skinny_kernel<1>), grid", "if (panel_fwd) {", "\n  if (big) {", "#define LAUNCH(TA, TB)")]
    assert at == sorted(at)
    assert re.findall(r"case (\d): PANEL\(TAv, TBv, (\d)\); break;", text) == [(str(i), str(i)) for i in range(1, 7)]
    assert "default: PANEL(TAv, TBv, 7); break;" in text
    for line in (
            "skinny = (not transA) and (not transB) and N <= 64 and M >= 256 ",
            "split_k = 1 if skinny else split_k_for(K, M, N, transA, transB)",
            "tiles = ((M + t - 1) // t) * ((N + t - 1) // t)",
            "return int(min(split, cap))"):
        assert line in ops_text, "ops.py no longer holds: " + line


def test_the_shapes_the_issue_checked():
    P = GR.gemm_path
    p = P(0, 0, 1665, 1665, 19)
    assert p.kernel == "big" and GR.cdiv(1665, C.LM) ** 2 == 196
    p = P(1, 0, 129, 129, 640, 40)
    assert (p.kernel, p.split_k, p.kchunk, p.last_depth) == ("big", 40, 16, 16) and 4 * 40 == C.BIG_MIN
    p = P(1, 0, 129, 129, 641, 41)
    assert (p.kernel, p.split_k, p.kchunk, p.last_depth) == ("big", 41, 16, 1)
    p = P(0, 1, 6081, 897, 5)
    assert (p.kernel, p.ncol_panels, p.ncp, 897 - p.ncp) == ("panel", 2, 480, 417)
    p = P(0, 0, 4096, 1793, 37)
    assert (p.kernel, p.ncol_panels, p.ncp) == ("panel", 3, 608)
    p = P(0, 0, 129, 56449, 5)
    assert (p.kernel, p.ncol_panels, p.ncp, p.MAXB) == ("panel", 64, 896, 7)
    assert P(0, 0, 129, 56449 + 896, 5).kernel == "big"                         # 65 panels: past the limit
    assert P(0, 1, 6080, 897, 5).kernel == "big" and P(0, 0, 4096, 1793, 257).kernel == "big"
    assert P(0, 0, 323, 323, 323).kernel == "tile64" and P(1, 0, 323, 323, 323).kernel == "tile64"
    assert P(0, 0, 8192, 32, 416).kernel == "skinny" and P(0, 1, 8192, 32, 416).kernel == "tile64"
    assert P(0, 0, 150, 45, 37).kernel == "tile64"
    for s in (2, 7, 64):
        p = P(1, 0, 48, 32, 4096, s)
        assert (p.kernel, p.split_k, p.kchunk % 16, p.ktail) == ("tile64", s, 0, 0) and p.last_depth >= 64
    assert P(0, 0, 3000, 1001, 200).kernel == "big" and P(0, 1, 16384, 323, 323).kernel == "panel"
    assert P(0, 1, 16384, 323, 323).MAXB == 3 and P(0, 1, 16384, 835, 835).MAXB == 7
    # split_k=None is ops.gemm: 1 on a skinny shape and for K < 1024, split_k_for elsewhere
    assert P(0, 0, 8192, 32, 4096).kernel == "skinny" and P(1, 0, 48, 32, 4096).split_k == 64
    assert GR.split_k_for(16384, 835, 835) == 15 and GR.split_k_for(16384, 323, 323) == 56
    # a request can shrink, down to one slice
    assert P(1, 0, 48, 32, 40, 8).split_k == 3 and P(1, 0, 48, 32, 16, 4).split_k == 1 and P(1, 0, 48, 32, 1, 64).split_k == 1


# every ops.gemm call of the two older files: (transA, transB, M, N, K, split_k as passed) -> what the module docstring says
_L7 = [(64, 64, 16), (8192, 32, 416), (100, 8, 32), (77, 1, 8), (323, 323, 323), (130, 70, 1), (5, 3, 2)]
OLDER = {
    "test_gemm_layouts": [(a, b) + s + (None,) for s in _L7 for a, b in GR.LAYOUTS],
    "test_gemm_epilogues": [(0, 0, 150, 45, 37, None)],
    "test_gemm_split_k_deterministic": [(1, 0, 48, 32, 4096, s) for s in (2, 7, 64)],
    "test_gemm_tall_skinny": [(0, 0) + s + (None,) for s in [(256, 32, 741), (8192, 32, 741), (257, 1, 8), (1000, 8, 32),
                                                              (4096, 64, 192), (300, 33, 17), (511, 2, 80), (2048, 64, 1),
                                                              (290, 20, 129)]],
    "test_short_k_wide_n_gemm_in_column_panels": [(0, tb, M, N, K, None) for M, N, K, tb in
                                                  [(4096, 3492, 96, 0), (4096, 3492, 96, 1), (3000, 1001, 200, 0),
                                                   (2048, 5000, 33, 1)]],
    "test_crossnet_gemms_at_config_c": [call for D in (323, 835) for call in
                                        [(0, 1, 16384, D, D, None), (0, 0, 16384, D, D, None), (1, 1, 16384, D, D, None)] +
                                        [(1, 0, D, D, 16384, s) for s in (None, 8, 40)]],
}


def test_where_the_older_shapes_land():
    """the table of the module docstring, from the restatement"""
    land = {t: [(call, GR.gemm_path(*call)) for call in calls] for t, calls in OLDER.items()}
    inst = lambda t: [GR.instance(p) for _, p in land[t]]
    assert sorted(set(inst("test_gemm_layouts"))) == ["skinny<1>"] + ["tile64<%d,%d>" % l for l in GR.LAYOUTS]
    assert [c[2:5] for c, p in land["test_gemm_layouts"] if p.kernel == "skinny"] == [(8192, 32, 416)]
    assert inst("test_gemm_epilogues") == ["tile64<0,0>"]
    assert inst("test_gemm_split_k_deterministic") == ["tile64<1,0>+reduce%d" % s for s in (2, 7, 64)]
    assert set(inst("test_gemm_tall_skinny")) == {"skinny<1>", "skinny<2>"}
    assert {c[4] for c in OLDER["test_gemm_tall_skinny"]} == {1, 8, 17, 32, 80, 129, 192, 741}
    assert inst("test_short_k_wide_n_gemm_in_column_panels") == ["panel<0,0,7>x4", "panel<0,1,7>x4", "big<0,0>",
                                                                 "panel<0,1,7>x6"]
    assert inst("test_crossnet_gemms_at_config_c") == [
        "panel<0,1,3>", "panel<0,0,3>", "big<1,1>", "big<1,0>+reduce54", "tile64<1,0>+reduce8", "big<1,0>+reduce40",
        "panel<0,1,7>", "panel<0,0,7>", "big<1,1>", "big<1,0>+reduce15", "big<1,0>+reduce8", "big<1,0>+reduce40"]
    every = [(c, p) for t in land for c, p in land[t]]
    big = [(c, p) for c, p in every if p.kernel == "big"]
    assert [c[2:5] for c, p in big if (p.TA, p.TB) == (0, 0)] == [(3000, 1001, 200)]
    assert not [c for c, p in big if (p.TA, p.TB) == (0, 1)]
    assert all(16384 in (c[2], c[4]) for c, p in big if p.TA == 1)
    panel = [(c, p) for c, p in every if p.kernel == "panel"]
    assert {p.MAXB for _, p in panel} == {3, 7} and {c[4] for c, _ in panel} == {323, 835, 96, 33}
    assert not any(p.partial_rows or p.kfull0 or p.kfull1 or c[4] == 32 for c, p in panel)
    sliced = [(c, p) for c, p in every if p.split_k > 1]
    assert all(p.ktail == 0 for _, p in sliced)
    assert all(p.split_k == (c[5] or GR.split_k_for(c[4], c[2], c[3])) for c, p in sliced
               if (c[2], c[5]) != (323, None)) and GR.split_k_for(16384, 323, 323) == 56     # 56 asked, 54 slices of 304
    assert not any(c[5] and c[5] > 1 and p.split_k == 1 for c, p in every)


# ---- membership and coverage -----------------------------------------------------------------------------------------
def test_every_case_is_in_the_class_it_claims():
    for c in GR.ALL_CASES:
        p = GR.path_of(c)
        assert GR.instance(p) == c.cls, (c.name, GR.instance(p))
        assert c.K < 16381 and max(c.M, c.N) >= 1
    for table, kernel in ((GR.TILE_CASES, "tile64"), (GR.SKINNY_CASES, "skinny"), (GR.BIG_CASES, "big"),
                          (GR.PANEL_CASES, "panel"), (GR.SPLIT_CASES, "tile64")):
        assert {GR.path_of(c).kernel for c in table} == {kernel}
    for name in GR.REAL_CASES:
        assert name in GR.BY_NAME
    assert {f for n in GR.REAL_CASES for f in GR.families_of(GR.path_of(GR.BY_NAME[n]))} == set(GR.FAMILIES)
    assert {GR.instance(GR.path_of(GR.BY_NAME[n])).split("<")[0] for n in GR.REAL_CASES} == {"tile64", "skinny", "big", "panel"}


def test_the_tables_reach_every_instance_and_flag():
    P = {c.name: GR.path_of(c) for c in GR.ALL_CASES}
    reached = {i for p in P.values() for i in GR.instances_of(p)}
    assert reached == set(GR.ALL_INSTANCES) and len(GR.ALL_INSTANCES) == 25
    by = lambda kernel, **kw: [n for n, p in P.items() if p.kernel == kernel and all(getattr(p, k) == v for k, v in kw.items())]
    for kernel in ("tile64", "skinny", "big", "panel"):
        assert by(kernel, partial_rows=True) and by(kernel, partial_rows=False), kernel
        tails = {p.ktail for p in P.values() if p.kernel == kernel}
        assert 0 in tails and 1 in tails and 15 in tails, (kernel, tails)
    # tile64 and big: every layout with and without a K tail, with full and partial row blocks
    for kernel in ("tile64", "big"):
        for a, b in GR.LAYOUTS:
            assert {(p.ktail > 0) for p in P.values() if (p.kernel, p.TA, p.TB) == (kernel, a, b)} == {False, True}
            assert by(kernel, TA=a, TB=b, partial_rows=True)
    # skinny: one, two and three idle waves and none, both instances; a 32-deep round that ends inside a 16-deep step
    for nt in (1, 2):
        assert {p.empty_waves for p in P.values() if p.kernel == "skinny" and p.NT == nt} == {0, 1, 2, 3}
        assert {c.N for c in GR.SKINNY_CASES if P[c.name].NT == nt} == ({1, 31, 32} if nt == 1 else {33, 63, 64})
        assert {c.M for c in GR.SKINNY_CASES if P[c.name].NT == nt} == {256, 257, 287}
        assert {c.K for c in GR.SKINNY_CASES if P[c.name].NT == nt} == set(GR.SKINNY_K)
    assert any((e - b) % 32 == 16 for b, e in GR.skinny_ranges(129)) and GR.skinny_ranges(129)[3] == (144, 144)
    # big: straddling 16-byte pieces with each k-major operand, and none; M % 128 in {1, 127}; slices with a short last one
    big = {n: p for n, p in P.items() if p.kernel == "big"}
    assert {(p.TA, p.TB, p.straddle) for p in big.values()} >= {(0, 0, True), (1, 0, True), (1, 1, True), (1, 0, False),
                                                               (0, 1, False)}
    assert {GR.BY_NAME[n].M % C.LM for n in big} >= {0, 1, 127}
    assert {GR.BY_NAME[n].K for n, p in big.items() if p.split_k == 1} >= {1, 15, 16, 17, 35}
    assert any(p.split_k == 1 and p.ktail == 0 and (p.TA, p.TB) == (0, 0) for p in big.values())
    for a, b in GR.LAYOUTS:
        assert {p.last_depth for p in big.values() if (p.TA, p.TB) == (a, b) and p.split_k > 1} >= {1, 16}
    # panel: every MAXB with both TB at a tail-only, an exact and a ragged K; acting row clamps; every K at two N
    one = {n: p for n, p in P.items() if p.kernel == "panel" and p.ncol_panels == 1}
    for mb in range(1, 8):
        for tb in (0, 1):
            mine = [(GR.BY_NAME[n].K, p) for n, p in one.items() if (p.MAXB, p.TB) == (mb, tb)]
            assert any(p.kfull0 for _, p in mine), (mb, tb)
            assert any(p.ktail == 0 for _, p in mine) and any(p.ktail and not p.kfull0 for _, p in mine), (mb, tb)
    assert {GR.BY_NAME[n].M for n in one} == {8192, 8193, 8255}
    assert {GR.BY_NAME[n].N for n in one} == {65, 128, 129, 257, 385, 513, 641, 769, 896}
    for N in (65, 129):
        assert {GR.BY_NAME[n].K for n in one if GR.BY_NAME[n].N == N} >= {1, 7, 15, 16, 17, 32, 33, 53}
    assert {(p.kfull0, p.kfull1) for p in one.values()} == {(True, False), (False, True), (False, False)}
    many = {n: p for n, p in P.items() if p.kernel == "panel" and p.ncol_panels > 1}
    assert {p.ncol_panels for p in many.values()} == {2, 3, 64} and {p.TB for p in many.values()} == {0, 1}
    assert {p.narrow_last for p in many.values()} == {False, True}
    assert {p.partial_rows for p in many.values()} == {False, True}
    # the reduce: every remainder of the four-chain loop, a collapsed request, a shrunk one, a last slice of one k
    eff = {p.split_k for n, p in P.items() if p.split_k > 1 and p.kernel == "tile64"}
    assert eff >= {2, 3, 4, 5, 7, 8} and {s % 4 for s in eff} == {0, 1, 2, 3}
    assert any(c.split and c.split > 1 and P[c.name].split_k == 1 for c in GR.SPLIT_CASES)
    assert any(c.split and 1 < P[c.name].split_k < c.split for c in GR.SPLIT_CASES)
    assert any(P[c.name].last_depth == 1 for c in GR.SPLIT_CASES)
    assert {(P[c.name].TA, P[c.name].TB) for c in GR.SPLIT_CASES if P[c.name].split_k > 1} == set(GR.LAYOUTS)


# ---- the exact inputs ------------------------------------------------------------------------------------------------
def _rows(M):
    """the rows on which the slower summation orders run: all of a small matrix, the first and the last 48 of a tall one
    (the argument for exactness is per element and the same in every row)"""
    return np.arange(M) if M <= 256 else np.r_[0:48, M - 48:M]


def _cols(N):
    return np.arange(N) if N <= 2048 else np.r_[0:64, N - 64:N]


@pytest.mark.parametrize("name", [c.name for c in GR.ALL_CASES if c.K <= 1024])
def test_exact_inputs_have_one_fp32_answer(name):
    c, x = GR.BY_NAME[name], GR.exact_input(name)
    assert set(np.unique(x.A * 8)) <= set(range(-8, 9)) and set(np.unique(x.bias * 8)) <= set(range(-16, 17))
    rows, cols = _rows(c.M), _cols(c.N)
    A, B = x.A[rows], np.ascontiguousarray(x.B[:, cols])
    ref = A.astype(np.float64) @ B.astype(np.float64)
    for order in GR.ORDERS:
        got = GR.f32_product(A, B, order)
        assert np.array_equal(got.astype(np.float64), ref), (name, order)
    sub = GR.Inputs(A, B, x.bias[cols], x.e0[np.ix_(rows, cols)], x.e1[np.ix_(rows, cols)])
    for epi in GR.EXACT_EPIS:
        want = GR.exact_reference(sub, epi)                    # asserts that the cast to fp32 is lossless
        got = GR.f32_epilogue(GR.f32_product(A, B, "chain"), sub, epi)
        for g, w in zip(got, want):
            assert (g is None) == (w is None) and (g is None or np.array_equal(g.view(np.uint32), w.view(np.uint32)))
    sa, sb = GR.activation_scale(c.K)
    u = (A * np.float32(sa)).astype(np.float64) @ (B * np.float32(sb)).astype(np.float64) + sub.bias
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert np.abs(u).max() <= 8, (name, np.abs(u).max())         # the activations are asked about arguments of order 1


def test_the_deepest_case_is_exact_too():
    c = GR.BY_NAME["split_tn_70x70x4096_s64"]
    x = GR.exact_input(c.name)
    ref = x.A.astype(np.float64) @ x.B.astype(np.float64)
    for order in GR.ORDERS:
        assert np.array_equal(GR.f32_product(x.A, x.B, order).astype(np.float64), ref)
    assert 512 * (2 * c.K + 6) < 2 ** 24 and 64 * c.K < 2 ** 24


# ---- the bound: room for a correct fp32 evaluation, none for a wrong one ----------------------------------------------
ROOM = 0.75    # one product and one addition (K = 1 with a bias) use at most half: u |ab| + ulp/2 of 2 u |ab| + ulp


@pytest.mark.parametrize("name", GR.REAL_CASES)
def test_a_correct_fp32_evaluation_stays_inside_the_bound(name):
    c, x, p = GR.BY_NAME[name], GR.real_input(name), GR.path_of(GR.BY_NAME[name])
    rows = _rows(c.M)
    sub = GR.Inputs(x.A[rows], x.B, x.bias, x.e0[rows], x.e1[rows])
    for epi in GR.REAL_EPIS:
        (ref, u), (bC, bu) = GR.reference(sub, epi), GR.real_bounds(sub, p, epi)
        for order in GR.ORDERS:
            got, aux = GR.f32_epilogue(GR.f32_product(sub.A, sub.B, order), sub, epi)
            q = GR.ratio(got, ref, bC)
            assert q <= ROOM, (name, epi, order, q)
            if aux is not None:
                assert GR.ratio(aux, u, bu) <= ROOM, (name, epi, order)


def test_the_bound_is_as_tight_as_the_issue_says():
    """at (129,129,641) the fp32 product uses below 1 % of the bound and a dropped last k leaves it on most elements"""
    r = np.random.Generator(np.random.PCG64(641))
    x = GR.Inputs(r.normal(size=(129, 641)).astype(np.float32), r.normal(size=(641, 129)).astype(np.float32),
                  np.zeros(129, np.float32), None, None)
    p = GR.gemm_path(0, 0, 129, 129, 641)
    bound, _ = GR.real_bounds(x, p, "none")
    ref, _ = GR.reference(x, "none")
    assert GR.ratio(GR.f32_product(x.A, x.B, "chain"), ref, bound) < 0.02
    dropped = x.A[:, :-1].astype(np.float64) @ x.B[:-1].astype(np.float64)
    assert (np.abs(dropped - ref) > bound).mean() > 0.9


def _candidates(fam):
    cs = [c for c in GR.ALL_CASES if fam in GR.families_of(GR.path_of(c))]
    return sorted(cs, key=lambda c: c.M * c.N * max(c.K, 1))


@pytest.mark.parametrize("mut", list(GR.MUTANTS))
def test_a_wrong_kernel_is_caught_on_every_path_it_can_occur_on(mut):
    for fam in GR.MUTANTS[mut]:
        hit = next((c.name for c in _candidates(fam) if GR.caught_exact(c, mut)), None)
        assert hit is not None, "no exact case of %s catches %s" % (fam, mut)
    caught = set()
    for name in GR.REAL_CASES:
        c = GR.BY_NAME[name]
        if set(GR.families_of(GR.path_of(c))) & set(GR.MUTANTS[mut]) and GR.caught_by_bound(c, mut):
            caught |= set(GR.families_of(GR.path_of(c)))
    if GR.MUTANT_EPI[mut] in GR.REAL_EPIS:
        assert caught >= set(GR.MUTANTS[mut]), (mut, sorted(set(GR.MUTANTS[mut]) - caught))


def test_a_right_kernel_is_not_caught():
    for name in ("tile_tn_65x65x17", "split_tn_48x32x100_s7", "skinny_nn_257x31x65"):
        c = GR.BY_NAME[name]
        for epi in sorted(set(GR.MUTANT_EPI.values())):
            x = GR.exact_input(name)
            Cb, auxb = GR.restated(c, x, epi)
            want, u = GR.exact_reference(x, epi)
            assert np.array_equal(Cb[:c.M, :c.N].view(np.uint32), want.view(np.uint32))
            assert (Cb[c.M] == GR.SENT).all() and (Cb[:, c.N:] == GR.SENT).all()
            if u is not None:
                assert np.array_equal(auxb[:c.M, :c.N].view(np.uint32), u.view(np.uint32))
