"""CPU checks behind tests/test_gpu_lookup_classes.py: tests/lookup_classes_ref.py restates the thresholds that are in the
text of csrc/embedding.hip today, every case of FM_FWD_CASES, GATHER_CASES, LISTS_CASES and FM_BWD_CASES is in the class
and holds the regimes it claims, their union reaches every template instantiation and regime, the integer-valued cases
cannot round, the references agree with each other and the bound of the normal-valued forward has room.  The class and
coverage tests run against the thresholds parsed out of the source (``th``), so a threshold edited in embedding.hip fails
the restatement test by name and the tables by case.  A failure on the GPU can then not be blamed on the case table."""
import os
import re

import numpy as np
import pytest

from oracle import layers_np as L
from tests import lookup_classes_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc", "embedding.hip")


def _one(pattern, text, what, count=1):
    """the single value ``pattern`` captures, found ``count`` times with the same value"""
    found = re.findall(pattern, text)
    assert len(found) == count and len(set(found)) == 1, "embedding.hip: %s found %d times as %s, the tests expect %d " \
        "identical" % (what, len(found), sorted(set(found)), count)
    return found[0]


def _body(text, head):
    body = text[text.index(head):]
    return body[:body.index("\n}\n")]


def _switch(body, pattern, default, what):
    pairs = re.findall(pattern, body)
    assert pairs and all(a == b for a, b in pairs), "%s: a case label launches another instantiation: %s" % (what, pairs)
    return tuple(int(a) for a, _ in pairs) + ((int(_one(default, body, what + " default")),) if default else ())


def source_thresholds(text):
    gather = _body(text, 'extern "C" int rec_emb_gather_f32(')
    lists = _body(text, 'extern "C" int rec_emb_gather_lists_f32(')
    fwd = _body(text, 'extern "C" int rec_emb_fm_fwd_f32(')
    loop = re.search(r"while \(split < (\d+) && LPR \* split \* 2 <= (\d+) && \(a\.F \+ split - 1\) / split > 1 &&\s*"
                     r"\(\(a\.F \+ split - 1\) / split > (\d+) \|\| a\.B \* LPR \* split < (\d+) \* (\d+)\)\)\s*"
                     r"split \*= 2;", text)
    assert loop, "embedding.hip: the split loop of dispatch_vec no longer reads as lookup_classes_ref.split_of restates it"
    max_split, wave, loop_nl, fa, fb = (int(x) for x in loop.groups())
    nl = int(_one(r"constexpr int NL = (\d+);", text, "NL"))
    assert loop_nl == nl, "the split loop keeps <= %d fields per lane group, the kernel has NL = %d loads in flight" % (
        loop_nl, nl)
    lds_kb = int(_one(r"\(size_t\)a\.F > (\d+) \* 1024\) return false;", text, "the id-staging limit"))
    max_e = {int(_one(r"if \(E > (\d+)\) return REC_E_UNSUPPORTED;", fwd, "the forward's E limit")),
             int(_one(r"E >= 4 && E <= (\d+)\)", gather, "the E limit of gather_rows")),
             int(_one(r"E >= 4 && E <= (\d+)\)", lists, "the E limit of the list gather"))}
    assert len(max_e) == 1, "the three E limits differ: %s" % sorted(max_e)
    max_e = max_e.pop()
    rungs = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"if \(E <= (\d+)\) FWD_GEN\((\d+), (\d+)\);", fwd)]
    last = re.findall(r"\n\s*else FWD_GEN\((\d+), (\d+)\);", fwd)
    assert len(last) == 1, "the FWD_GEN ladder has no single final else"
    return LR.Thresholds(
        UNR=int(_one(r"constexpr int UNR = (\d+);", text, "UNR", 2)), NL=nl, LDS_LIMIT=lds_kb * 1024, FILL=fa * fb,
        MAX_SPLIT=max_split, WAVE=wave,
        MAX_FUSED_LD=int(_one(r"\(ld_e & \(ld_e - 1\)\) == 0 && ld_e <= (\d+);", fwd, "the fused ld_e limit")),
        MAX_VEC_E=int(_one(r"if \(!done && \(E & \(E - 1\)\) == 0 && E <= (\d+)\) done = dispatch_lpr<false>\(a, E / 4\);",
                           fwd, "the separate vec class's E limit")),
        MAX_E=max_e,
        HDR=int(_one(r"msg, cap, \\\n\s*(\d+), n, \(float4\*\)out, oob_flag, nc\)", text, "the header words")),
        ROWS_LPRS=_switch(gather, r"case (\d+): GATHER_ROWS\((\d+)\); break;", r"default: GATHER_ROWS\((\d+)\); break;",
                          "GATHER_ROWS"),
        LISTS_LPRS=_switch(lists, r"case (\d+): GATHER_LISTS\((\d+)\); break;",
                           r"default: GATHER_LISTS\((\d+)\); break;", "GATHER_LISTS"),
        FWD_LPRS=_switch(text, r"case (\d+): return dispatch_vec<(\d+), FUSED>\(a\);", None, "dispatch_lpr"),
        GEN_LADDER=tuple(rungs) + ((max_e, int(last[0][0]), int(last[0][1])),))


@pytest.fixture(scope="module")
def text():
    with open(SOURCE) as f:
        return f.read()


@pytest.fixture(scope="module")
def th(text):
    return source_thresholds(text)


# ---- the restatements are the source's ------------------------------------------------------------------------------
def test_thresholds_are_the_ones_in_the_source(th):
    for field in LR.Thresholds._fields:
        assert getattr(th, field) == getattr(LR.TH, field), "embedding.hip has %s = %s, lookup_classes_ref.TH.%s = %s" % (
            field, getattr(th, field), field, getattr(LR.TH, field))
    assert (LR.TH.UNR, LR.TH.NL, LR.TH.LDS_LIMIT, LR.TH.FILL, LR.TH.HDR, LR.TH.MAX_E, LR.TH.MAX_FUSED_LD) == (
        4, 16, 61440, 65536, 2, 256, 64)


def test_dispatch_text_is_what_the_restatements_read(text):
    for line in (
            "return E % 4 == 0 && ld % 4 == 0 && rec_is_aligned16(p);",
            "if (vec4_ok(table, E, ld) && vec4_ok(out, E, E) && (E & (E - 1)) == 0 && E >= 4 && E <= 256) {",
            "} else if (vec4_ok(table, E, ld) && vec4_ok(out, E, E)) {",
            "const unsigned grid = (unsigned)ceil_div64(n, (256 / lpr) * UNR);",
            "constexpr int R = 256 / LPR;",
            "if (!(vec4_ok(table, E, ld) && vec4_ok(out, E, E) && E >= 4 && E <= 256)) return REC_E_UNSUPPORTED;",
            "const int nc = E / 4;", "while (lpr < nc) lpr *= 2;",
            "if (sizeof(int) * (size_t)(256 / (LPR * split)) * (size_t)a.F > 60 * 1024) return false;",
            "else launch_vec<LPR, (LPR * 4 <= 64 ? 4 : 2), FUSED>(a);",
            "bool out_ok = (!emb_out || rec_is_aligned16(emb_out)) && (!sumvec || rec_is_aligned16(sumvec));",
            "if (vec4_ok(embed, E, ld_e) && out_ok) {",
            "bool fused = (w == embed + E) && ld_w == ld_e && ld_e > E && (ld_e & (ld_e - 1)) == 0 && ld_e <= 64;",
            "if (fused) done = dispatch_lpr<true>(a, (int)(ld_e / 4));",
            "constexpr int EPW = 256 / LPE;", "const int FP = (F + SPLIT - 1) / SPLIT;",
            "if (V >= (int64_t(1) << 31)) return REC_E_UNSUPPORTED;",
            "bool ok = (uint64_t)id < (uint64_t)V;\n    bad |= !ok;\n    ids_lds[i] = ok ? (int)id : -1;",
            "if (E % 4 == 0 && al && (emb_rows || vec4_ok(embed, E, ld_e))) {",
            "bool al = rec_is_aligned16(sumvec) && rec_is_aligned16(dvals) && (!emb_rows || rec_is_aligned16(emb_rows)) "
            "&&\n            (!extra || rec_is_aligned16(extra));"):
        assert line in text, "embedding.hip no longer holds: " + line
    assert text.count("E >= 4 && E <= 256") == 2 and text.count("constexpr int UNR = 4;") == 2


def test_class_functions_over_the_whole_range(th):
    ladder = {top: (g, a) for top, g, a in th.GEN_LADDER}
    for E in range(1, 257):
        for ld in (E, E + 1, E + 4, 2 * E):
            for al in (True, False):
                g = LR.gather_class(E, ld, al, True, th)
                both = E % 4 == 0 and ld % 4 == 0 and al
                if both and LR.is_pow2(E) and E >= 4:
                    assert g == ("rows", E // 4, 1024 // E, 4 * (1024 // E)), (E, ld, g)      # the switch is complete
                else:
                    assert g.kernel == ("vec4" if both else "scalar")
                assert LR.gather_class(E, ld, True, False, th).kernel == "scalar"
                c = LR.lists_class(E, ld, al, th)
                if both and E >= 4:
                    assert c.nc == E // 4 and c.lpr >= c.nc and c.lpr < 2 * c.nc and LR.is_pow2(c.lpr)
                    assert c.R == 256 // c.lpr and c.rows_per_wg == 4 * c.R and c.hdr == 2
                else:
                    assert c is None
                for rows in (True, False):
                    assert LR.fm_bwd_class(E, ld, rows, al) == ("vec" if E % 4 == 0 and al and (rows or ld % 4 == 0)
                                                                else "scalar")
        f = LR.fm_fwd_class(37, 3, E, E + 1, False, True, th)          # ld % 4 and E % 4 cannot both be 0
        assert f.kernel == "gen" and (f.GW, f.NACC) == ladder[min(t for t in ladder if E <= t)]
        assert f.GW * f.NACC >= E and (f.GW >= min(E, 64)) and (f.GW == 1 or f.GW // 2 < E)
    assert LR.gather_class(260, 260).kernel == "vec4" and LR.gather_class(512, 512).kernel == "vec4"
    assert LR.lists_class(260, 260) is None and LR.lists_class(6, 8) is None
    for B, F, LPR, want in ((65536, 2, 1, 1), (65535, 2, 1, 2), (16384, 10, 8, 1), (8192, 16, 8, 1), (8192, 17, 8, 2),
                            (8192, 33, 8, 4), (37, 1, 4, 1), (37, 3, 4, 4), (37, 5, 16, 4), (37, 64, 4, 4)):
        assert LR.split_of(B, F, LPR, th) == want, (B, F, LPR)
    for B, F, E in ((3, 5, 0), (3, 0, 4), (3, 5, 257)):
        with pytest.raises(ValueError):
            LR.fm_fwd_class(B, F, E, max(E, 1))
    with pytest.raises(ValueError):
        LR.gather_class(4, 3)


# ---- the forward table ----------------------------------------------------------------------------------------------
def test_forward_cases_are_in_the_class_and_hold_the_regimes_they_claim(th):
    for c in LR.FM_FWD_CASES:
        cls = LR.case_class(c, th)
        assert cls.kernel == c.kernel, (c.name, cls)
        if c.kernel == "vec":
            assert (cls.LPR, cls.SPLIT, cls.fused) == (c.LPR, c.SPLIT, c.cfused), (c.name, cls)
            assert cls.NE == c.E // 4 and cls.lds <= 61440
        else:
            assert (cls.GW, cls.NACC) == (c.GW, c.NACC) == LR.GEN_CLAIMS[c.E], (c.name, cls)
        got = LR.case_regimes(c, th)
        assert got >= c.claims, (c.name, c.claims - got)
        assert c.scale == (0.5 if c.E <= 16 else 0.2)                  # the scale of the existing tests
    assert LR.case_class(LR.FWD_BY_NAME["sep_e4_b10_f240"], th).lds == 61440
    assert LR.case_class(LR.FWD_BY_NAME["gen_e4_b10_f241"], th)[-2:] == (4, 1)


def test_forward_table_holds_the_issue_s_cases():
    have = {(c.B, c.F, c.E, c.ld, c.fused, c.aligned) for c in LR.FM_FWD_CASES}
    for L_ in (1, 2, 4, 8, 16):
        for B, F in ((65536 // L_, 2), (65536 // L_, 5), (32768 // L_, 5), (37, 2), (37, 5), (3, 1)):
            assert (B, F, 4 * L_, 4 * L_, False, True) in have
    assert set(LR.FUSED_ROWS) == {(4, 8), (8, 16), (12, 16), (16, 32), (28, 32), (20, 32), (32, 64), (60, 64)}
    for E, ld in LR.FUSED_ROWS:
        for B, F in ((65536 // (ld // 4), 3), (32768 // (ld // 4), 5), (37, 2), (37, 7)):
            assert (B, F, E, ld, True, True) in have
    for row in ((9, 64, 16, 16, False, True), (9, 70, 16, 16, False, True), (9, 70, 16, 32, True, True),
                (9, 70, 64, 64, False, True), (10, 240, 4, 4, False, True), (10, 241, 4, 4, False, True),
                (8192, 16, 32, 32, False, True)):
        assert row in have, row
    for E, ld, al in ((1, 1, True), (2, 2, True), (3, 3, True), (5, 5, True), (8, 8, False), (12, 12, True),
                      (16, 16, False), (20, 20, True), (36, 36, True), (64, 65, True), (100, 100, True),
                      (128, 128, True), (130, 130, True), (256, 256, True)):
        GW = LR.GEN_CLAIMS[E][0]
        for B in (37, 64):
            assert (B, 3, E, ld, False, al) in have
            assert GW > 16 or any(r[:1] + r[2:] == (B, E, ld, False, al) and r[1] > GW for r in have), (E, B)


def test_union_of_forward_cases_reaches_every_instantiation_and_regime(th):
    assert len(LR.ALL_VEC_KEYS) == 27 and len(LR.ALL_GEN_KEYS) == 9
    reached, with_fields, regimes = set(), set(), {}
    for c in LR.FM_FWD_CASES:
        cls = LR.case_class(c, th)
        key = ("vec", cls.LPR, cls.SPLIT, cls.fused) if cls.kernel == "vec" else ("gen", cls.GW, cls.NACC)
        reached.add(key)
        if c.F > 1:
            with_fields.add(key)
        for reg in LR.case_regimes(c, th):
            regimes.setdefault(reg, set()).add(key)
    assert reached == LR.ALL_VEC_KEYS | LR.ALL_GEN_KEYS, (LR.ALL_VEC_KEYS | LR.ALL_GEN_KEYS) ^ reached
    assert with_fields == reached, reached - with_fields               # each with a case that walks several fields
    count = lambda keys: {k: keys.count(k) for k in set(keys)}         # and each as often as the table claims it
    got = count([k for c in LR.FM_FWD_CASES for k in [LR.case_class(c, th)]
                 for k in [("vec", k.LPR, k.SPLIT, k.fused) if k.kernel == "vec" else ("gen", k.GW, k.NACC)]])
    assert got == count([LR.class_key(c) for c in LR.FM_FWD_CASES]), "cases moved between instantiations"
    assert set(regimes) == set(LR.VEC_REGIMES + LR.FUSED_REGIMES + LR.GEN_REGIMES), regimes.keys()
    split1 = {k for k in LR.ALL_VEC_KEYS if k[2] == 1}
    assert all(any(LR.class_key(c) == k and c.F > 1 for c in LR.FM_FWD_CASES) for k in split1)
    for reg in ("F_not_multiple_of_split", "B_lt_EPW"):                # on every lane width
        assert {k[1] for k in regimes[reg]} >= {1, 2, 4, 8}, reg
    assert {k[1] for k in regimes["last_workgroup_partial"]} == {1, 2, 4, 8, 16}
    fused_keys = {k for k in LR.ALL_VEC_KEYS if k[3]}                  # both kinds of fused row on every fused class
    assert regimes["fused_w_lane_is_last"] == fused_keys               # (a row of two lanes has no idle one)
    assert regimes["fused_idle_lanes"] == {k for k in fused_keys if k[1] >= 4}
    assert any(c.F < c.SPLIT for c in LR.FM_FWD_CASES if c.kernel == "vec")
    assert regimes["E_not_multiple_of_GW"] >= {("gen", 64, 2), ("gen", 64, 4)}
    assert regimes["F_gt_GW"] >= {("gen", g, 1) for g in (1, 2, 4, 8, 16)}
    assert regimes["tail_block"] >= LR.ALL_GEN_KEYS and len({LR.class_key(c) for c in LR.FM_FWD_CASES if c.kernel == "gen"
                                                             and "tail_block" not in LR.case_regimes(c, th)}) >= 7
    # the fused rows of the sharded engine, and what the classes of the same data are when the tables are separate
    assert LR.fm_fwd_class(37, 7, 20, 32, True, True, th)[:5] == ("vec", 8, 4, True, 5)
    assert {LR.fm_fwd_class(37, 7, E, E, False, True, th).kernel for E, _ in LR.FUSED_ROWS} == {"vec", "gen"}


def test_out_of_range_cases_cover_every_instantiation():
    names = LR.oob_cases()
    assert {LR.class_key(LR.FWD_BY_NAME[n]) for n in names} == LR.ALL_VEC_KEYS | LR.ALL_GEN_KEYS
    assert len(names) == 36
    for n in names[:6] + names[-3:]:
        c = LR.FWD_BY_NAME[n]
        X, Xc = LR.fwd_X(n, True), LR.fwd_X(n)
        assert Xc.min() == 0 and Xc.max() == c.V - 1
        assert X[0, 0] == -1 and X[0, 1] == c.V and X[-1, -2] == 2 ** 31 + 5 and X[-1, -1] == 2 ** 32 + 3
        assert int(np.int64(X[-1, -1]).astype(np.int32)) == 3 < c.V    # aliases a row once narrowed to 32 bits
        assert np.sum((X < 0) | (X >= c.V)) == 4
        ref = LR.fwd_reference(n, "int", True)
        assert np.all(ref["rows"][0, :2] == 0) and np.all(ref["rows"][-1, -2:] == 0)


def test_integer_forward_cases_cannot_round():
    for c in LR.FM_FWD_CASES:
        assert LR.int_case_is_exact(c.E, c.F), c.name
        assert 16 * c.E * c.F ** 2 + 32 * (c.F + 1) < 2 ** 24, c.name
        Ke, Kw, kb = LR.int_params(c.V, c.E, c.seed)
        assert max(np.abs(Ke).max(), np.abs(Kw).max(), abs(kb)) <= 4 and Ke.shape == (c.V, c.E)
        p = LR.fwd_params(c.name, "int")
        assert all(a.dtype == np.float32 for a in p.values()) and np.array_equal(p["embed"] * 4, Ke)
    assert not LR.int_case_is_exact(256, 64) and LR.int_case_is_exact(4, 241)


@pytest.mark.parametrize("name", [c.name for c in LR.FM_FWD_CASES if c.B * c.F * c.E <= 40000][::4])
def test_integer_reference_agrees_with_the_fp64_oracle(name):
    for oob in ((False, True) if LR.FWD_BY_NAME[name].F > 1 else (False,)):
        ref, p, X = LR.fwd_reference(name, "int", oob), LR.fwd_params(name, "int"), LR.fwd_X(name, oob)
        ez, Xz = LR.with_zero_row(p["embed"], X)
        wz = LR.with_zero_row(p["w"], X)[0]
        _, z64 = L.fm_forward(ez, wz, p["bias"], Xz, np.float64)
        assert np.array_equal(ref["z"], z64[:, 0]) and np.array_equal(ref["S"], L.fm_terms(ez, wz, Xz, np.float64)[1])
        assert ref["z"].dtype == np.float32 and np.any(ref["z"] != 0)


@pytest.mark.parametrize("name", [c.name for c in LR.FM_FWD_CASES])
def test_normal_forward_bound_has_room(name):
    """an fp32 evaluation in plain field order stays under half of the bound the GPU test uses"""
    ref = LR.fwd_reference(name, "normal")
    bound = LR.fwd_bounds(ref)
    z, S = LR.fwd_fp32_plain(name)
    assert z.dtype == np.float32 and S.dtype == np.float32
    rz, rs = np.abs(z - ref["z"]).max() / bound["z"], np.abs(S - ref["S"]).max() / bound["S"]
    print("%s z %.3f S %.3f of the bound" % (name, rz, rs))
    assert rz <= 0.5 and rs <= 0.5, (name, rz, rs)


def test_sizes_stay_small():
    for c in LR.FM_FWD_CASES:
        assert c.B * c.F <= LR.MAX_IDS == 327680, c.name
        # the one case of SPLIT = 1 with FP = 16 needs B LPR >= 65536 with 16 fields: 4.2 M floats of rows
        assert c.B * c.F * c.E <= (LR.MAX_FLOATS if c.name != "sep_e32_b8192_f16" else 8192 * 16 * 32), c.name
    assert LR.MAX_FLOATS == 1_500_000
    for c in LR.GATHER_CASES:
        assert c.n * c.E <= 600_000 and c.n <= 2051, c.name
    for c in LR.LISTS_CASES:
        assert c.n_lists * c.cap * c.E <= 400_000, c.name
    for c in LR.FM_BWD_CASES:
        assert c.B * c.F * c.E <= 70_000, c.name


# ---- gather, list gather, backward ----------------------------------------------------------------------------------
def test_gather_cases_are_in_the_class_and_regime_they_claim(th):
    reached = {}
    for c in LR.GATHER_CASES:
        cls = LR.gather_class(c.E, c.ld, not c.table_off, not c.out_off, th)
        assert (cls.kernel, cls.LPR) == (c.kernel, c.LPR), (c.name, cls)
        assert LR.gather_regime(c, th) == c.regime, c.name
        reached.setdefault((c.kernel, c.LPR), set()).add((c.regime, c.ld == c.E))
    for lpr in (1, 2, 4, 8, 16, 32, 64):
        assert reached[("rows", lpr)] == {(r, d) for r in LR.ROWS_N_REGIMES for d in (True, False)}, lpr
    assert len(reached) == 9
    for k in ("vec4", "scalar"):
        assert {r for r, _ in reached[(k, None)]} == set(LR.FLAT_N_REGIMES)
    assert {c.E for c in LR.GATHER_CASES if c.kernel == "vec4"} == {12, 20, 100, 260, 512}
    scalar = {(c.E, c.ld, c.table_off, c.out_off) for c in LR.GATHER_CASES if c.kernel == "scalar"}
    assert scalar >= {(1, 1, 0, 0), (3, 3, 0, 0), (7, 7, 0, 0), (33, 33, 0, 0), (16, 17, 0, 0), (16, 16, 4, 0),
                      (16, 16, 0, 4)}
    for c in LR.GATHER_CASES:
        idx = LR.gather_ids(c)
        assert idx.shape == (c.n,) and idx.min() >= 0 and idx.max() == c.V - 1 and (c.n == 1 or idx.min() == 0)
        if c.n >= 8:
            bad = LR.gather_ids(c, True)
            assert sorted(bad[(bad < 0) | (bad >= c.V)].tolist()) == [-1, c.V, 2 ** 31 + 5, 2 ** 32 + 3]
            assert np.all(LR.gather_reference(LR.table_vals(c.V, c.E, 0), bad)[[0, -1]] == 0)


def test_lists_cases_are_in_the_class_they_claim_and_reach_every_lpr(th):
    seen, straddle, counts_seen = set(), set(), set()
    for c in LR.LISTS_CASES:
        cls = LR.lists_class(c.E, c.ld, True, th)
        assert (cls.nc, cls.lpr) == (c.nc, c.lpr) == LR.LISTS_CLAIMS[c.E], c.name
        assert c.ld in (c.E, c.E + 4) and c.ld % 4 == 0 and len(c.counts) == c.n_lists
        seen.add((c.lpr, c.nc == c.lpr, c.ld == c.E))
        n = c.n_lists * c.cap
        rows = (np.arange(0, n, 4 * cls.R)[:, None, None] + np.arange(cls.R)[None, :, None]
                + np.arange(4)[None, None, :] * cls.R).reshape(-1, 4)           # the UNR rows of every thread
        if np.any([len({r // c.cap for r in t if r < n}) > 1 for t in rows]):
            straddle.add((c.lpr, c.cap))
        counts_seen |= {"0" if k == 0 else "1" if k == 1 else "cap" if k == c.cap else "mixed" for k in c.counts}
        msg, used = LR.lists_msg(c), LR.lists_used(c)
        assert msg.shape == (c.n_lists, 2 + c.cap) and np.all(msg[:, 1] == LR.GARBAGE_WORD)
        slots = msg[:, 2:].reshape(-1)
        assert np.all((slots[used] >= 0) & (slots[used] < c.V)) and set(slots[~used].tolist()) <= {-7, c.V + 9}
        assert used.sum() == sum(c.counts)
        if used.any():
            bad = LR.lists_msg(c, True)[:, 2:].reshape(-1)
            assert np.sum((bad[used] < 0) | (bad[used] >= c.V)) == 1
    want = {(l, True, d) for l in th.LISTS_LPRS for d in (True, False)} | {
        (l, False, d) for l in th.LISTS_LPRS if l >= 4 for d in (True, False)}
    assert seen == want, want ^ seen
    assert {l for l, cap in straddle if cap == 7} == {8, 16, 32, 64}         # cap = 7, five lists: R <= 32 < 35 rows
    assert {l for l, _ in straddle} == set(th.LISTS_LPRS)
    assert counts_seen == {"0", "1", "cap", "mixed"}
    assert {c.E for c in LR.LISTS_CASES} >= {4, 8, 12, 16, 20, 32, 36, 64, 128, 132, 256}
    assert {(c.n_lists, c.cap) for c in LR.LISTS_CASES} == {(a, b) for a in (1, 5) for b in (1, 7, 300)}


def test_backward_cases_are_in_the_class_they_claim_and_reach_both():
    reached = set()
    for c in LR.FM_BWD_CASES:
        assert LR.fm_bwd_class(c.E, c.ld, c.rows_given, c.aligned) == c.kernel, c.name
        reached.add((c.kernel, c.rows_given, c.extra, c.ld == c.E, LR.bwd_units(c) % 256 == 0))
    assert reached == {(k, r, x, d, m) for k in ("vec", "scalar") for r in (True, False) for x in (True, False)
                       for d in (True, False) for m in (True, False)}
    assert {(c.E, c.kernel) for c in LR.FM_BWD_CASES} == {(4, "vec"), (12, "vec"), (16, "vec"), (64, "vec"),
                                                           (256, "vec"), (1, "scalar"), (3, "scalar"), (5, "scalar"),
                                                           (16, "scalar")}
    for E in (4, 12, 16, 64, 256, 1, 3, 5):
        assert {LR.bwd_units(c) % 256 == 0 for c in LR.FM_BWD_CASES if c.E == E and c.aligned} == {True, False}, E


@pytest.mark.parametrize("name", [c.name for c in LR.FM_BWD_CASES][::7])
def test_backward_references_agree(name):
    c = LR.BWD_BY_NAME[name]
    for oob in (False, True):
        i = LR.bwd_inputs(c, "int", oob)
        assert all(i[k].dtype == np.float32 for k in ("embed", "gz", "S", "extra", "ref"))
        assert np.abs(i["embed"] * 4).max() <= 4 and np.array_equal(i["embed"] * 4, np.rint(i["embed"] * 4))
        ez, Xz = LR.with_zero_row(i["embed"], i["X"])
        ref = L.fm_backward(ez, Xz, i["gz"].reshape(-1, 1), np.float64)[0] + (i["extra"] if c.extra else 0)
        assert np.array_equal(i["ref"], ref) and np.array_equal(i["S"], ez[Xz].astype(np.float64).sum(1))
        assert np.sum((i["X"] < 0) | (i["X"] >= c.V)) == (2 if oob else 0)
    n = LR.bwd_inputs(c, "normal")
    assert n["ref"].dtype == np.float64 and n["ref"].shape == (c.B * c.F, c.E) and LR.bwd_bound(n["ref"]) >= 2e-6
