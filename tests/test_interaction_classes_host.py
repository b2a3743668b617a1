"""CPU checks behind tests/test_gpu_interaction_classes.py: tests/interaction_classes_ref.py restates the thresholds and the
two LDS byte formulas that are in the text of csrc/interactions.hip today, every case of IPN_CASES, BI_CASES, ATTN_CASES and
FFM_CASES is in the class it claims, their union reaches every class and regime, the references agree with
oracle/layers_np.py, the derived bounds leave room for a correct fp32 evaluation in three summation orders and catch eleven
wrong kernels, the PNN forward and backward accept the same shapes and the FFM forward never asks for more LDS than its
launch path allows.  A failure on the GPU can then not be blamed on the case table or on the bounds.

Where the shapes of tests/test_gpu_f4.py land (the gap this closes; B, F, E or B, T, C, E as listed there):
  ipn   (1,1,4) (3,2,3) (4,5,8) (257,5,16 strided) (1030,26,16 strided) (65,40,32) (9,7,6): EX = 1 in both directions;
        (8192,26,16): forward EX = 4 vec4, backward EX = 2, no partial group.  Never: EX = 8, EX = 2 forward, a partial
        group, scalar at EX > 1, a vec4 fall-back, a single example above 16 KB with more than 64 KB in the backward.
  bi    F in {1, 3, 9, 10, 26}: one or two ragged blocks of 8 (10 and 26 are ragged too); every vec case aligned, no
        out-of-range id.  Never: F % 8 == 0, three blocks with an exact end, a fall-back.
  attn  D = 4, 24, 48, 96, 250 -> NPL 1, 1, 1, 2, 4; T = 1, 7, 100, 33, 20; padding at the tail only.  Never: NPL = 3, D a
        multiple of 64, a padded step in the middle, a padded step with other ids, an out-of-range id, ld_q > D.
  ffm   (1,1,4) (4,3,4) (33,5,16) (700,26,16) (500,10,8 zipf): vec; (65,7,6): scalar, one item pass.  Never: the scalar
        fall-back at E % 4 == 0, ld_v > F*E, ld_w > 1, two item passes, an out-of-range id.
"""
import os
import re

import numpy as np
import pytest

from oracle import layers_np as L
from tests import interaction_classes_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")
K = IR.K


@pytest.fixture(scope="module")
def text():
    with open(os.path.join(CSRC, "interactions.hip")) as f:
        return f.read()


@pytest.fixture(scope="module")
def common():
    with open(os.path.join(CSRC, "common.h")) as f:
        return f.read()


def _one(pattern, text, what, count=1, flags=0):
    found = re.findall(pattern, text, flags)
    assert len(found) == count and len(set(found)) == 1, "interactions.hip: %s found %d times as %s, the tests expect %d " \
        "identical" % (what, len(found), sorted(set(found)), count)
    return found[0]


def _body(text, head):
    body = text[text.index(head):]
    return body[:body.index("\n}\n")]


def _c_expr(expr, **names):
    """a C integer expression of the source, evaluated with Python's integers"""
    expr = expr.replace("(size_t)", "").replace("(int64_t)", "").replace("/", "//")
    assert re.fullmatch(r"[\w\s+\-*/()]+", expr), "not an arithmetic expression: " + expr
    return eval(expr, {"__builtins__": {}}, names)


def _c_lambda(expr, args):
    expr = expr.replace("(size_t)", "").replace("(int64_t)", "").replace("/", "//")
    assert re.fullmatch(r"[\w\s+\-*/()]+", expr), "not an arithmetic expression: " + expr
    return eval("lambda %s: %s" % (args, expr), {"__builtins__": {}})


def _constants(text, common):
    """every ``constexpr int|size_t NAME = <product of numbers>;`` of the two files"""
    out = {}
    for name, val in re.findall(r"constexpr (?:size_t|int) (\w+) = (\d+(?: \* \d+)*);", common + text):
        out[name] = _c_expr(val)
    return out


class Source:
    """what interactions.hip says about the IPN and FFM domains, read from its text"""

    def __init__(self, text, common):
        self.const = _constants(text, common)
        bwd, fwd = _one(r"(?:size_t bytes =|return) bwd \? (.+?)\s*: (.+?);", text, "the two IPN byte formulas",
                        flags=re.S)
        self.formula = {True: _c_lambda(bwd, "EX, F, E, P"), False: _c_lambda(fwd, "EX, F, E, P")}
        self._caps = {}
        group = _body(text, "static int ipn_examples_per_group(")
        self.groups = int(_one(r"while \(EX > 1 && \(B / EX\) < (\d+)\) EX >>= 1;", group, "the grid rule"))
        self.ex_max = int(_one(r"int EX = (\d+);", group, "the largest EX"))
        self.group_lds = _c_expr(_one(r"if \(bytes <= (\d+ \* \d+) \|\| EX == 1\)", group, "the LDS rule"))
        cap = _one(r"return \(bytes <= (.+?)\) \? EX : 0;", group, "the single-example limit")
        both = re.fullmatch(r"\(bwd \? (\w+) : (\w+)\)", cap)
        self.cap_names = {True: both.group(1), False: both.group(2)} if both else {True: cap, False: cap}
        self.common_domain = {}
        for d, head in ((False, 'extern "C" int rec_emb_ipn_fwd_f32('), (True, 'extern "C" int rec_emb_ipn_bwd_vals_f32(')):
            body = _body(text, head)
            self.common_domain[d] = "ipn_shape_ok(B, F, E)" in body
            assert ("ipn_examples_per_group(B, F, E, %s, &lds)" % ("true" if d else "false")) in body
        if any(self.common_domain.values()):
            ok = _body(text, "static bool ipn_shape_ok(")
            assert "ipn_examples_per_group(B, F, E, false, &lds) > 0 && ipn_examples_per_group(B, F, E, true, &lds) > 0" in ok
        self.ipn_max_f = self.name(_one(r"F <= 0 \|\| F > (\w+)\) return REC_E_ARG;", text, "the IPN field limit", 2))
        self.opt_in = re.findall(r"rec_allow_lds<emb_ipn_bwd_kernel>\((\w+)\)", text)

    def name(self, x):
        if x in self.const:
            return self.const[x]
        if x == "IPN_BWD_LDS_MAX":
            return min(self.bwd_need(), self.const["REC_LDS_CU_BYTES"])
        return _c_expr(x)

    def bytes(self, EX, F, E, bwd):
        return self.formula[bwd](EX, F, E, F * (F - 1) // 2)

    def bwd_need(self):
        need = 0
        for F in range(1, self.const["IPN_MAX_F"] + 1):
            fixed = self.bytes(1, F, 0, False)
            if fixed + 4 * F > self.const["IPN_FWD_LDS_MAX"]:
                break
            need = max(need, self.bytes(1, F, (self.const["IPN_FWD_LDS_MAX"] - fixed) // (4 * F), True))
        return need

    def cap(self, bwd):
        if bwd not in self._caps:
            self._caps[bwd] = self.name(self.cap_names[bwd])
        return self._caps[bwd]

    def runs(self, F, E, bwd):
        """a single example of direction ``bwd`` fits its limit"""
        return self.bytes(1, F, E, bwd) <= self.cap(bwd)

    def accepts(self, F, E, bwd):
        if not 1 <= F <= self.ipn_max_f:
            return False
        if self.common_domain[bwd]:
            return self.runs(F, E, False) and self.runs(F, E, True)
        return self.runs(F, E, bwd)


@pytest.fixture(scope="module")
def src(text, common):
    return Source(text, common)


# ---- the restatements are the source's ------------------------------------------------------------------------------
def test_thresholds_are_the_ones_in_the_source(text, common, src):
    got = dict(
        GROUPS=src.groups, GROUP_LDS=src.group_lds, FWD_LDS_MAX=src.cap(False), CU_LDS=src.const["REC_LDS_CU_BYTES"],
        IPN_MAX_F=src.ipn_max_f, EX_MAX=src.ex_max,
        WG=int(_one(r"dim3\(\(unsigned\)ceil_div64\(B, EX\)\), dim3\((\d+)\)", text, "the IPN workgroup", 2)),
        ROW_UNROLL=int(_one(r"i0 \+= (\d+) \* 256\)", text, "the row-load unroll", 3)),
        F_BLOCK=int(_one(r"for \(int f0 = 0; f0 < F; f0 \+= (\d+)\)", text, "the field block")),
        TB=int(_one(r"constexpr int TB = (\d+);", text, "TB")),
        WAVES=int(_one(r"for \(int t0 = wave \* TB; t0 < T; t0 \+= (\d+) \* TB\)", text, "the waves of ip_attn")),
        LANES=int(_one(r"const int npl = \(D \+ 63\) / (\d+);", text, "the lanes of a wave")),
        ATTN_MAX_D=int(_one(r"T <= 0 \|\| D > (\d+) \|\| ld_q < D\)", text, "the D limit")),
        ATTN_LDS_MAX=_c_expr(_one(r"if \(lds > (\d+ \* \d+)\) return REC_E_ARG;", text, "the ip_attn LDS limit")),
        FFM_MAX_F=src.name(_one(r"F <= 0 \|\| F > (\w+) \|\| ld_v < \(int64_t\)F \* E", text, "the FFM field limit", 2)),
        FFM_FWD_STRIDE=int(_one(r"for \(int i = tid; i < P \* EL; i \+= (\d+)\)", text, "the pair loop's stride")),
        FFM_BWD_STRIDE=int(_one(r"for \(int item = threadIdx\.x; item < F \* EL; item \+= (\d+)\)", text, "the item loop")),
        LAUNCH_LDS=_c_expr(_one(r"if \(cap_bytes <= (\d+ \* \d+)\) return hipSuccess;", common, "the opt-in threshold")))
    for field in IR.Consts._fields:
        assert got[field] == getattr(K, field), "the source has %s = %s, interaction_classes_ref.K.%s = %s" % (
            field, got[field], field, getattr(K, field))
    assert src.cap(True) == IR.ipn_bwd_lds_max() == K.CU_LDS
    assert src.opt_in == [src.cap_names[True]], "the backward opts in for another size than its argument check admits"
    for line in (
            "constexpr size_t IPN_BWD_LDS_MAX = ipn_bwd_need() < REC_LDS_CU_BYTES ? ipn_bwd_need() : REC_LDS_CU_BYTES;",
            "const int vec4 = (E & 3) == 0 && (ld & 3) == 0 && rec_is_aligned16(table);",
            "const bool vec = (E & 3) == 0 && (ld & 3) == 0 && rec_is_aligned16(table);",
            "reinterpret_cast<uintptr_t>(vals)) & 15) == 0;",
            "const size_t lds = (size_t)T * C * 4 + (size_t)4 * D * 4;",
            "const bool vec = (E & 3) == 0 && (ld_v & 3) == 0 && rec_is_aligned16(v);",
            "((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(g_rows)) & 15) == 0;",
            "bool pad = id0 == padding_index;", "if (a == c) continue;"):
        assert line in text, "interactions.hip no longer holds: " + line
    # both directions launch ip_attn_kernel<npl, .> through the 1..4 dispatch of common.h: 1, 2, 3 as given, else 4
    launch = _body(text, "static int ip_attn_launch(")
    assert "return rec_dispatch_1to4(npl, [&](auto n) {" in launch
    assert re.findall(r"go\(ip_attn_kernel<decltype\(n\)::value, (false|true)>\);", launch) == ["true", "false"]
    dispatch = _body(common, "static inline int rec_dispatch_1to4(int n, Fn&& f) {")
    assert re.findall(r"case (\d): return f\(std::integral_constant<int, (\d)>\{\}\);", dispatch) == [
        ("1", "1"), ("2", "2"), ("3", "3")]
    assert re.findall(r"default: return f\(std::integral_constant<int, (\d)>\{\}\);", dispatch) == ["4"]


def test_byte_formulas_are_the_ones_in_the_source(src):
    for F in (1, 2, 3, 26, 64, 80, 100, 200, 244, 255):
        for E in (1, 3, 4, 16, 64, 256):
            for EX in (1, 2, 4, 8):
                for bwd in (False, True):
                    assert src.bytes(EX, F, E, bwd) == IR.ipn_lds_bytes(EX, F, E, bwd), (EX, F, E, bwd)


def test_ipn_backward_accepts_exactly_what_the_forward_accepts(src):
    """defect 1: at F = 80, E = 64 the forward needs 28416 bytes and ran, the backward 66880 and was refused"""
    split = [(F, E) for F in range(1, 256) for E in range(1, 257) if src.accepts(F, E, False) != src.accepts(F, E, True)]
    assert not split, "%d shapes that one direction of rec_emb_ipn accepts and the other refuses, the first (F, E) = %s: " \
        "forward %s (%d bytes), backward %s (%d bytes)" % (
            len(split), split[0], src.accepts(*split[0], False), src.bytes(1, *split[0], False),
            src.accepts(*split[0], True), src.bytes(1, *split[0], True))
    for F in range(1, 256):
        for E in range(1, 257):
            assert src.accepts(F, E, False) == IR.ipn_accepts(F, E), (F, E)
            if src.accepts(F, E, True):                   # and what it accepts it can launch
                assert src.bytes(1, F, E, True) <= src.const["REC_LDS_CU_BYTES"]
                assert src.bytes(1, F, E, True) <= K.LAUNCH_LDS or src.opt_in, (F, E)
    assert IR.ipn_accepts(80, 64) and IR.ipn_accepts(100, 32) and IR.ipn_accepts(200, 1)
    assert not IR.ipn_accepts(244, 1) and not IR.ipn_accepts(255, 1)


def test_ffm_forward_never_asks_for_more_lds_than_it_may_launch(text, src):
    """defect 2: F = 255 passed the argument check and asked for 65806 bytes without the opt-in"""
    body = _body(text, 'extern "C" int rec_ffm_fwd_f32(')
    limit = src.name(_one(r"F <= 0 \|\| F > (\w+) \|\| ld_v", body, "the forward's field limit"))
    inline = re.findall(r"const size_t lds = (\(size_t\)F[^;]+);", body)
    formula = inline[0] if inline else _one(r"constexpr size_t ffm_fwd_lds_bytes\(int F\) \{ return ([^;]+); \}", text,
                                            "the FFM byte formula")
    fn = _c_lambda(formula, "F")
    may = src.const["REC_LDS_CU_BYTES"] if "rec_allow_lds<" in body else K.LAUNCH_LDS
    for F in range(1, limit + 1):
        need = fn(F)
        assert need == IR.ffm_fwd_lds_bytes(F)
        assert need <= may, "rec_ffm_fwd_f32 accepts F = %d and asks for %d bytes of LDS; its launch path allows %d" % (
            F, need, may)
    assert IR.ffm_fwd_lds_bytes(limit + 1) > may, "the field limit could be higher"
    bwd = _body(text, 'extern "C" int rec_ffm_bwd_rows_f32(')
    assert src.name(_one(r"F <= 0 \|\| F > (\w+) \|\| ld_v", bwd, "the backward's field limit")) == limit


# ---- membership and coverage -----------------------------------------------------------------------------------------
def test_every_case_is_in_the_class_it_claims():
    for c in IR.IPN_CASES:
        assert c.fwd == IR.ipn_class(c.B, c.F, c.E, c.ld, c.off % 4 == 0) and c.fwd is not None, c.name
        assert c.bwd == IR.ipn_class(c.B, c.F, c.E, c.ld, c.off % 4 == 0, bwd=True) and not c.bwd.vec4, c.name
        tag = re.match(r"ex(\d)_", c.name)
        assert int(tag.group(1)) == c.fwd.EX, c.name
        assert ("partial" in c.name) <= c.fwd.partial_last and ("exact" in c.name) <= (not c.fwd.partial_last), c.name
        assert ("vec" in c.name) <= c.fwd.vec4 and ("scalar" in c.name or "fallback" in c.name) <= (not c.fwd.vec4), c.name
        assert IR.has_oob(IR.ipn_input(c.name)[1], IR.V_IPN) == c.oob, c.name
    for c in IR.BI_CASES:
        assert c.fwd == IR.bi_class(c.B, c.F, c.E, c.ld, c.off == 0), c.name
        assert c.bwd == IR.bi_class(c.B, c.F, c.E, c.ld, c.off == 0, True, c.off_sum == 0, c.off_vals == 0), c.name
        assert c.name.startswith("vec") <= (c.fwd.vec and c.bwd.vec), c.name
        assert (c.name.startswith("scalar") or c.name.startswith("fallback")) <= (not c.fwd.vec and not c.bwd.vec), c.name
        assert c.name.startswith("bwd_fallback") <= (c.fwd.vec and not c.bwd.vec), c.name
        assert IR.has_oob(IR.bi_input(c.name)[1], IR.V_BI) == c.oob, c.name
    for c in IR.ATTN_CASES:
        assert c.cls == IR.ip_attn_class(c.C, c.E, c.T) and c.cls is not None, c.name
        assert c.name.startswith("d%d_t%d" % (c.C * c.E, c.T)), c.name
        assert min(c.ld_q, c.ld_p, c.ld_gp) >= c.C * c.E and c.ld >= c.E
        assert IR.has_oob(IR.attn_input(c.name)[1], IR.V_ATTN) == c.oob, c.name
    for c in IR.FFM_CASES:
        assert c.fwd == IR.ffm_class(c.F, c.E, c.ld_v, c.off == 0) and c.fwd is not None, c.name
        assert c.bwd == IR.ffm_class(c.F, c.E, c.ld_v, c.off == 0, True, c.off_rows == 0), c.name
        assert ("vec" in c.name) <= c.fwd.vec and ("scalar" in c.name or c.name.startswith("fallback")) <= (not c.fwd.vec)
        assert IR.has_oob(IR.ffm_input(c.name)[3], IR.V_FFM) == c.oob, c.name


def test_the_tables_reach_every_class_and_regime():
    want = {(EX, v, p) for EX in (1, 2, 4, 8) for v in (False, True) for p in (False, True) if EX > 1 or not p}
    assert {(c.fwd.EX, c.fwd.vec4, c.fwd.partial_last) for c in IR.IPN_CASES} == want
    assert {(c.bwd.EX, c.bwd.partial_last) for c in IR.IPN_CASES} == {(e, p) for e, v, p in want if not v}
    ipn = {c.name: c for c in IR.IPN_CASES}
    assert {(c.B, c.F, c.E) for c in IR.IPN_CASES} >= {(8195, 3, 4), (8195, 3, 3), (8192, 3, 4), (8195, 26, 16)}
    assert {c.B for c in IR.IPN_CASES} >= {4097, 2049}
    c = ipn["ex4_lds_bwd_ex2"]                             # EX = 4 by the LDS rule, the backward at EX = 2
    assert c.B // 8 >= K.GROUPS and IR.ipn_lds_bytes(8, c.F, c.E, False) > K.GROUP_LDS and (c.fwd.EX, c.bwd.EX) == (4, 2)
    c = ipn["ex4_grid_vec_partial"]                        # EX = 4 by the grid rule
    assert c.B // 8 < K.GROUPS <= c.B // 4 and IR.ipn_lds_bytes(8, c.F, c.E, False) <= K.GROUP_LDS
    for name in ("ex1_over16k_vec", "ex1_over16k_scalar"):  # EX = 1 although a few examples would fit the grid rule
        c = ipn[name]
        assert K.GROUP_LDS < IR.ipn_lds_bytes(1, c.F, c.E, False) <= K.FWD_LDS_MAX
    over = [c for c in IR.IPN_CASES if IR.ipn_lds_bytes(1, c.F, c.E, True) > K.LAUNCH_LDS]
    assert {(c.F, c.E) for c in over} >= {(80, 64), (100, 32)} and max(
        IR.ipn_lds_bytes(1, c.F, c.E, True) for c in over) > 0.99 * K.CU_LDS
    fall = [c for c in IR.IPN_CASES if c.E % 4 == 0 and not c.fwd.vec4]
    assert {("ld" if c.ld % 4 else "") + ("align" if c.off else "") for c in fall} == {"ld", "align"}
    assert {("ld" if c.ld % 4 else "") + ("align" if c.off else "") for c in fall if c.fwd.EX > 1} == {"ld", "align"}
    rp = {(d, min(IR.ipn_row_passes(c.bwd if d else c.fwd, c.F, c.E, d), 2)) for c in IR.IPN_CASES for d in (False, True)}
    assert rp == {(False, 1), (False, 2), (True, 1), (True, 2)}
    W = [c.F * c.E + c.F * (c.F - 1) // 2 for c in IR.IPN_CASES]
    assert min(W) <= K.WG < max(W) and {1, 2} <= {c.F for c in IR.IPN_CASES}
    assert {c.oob for c in IR.IPN_CASES if c.fwd.EX > 1} == {True, False}
    for c in IR.IPN_CASES:
        if c.oob:                                          # the first and the last example of a group, and the last of all
            bad = np.nonzero(((IR.ipn_input(c.name)[1] < 0) | (IR.ipn_input(c.name)[1] >= IR.V_IPN)).any(1))[0]
            assert set(bad) >= {0, min(c.fwd.EX, c.B) - 1, c.B - 1}, c.name
    # bi
    for vec in (False, True):
        assert {c.F for c in IR.BI_CASES if c.fwd.vec == vec and not c.off} >= {1, 7, 8, 9, 16, 17}
        assert {c.bwd.vec for c in IR.BI_CASES} == {False, True}
        assert {c.oob for c in IR.BI_CASES if c.fwd.vec == vec} == {False, True}
    assert {(c.fwd.groups > 1, c.fwd.grid_tail) for c in IR.BI_CASES} >= {(True, True), (False, False), (False, True)}
    assert {(c.off, c.off_sum, c.off_vals) for c in IR.BI_CASES} == {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)}
    assert any(c.E % 4 == 0 and c.ld % 4 and not c.off for c in IR.BI_CASES)
    # attn
    assert {c.cls.NPL for c in IR.ATTN_CASES} == {1, 2, 3, 4}                       # each runs forward and backward
    assert {c.C * c.E for c in IR.ATTN_CASES} == {4, 63, 64, 65, 128, 130, 192, 250, 256}
    assert {c.T for c in IR.ATTN_CASES} == {1, 8, 9, 32, 33, 65}
    assert {(c.cls.NPL, c.cls.lane_tail) for c in IR.ATTN_CASES} == {(1, True), (1, False), (2, True), (2, False),
                                                                     (3, True), (3, False), (4, True), (4, False)}
    assert {p for c in IR.ATTN_CASES for p in IR.attn_patterns(c)} == set(IR.ATTN_PATTERNS)
    assert {c.oob for c in IR.ATTN_CASES} == {False, True}
    assert any(c.ld > c.E and c.ld_q > c.C * c.E and c.ld_p > c.C * c.E and c.ld_gp > c.C * c.E for c in IR.ATTN_CASES)
    for c in IR.ATTN_CASES:                                                         # the patterns are what they say
        s = IR.attn_input(c.name)[1]
        for b, p in enumerate(IR.attn_patterns(c)):
            pad, T = s[b, :, 0] == IR.PAD, c.T
            if p == "none":
                assert not pad.any()
            if p == "all":
                assert pad.all()
            if p == "middle" and T > 2:
                assert pad[T // 2] and not pad[T - 1] and not pad[1 if T // 2 != 1 else 2]
            if p == "pad_live_channels" and T > 1:
                assert pad[T // 2] and (s[b, T // 2, 1:] != IR.PAD).all() and not IR.has_oob(s[b], IR.V_ATTN)
                assert not pad[T - 1] and (s[b, T - 1, 1:] == IR.PAD).all()
            if p == "pad_oob_channels":
                assert pad[T // 2] and IR.has_oob(s[b, T // 2, 1:], IR.V_ATTN)
            if p == "oob_valid_step":
                assert IR.has_oob(s[b][~pad], IR.V_ATTN)
    # ffm
    assert {c.F for c in IR.FFM_CASES} >= {1, 2, 26, 40}
    assert {c.fwd.vec for c in IR.FFM_CASES} == {c.bwd.vec for c in IR.FFM_CASES} == {False, True}
    fall = [c for c in IR.FFM_CASES if c.E % 4 == 0 and not c.bwd.vec]
    assert {(c.off, c.ld_v % 4 != 0, c.off_rows) for c in fall} == {(1, False, 0), (0, True, 0), (0, False, 1)}
    assert any(c.ld_v > c.F * c.E and c.ld_w == 16 for c in IR.FFM_CASES)
    assert max(c.fwd.pair_passes for c in IR.FFM_CASES) > 1 and max(c.bwd.item_passes for c in IR.FFM_CASES) > 1
    assert any(c.fwd.pair_passes > 1 and (c.F * (c.F - 1) // 2 * (c.E // 4 if c.fwd.vec else c.E)) % K.FFM_FWD_STRIDE
               for c in IR.FFM_CASES)
    assert {c.oob for c in IR.FFM_CASES} == {False, True}
    z = [c for c in IR.FFM_CASES if c.zipf]
    assert z and np.diff(IR.ffm_reference(z[0].name)[1][1][:5].astype(np.int64)).max() > 500      # a long segment
    for c in IR.FFM_CASES:
        X = IR.ffm_input(c.name)[3]
        assert c.F == 1 or (X[1, 0] == X[1, c.F - 1] and (X[2] == X[2, 0]).all()), c.name


def test_the_refusals_the_gpu_module_tries_are_refusals():
    assert IR.ip_attn_class(1, 257, 4) is None and IR.ip_attn_class(4, 64, 33) is not None
    assert IR.ip_attn_class(4, 64, 3841) is None and IR.ip_attn_class(4, 64, 3840) is not None       # T*C*4 + 16 D
    assert IR.ffm_class(256, 4, 1024) is None and IR.ffm_class(255, 4, 1020) is None and IR.ffm_class(254, 4, 1016)
    assert IR.ipn_class(4, 256, 1, 1) is None and IR.ipn_class(4, 244, 1, 1) is None and IR.ipn_class(4, 10, 8, 7) is None


# ---- the references -------------------------------------------------------------------------------------------------
def test_references_agree_with_the_oracle_on_in_range_ids():
    r = np.random.default_rng(5)
    V, B, F, E = 50, 9, 5, 6
    tab, X = IR.values(r, (V, E)), r.integers(0, V, size=(B, F))
    g = IR.values(r, (B, F * E + F * (F - 1) // 2))
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-14)
    assert close(IR.ref_ipn_fwd(tab, X).out, L.ipn_forward(tab, X, np.float64))
    assert close(IR.ref_ipn_bwd(tab, X, g).vals, L.ipn_backward_vals(tab, X, g, np.float64))
    assert close(IR.ref_bi_fwd(tab, X).out, L.bi_interaction_forward(tab, X, np.float64))
    assert close(IR.ref_bi_bwd(tab, X, g[:, :E]).vals, L.bi_interaction_backward_vals(tab, X, g[:, :E], np.float64))
    T, C = 7, 3
    s = r.integers(1, V, size=(B, T, C))
    s[0, 3:] = 0
    s[1, 2, 0] = 0
    q, gp = IR.values(r, (B, C * E)), IR.values(r, (B, C * E))
    f = IR.ref_attn_fwd(tab, q, s, 0)
    so, po = L.ip_attention_forward(tab, q, s, 0, np.float64)
    assert close(f.scores, so) and close(f.pooled, po)
    b = IR.ref_attn_bwd(tab, q, s, 0, so, gp)
    gk, gq = L.ip_attention_backward(tab, q, s, gp, 0, np.float64)
    assert close(b.gkeys, gk) and close(b.gq, gq)
    v, w, bias, gz = IR.values(r, (V, F, E)), IR.values(r, (V, 1)), np.array([0.3], np.float32), IR.values(r, (B, 1))
    p, z = L.ffm_forward(v, w, bias, X, np.float64)
    f = IR.ref_ffm_fwd(v, w[:, 0], bias, X)
    assert close(f.z, z[:, 0]) and close(f.prob, p[:, 0])
    rows, _, _ = L.ffm_backward(v, X, gz, np.float64)
    uid, want = L.dedup_indexed_slices(X.reshape(-1), rows.reshape(B * F, F * E), "sorted")
    plan = IR.host_plan(X)
    got = IR.ref_ffm_bwd(v, X, gz[:, 0], plan).vals
    assert plan[2] == len(uid) and close(got[:len(uid)].reshape(len(uid), -1), want) and not got[len(uid):].any()


# ---- the bounds: room for a correct fp32 evaluation, none for a wrong one ------------------------------------------------
ROOM = 0.75      # the worst share of a bound a correct evaluation used here was 0.57 (ipn pairs at E = 4: gamma(4) + 1 ulp)


def _ipn(name, order="kernel", mut=None):
    c, (table, X, g), (f, b) = IR.BY_NAME["ipn", name], IR.ipn_input(name), IR.ipn_reference(name)
    return max(IR.ratio(IR.f32_ipn_fwd(table, X, order, c.fwd.vec4, c.fwd.EX, mut), f.out, f.bound),
               IR.ratio(IR.f32_ipn_bwd(table, X, g, order, c.bwd.EX, mut), b.vals, b.bound))


def _bi(name, order="kernel", mut=None):
    (table, X, g), f = IR.bi_input(name), IR.bi_reference(name)
    out, S = IR.f32_bi_fwd(table, X, order, mut)
    ok_out, ok_S = IR.f32_bi_fwd(table, X, order)
    b = IR.ref_bi_bwd(table, X, g, ok_S)
    return max(IR.ratio(out, f.out, f.bout), IR.ratio(S, f.S, f.bS),
               IR.ratio(IR.f32_bi_bwd(table, X, g, ok_S, mut), b.vals, b.bound))


def _attn(name, order="kernel", mut=None):
    (table, s, q, gp), f = IR.attn_input(name), IR.attn_reference(name)
    sc, po = IR.f32_attn_fwd(table, q, s, IR.PAD, order, mut)
    given = IR.f32_attn_fwd(table, q, s, IR.PAD, order)[0]
    given[~f.valid] = np.nan                                # the score of a padded step is never read
    b = IR.ref_attn_bwd(table, q, s, IR.PAD, given, gp)
    gk, gq = IR.f32_attn_bwd(table, q, s, IR.PAD, given, gp, order, mut)
    return max(IR.ratio(sc, f.scores, f.bs), IR.ratio(po, f.pooled, f.bp), IR.ratio(gk, b.gkeys, b.bgk),
               IR.ratio(gq, b.gq, b.bgq))


def _ffm(name, order="kernel", mut=None):
    c, (v, w, bias, X, gz), (f, plan, b) = IR.BY_NAME["ffm", name], IR.ffm_input(name), IR.ffm_reference(name)
    return max(IR.ratio(IR.f32_ffm_fwd(v, w, bias, X, order, c.fwd.vec, mut), f.z, f.bz),
               IR.ratio(IR.f32_ffm_bwd(v, X, gz, plan, order, mut), b.vals, b.bound))


RUN = {"ipn": _ipn, "bi": _bi, "attn": _attn, "ffm": _ffm}


@pytest.mark.parametrize("table,name", sorted(IR.BY_NAME))
def test_a_correct_fp32_evaluation_stays_inside_the_bounds(table, name):
    for order in IR.ORDERS:
        q = RUN[table](name, order)
        assert q <= ROOM, (table, name, order, q)


CATCH = [("pair_off_by_one", "ipn", "ex1_scalar"), ("pair_transposed", "ipn", "ex1_scalar"),
         ("partial_example_dropped", "ipn", "ex8_vec_partial"), ("partial_example_dropped", "ipn", "ex2_scalar_partial"),
         ("ragged_field_dropped", "bi", "vec_f9"), ("ragged_field_dropped", "bi", "scalar_f17"),
         ("diag_not_zero", "ipn", "ex1_scalar"), ("diag_not_zero", "ipn", "ex4_grid_vec_partial"),
         ("valid_any_channel", "attn", "d63_t8"), ("wave_partial_dropped", "attn", "d128_t33"),
         ("oob_row0", "ipn", "ex8_vec_partial"), ("oob_row0", "bi", "vec_f1"), ("oob_row0", "attn", "d65_t32"),
         ("oob_row0", "ffm", "f26_vec"), ("ffm_own_field", "ffm", "f2_vec"), ("ffm_own_field", "ffm", "f26_scalar"),
         ("ffm_diag_kept", "ffm", "f2_vec"), ("ffm_diag_kept", "ffm", "zipf_long"),
         ("segment_last_dropped", "ffm", "f7_scalar"), ("segment_last_dropped", "ffm", "zipf_long")]


@pytest.mark.parametrize("mut,table,name", CATCH)
def test_a_wrong_kernel_leaves_the_bounds(mut, table, name):
    assert RUN[table](name, "kernel", mut) > 10, (mut, table, name)


def test_every_mutant_is_tried():
    assert {m for m, _, _ in CATCH} == set(IR.MUTANTS)
