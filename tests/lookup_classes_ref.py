"""The kernel classes of the embedding lookups (csrc/embedding.hip: rec_emb_gather_f32, rec_emb_gather_lists_f32,
rec_emb_fm_fwd_f32, rec_emb_fm_bwd_vals_f32) restated for the tests, the tables of cases that reach every one of them,
and the references the GPU tests compare with.  No GPU and no package import here: numpy alone.

TH holds every threshold the four dispatchers read; each class function takes a ``th`` so that
tests/test_lookup_classes_host.py can run the case tables against the thresholds it parses out of the source text.

gather_class()   vec4_ok = E % 4 == 0 and ld % 4 == 0 and 16-byte aligned, asked of the table (E, ld) and of the output
                 (E, E).  Both and E a power of two in 4..256: gather_rows_kernel<LPR = E/4, UNR>, R = 256 / LPR rows a
                 pass, R UNR rows a workgroup.  Both: gather_vec4_kernel.  Else gather_scalar_kernel.
lists_class()    None (REC_E_UNSUPPORTED) unless vec4_ok and 4 <= E <= 256; nc = E/4 16-byte pieces a row, lpr = the
                 next power of two >= nc lanes a row, a header of HDR int64 words before the cap slots of a list.
fm_fwd_class()   fused when w == embed + E, ld_w == ld_e, ld_e > E, ld_e a power of two <= 64: LPR = ld_e/4, NE = E/4.
                 Else separate when E is a power of two <= 64: LPR = NE = E/4.  split_of() is the split loop; a class
                 whose id staging 4 (256 // (LPR split)) F exceeds LDS_LIMIT is refused -- a refused fused class tries
                 the separate one, a refused separate class goes to emb_fm_fwd_gen_kernel<GW, NACC> (GEN_LADDER).
fm_bwd_class()   vec when E % 4 == 0, sumvec / dvals / rows / extra are aligned and rows are given or the table is
                 vec4_ok; else scalar.
fm_fwd_regimes() names what a forward case holds of the edges inside a kernel (the docstring there).

Two kinds of values: int_*() -- multiples of 1/4 in [-1, 1], so small that every sum the kernels form, in every order
and with or without fused multiply-adds, is exact in fp32 (int_case_is_exact states the condition) and an int64
evaluation in units of 1/32 is the answer bit for bit; normal_*() -- helpers.deepfm_params, compared with the fp64
oracle.layers_np under the suite's own bounds.  An id outside [0, V) stands for a zero row and a zero w.
"""
import collections
import functools

import numpy as np

from tests import helpers as H_

Thresholds = collections.namedtuple(
    "Thresholds", "UNR NL LDS_LIMIT FILL MAX_SPLIT WAVE MAX_FUSED_LD MAX_VEC_E MAX_E HDR ROWS_LPRS LISTS_LPRS FWD_LPRS "
                  "GEN_LADDER")
TH = Thresholds(
    UNR=4,                      # rows in flight per thread of gather_rows_kernel / gather_lists_kernel
    NL=16,                      # row loads in flight per lane of emb_fm_fwd_vec_kernel
    LDS_LIMIT=60 * 1024,        # bytes of id staging a vec class may ask for
    FILL=1024 * 64,             # lanes (B LPR split) from which the split loop stops splitting for occupancy
    MAX_SPLIT=4, WAVE=64,       # lane groups per example; LPR split stays inside one wave
    MAX_FUSED_LD=64,            # widest fused row (floats)
    MAX_VEC_E=64,               # widest separate-table row of the vec kernel
    MAX_E=256,                  # widest row of gather_rows / gather_lists / the FM forward
    HDR=2,                      # int64 words in front of a list's slots
    ROWS_LPRS=(1, 2, 4, 8, 16, 32, 64), LISTS_LPRS=(1, 2, 4, 8, 16, 32, 64), FWD_LPRS=(1, 2, 4, 8, 16),
    GEN_LADDER=((1, 1, 1), (2, 2, 1), (4, 4, 1), (8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2),
                (256, 64, 4)))                                # (largest E, GW, NACC)
MAX_FLOATS, MAX_IDS = 1_500_000, 65536 * 5                    # no case above these (output floats, ids)
V_DEFAULT = 997
OOB_IDS = (-1, None, (1 << 31) + 5, (1 << 32) + 3)            # None: V itself; the last aliases row 3 once narrowed

GatherClass = collections.namedtuple("GatherClass", "kernel LPR R rows_per_wg")
ListsClass = collections.namedtuple("ListsClass", "nc lpr R rows_per_wg hdr")
FwdClass = collections.namedtuple("FwdClass", "kernel LPR SPLIT fused NE EPW FP lds GW NACC")


def is_pow2(x):
    return x >= 1 and x & (x - 1) == 0


def vec4_ok(E, ld, aligned):
    return E % 4 == 0 and ld % 4 == 0 and bool(aligned)


def _switch(lpr, listed):
    """a ``switch (lpr)`` whose last entry is the ``default:``"""
    return lpr if lpr in listed[:-1] else listed[-1]


def gather_class(E, ld, table_aligned=True, out_aligned=True, th=TH):
    if E < 1 or ld < E:
        raise ValueError("rec_emb_gather_f32 takes E >= 1 and ld >= E")
    both = vec4_ok(E, ld, table_aligned) and vec4_ok(E, E, out_aligned)
    if both and is_pow2(E) and 4 <= E <= th.MAX_E:
        L = _switch(E // 4, th.ROWS_LPRS)
        return GatherClass("rows", L, 256 // L, (256 // (E // 4)) * th.UNR)
    return GatherClass("vec4" if both else "scalar", None, None, None)


def lists_class(E, ld, aligned=True, th=TH):
    if E < 1 or ld < E:
        raise ValueError("rec_emb_gather_lists_f32 takes E >= 1 and ld >= E")
    if not (vec4_ok(E, ld, aligned) and 4 <= E <= th.MAX_E):
        return None
    nc, lpr = E // 4, 1
    while lpr < nc:
        lpr *= 2
    L = _switch(lpr, th.LISTS_LPRS)
    return ListsClass(nc, L, 256 // L, (256 // lpr) * th.UNR, th.HDR)


def split_of(B, F, LPR, th=TH):
    split = 1
    while (split < th.MAX_SPLIT and LPR * split * 2 <= th.WAVE and -(-F // split) > 1
           and (-(-F // split) > th.NL or B * LPR * split < th.FILL)):
        split *= 2
    return split


def _vec_class(B, F, LPR, NE, fused, th):
    if LPR not in th.FWD_LPRS:
        return None
    split = split_of(B, F, LPR, th)
    EPW = 256 // (LPR * split)
    lds = 4 * EPW * F
    if lds > th.LDS_LIMIT:
        return None
    return FwdClass("vec", LPR, split, fused, NE, EPW, -(-F // split), lds, None, None)


def fm_fwd_class(B, F, E, ld_e, w_is_fused=False, aligned=True, th=TH):
    """``w_is_fused``: w is float E of the embed rows (w == embed + E and ld_w == ld_e); ``aligned``: the embed table is
    16-byte aligned (rows and sumvec always are, here)"""
    if E < 1 or E > th.MAX_E or ld_e < E or F < 1 or B < 1 or (w_is_fused and ld_e <= E):
        raise ValueError("rec_emb_fm_fwd_f32 takes 1 <= E <= %d, ld_e >= E, F >= 1" % th.MAX_E)
    if vec4_ok(E, ld_e, aligned):
        if w_is_fused and ld_e > E and is_pow2(ld_e) and ld_e <= th.MAX_FUSED_LD:
            c = _vec_class(B, F, ld_e // 4, E // 4, True, th)
            if c:
                return c
        if is_pow2(E) and E <= th.MAX_VEC_E:
            c = _vec_class(B, F, E // 4, E // 4, False, th)
            if c:
                return c
    GW, NACC = next((g, a) for top, g, a in th.GEN_LADDER if E <= top)
    return FwdClass("gen", None, None, None, None, None, None, 0, GW, NACC)


def fm_bwd_class(E, ld_e, rows_given, aligned=True):
    """``aligned``: sumvec, dvals, rows, extra and the table, all 16-byte aligned or all 4 bytes past it"""
    if E < 1 or ld_e < E:
        raise ValueError("rec_emb_fm_bwd_vals_f32 takes E >= 1 and ld_e >= E")
    return "vec" if E % 4 == 0 and aligned and (rows_given or vec4_ok(E, ld_e, aligned)) else "scalar"


VEC_REGIMES = ("F_lt_split", "F_not_multiple_of_split", "FP_eq_16", "FP_gt_16", "B_lt_EPW", "B_multiple_of_EPW",
               "last_workgroup_partial", "lds_eq_limit")
FUSED_REGIMES = ("fused_idle_lanes", "fused_w_lane_is_last")
GEN_REGIMES = ("E_lt_GW", "E_eq_GW", "E_not_multiple_of_GW", "F_gt_GW", "F_lt_GW", "tail_block")


def fm_fwd_regimes(B, F, E, ld_e, w_is_fused=False, aligned=True, th=TH):
    """What a forward case holds.  Vec classes (FP = ceil(F / SPLIT) fields per lane group, EPW examples a workgroup):
      F_lt_split              a lane group is left without a field (s FP >= F for some s < SPLIT)
      F_not_multiple_of_split the last lane group with fields has fewer than FP
      FP_eq_16 / FP_gt_16     one full round of the NL-loads-in-flight loop / a second round
      B_lt_EPW, B_multiple_of_EPW, last_workgroup_partial
      lds_eq_limit            the id staging is exactly LDS_LIMIT bytes
      fused_idle_lanes        NE < LPR - 1: lanes behind the w lane load nothing
      fused_w_lane_is_last    NE == LPR - 1
    gen classes: E_lt_GW, E_eq_GW, E_not_multiple_of_GW (NACC > 1: the last accumulator is partly masked), F_gt_GW /
    F_lt_GW (the first-order loads wrap round the lanes / leave lanes idle), tail_block (B GW % 256 != 0)."""
    c = fm_fwd_class(B, F, E, ld_e, w_is_fused, aligned, th)
    out = set()
    if c.kernel == "vec":
        if any(s * c.FP >= F for s in range(c.SPLIT)):
            out.add("F_lt_split")
        if F % c.SPLIT:
            out.add("F_not_multiple_of_split")
        if c.FP == th.NL:
            out.add("FP_eq_16")
        if c.FP > th.NL:
            out.add("FP_gt_16")
        out.add("B_lt_EPW" if B < c.EPW else "B_multiple_of_EPW" if B % c.EPW == 0 else "last_workgroup_partial")
        if c.lds == th.LDS_LIMIT:
            out.add("lds_eq_limit")
        if c.fused:
            out.add("fused_idle_lanes" if c.NE < c.LPR - 1 else "fused_w_lane_is_last")
    else:
        if c.NACC == 1:
            out.add("E_lt_GW" if E < c.GW else "E_eq_GW")
        elif E % c.GW:
            out.add("E_not_multiple_of_GW")
        if F > c.GW:
            out.add("F_gt_GW")
        if F < c.GW:
            out.add("F_lt_GW")
        if B * c.GW % 256:
            out.add("tail_block")
    return out


# ---- the forward table ----------------------------------------------------------------------------------------------
FwdCase = collections.namedtuple("FwdCase", "name B F E ld fused aligned V scale seed kernel LPR SPLIT cfused GW NACC claims")
# written out, not computed by fm_fwd_class: E -> (GW, NACC) of the generic kernel
GEN_CLAIMS = {1: (1, 1), 2: (2, 1), 3: (4, 1), 4: (4, 1), 5: (8, 1), 8: (8, 1), 12: (16, 1), 16: (16, 1), 20: (32, 1),
              36: (64, 1), 64: (64, 1), 100: (64, 2), 128: (64, 2), 130: (64, 4), 256: (64, 4)}
FUSED_ROWS = ((4, 8), (8, 16), (12, 16), (16, 32), (28, 32), (20, 32), (32, 64), (60, 64))     # (E, ld)


def _fwd_cases():
    out = []

    def add(prefix, B, F, E, ld=None, fused=False, aligned=True, vec=None, claims=()):
        """vec = (LPR, SPLIT, class is fused) as the table claims it, None: the generic kernel by GEN_CLAIMS"""
        ld = E if ld is None else ld
        name = "%s_e%d%s%s_b%d_f%d" % (prefix, E, "ld%d" % ld if ld != E else "", "" if aligned else "mis", B, F)
        LPR, SPLIT, cfused = vec if vec else (None, None, None)
        GW, NACC = (None, None) if vec else GEN_CLAIMS[E]
        out.append(FwdCase(name, B, F, E, ld, fused, aligned, V_DEFAULT, 0.5 if E <= 16 else 0.2, len(out),
                           "vec" if vec else "gen", LPR, SPLIT, cfused, GW, NACC, frozenset(claims)))

    for L in (1, 2, 4, 8, 16):                                 # separate tables, E = 4 L
        for B, F, split in ((65536 // L, 2, 1), (65536 // L, 5, 1), (32768 // L, 5, 2), (37, 2, 2), (37, 5, 4),
                            (3, 1, 1)):
            add("sep", B, F, 4 * L, vec=(L, split, False))
    for E, ld in FUSED_ROWS:                                   # storage[V, ld]: embed = [:, :E], w = [:, E]
        L = ld // 4
        for B, F, split in ((65536 // L, 3, 1), (32768 // L, 5, 2), (37, 2, 2), (37, 7, 4)):
            add("fus", B, F, E, ld, fused=True, vec=(L, split, True),
                claims=("fused_w_lane_is_last" if E // 4 == L - 1 else "fused_idle_lanes",))
    add("sep", 9, 64, 16, vec=(4, 4, False), claims=("FP_eq_16",))
    add("sep", 9, 70, 16, vec=(4, 4, False), claims=("FP_gt_16", "F_not_multiple_of_split"))
    add("fus", 9, 70, 16, 32, fused=True, vec=(8, 4, True), claims=("FP_gt_16", "fused_idle_lanes"))
    add("sep", 9, 70, 64, vec=(16, 4, False), claims=("FP_gt_16", "last_workgroup_partial"))
    add("sep", 10, 240, 4, vec=(1, 4, False), claims=("lds_eq_limit", "FP_gt_16", "B_lt_EPW"))
    add("gen", 10, 241, 4, claims=("E_eq_GW", "F_gt_GW"))      # the staging limit refuses vec <1, 4>
    add("sep", 8192, 16, 32, vec=(8, 1, False), claims=("FP_eq_16", "B_multiple_of_EPW"))
    add("sep", 37, 3, 16, vec=(4, 4, False), claims=("F_lt_split",))          # F < SPLIT itself
    add("sep", 300, 5, 4, vec=(1, 4, False), claims=("last_workgroup_partial",))      # on the narrowest row too
    add("sep", 9, 5, 64, 128, fused=True, vec=(16, 4, False))  # a fused row too wide for the fused class
    gen = ((1, 1, True), (2, 2, True), (3, 3, True), (5, 5, True), (8, 8, False), (12, 12, True), (16, 16, False),
           (20, 20, True), (36, 36, True), (64, 65, True), (100, 100, True), (128, 128, True), (130, 130, True),
           (256, 256, True))
    for E, ld, aligned in gen:
        GW = GEN_CLAIMS[E][0]
        for F in (3, GW + 3) if GW <= 16 else (3,):
            for B in (37, 64):
                add("gen", B, F, E, ld, aligned=aligned)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


FM_FWD_CASES = _fwd_cases()
FWD_BY_NAME = {c.name: c for c in FM_FWD_CASES}


def case_class(c, th=TH):
    return fm_fwd_class(c.B, c.F, c.E, c.ld, c.fused, c.aligned, th)


def case_regimes(c, th=TH):
    return fm_fwd_regimes(c.B, c.F, c.E, c.ld, c.fused, c.aligned, th)


def class_key(c):
    """the template instantiation a case claims"""
    return ("vec", c.LPR, c.SPLIT, c.cfused) if c.kernel == "vec" else ("gen", c.GW, c.NACC)


ALL_VEC_KEYS = frozenset(("vec", L, s, f) for L in (1, 2, 4, 8, 16) for s in (1, 2, 4) for f in (False, True)
                         if not (f and L == 1))
ALL_GEN_KEYS = frozenset(("gen", g, a) for _, g, a in TH.GEN_LADDER)


def oob_cases():
    """one case per instantiation for the out-of-range ids: the one with the fewest ids among those with F > 1"""
    best = {}
    for c in FM_FWD_CASES:
        k = class_key(c)
        if c.F > 1 and (k not in best or c.B * c.F < best[k].B * best[k].F):
            best[k] = c
    return [c.name for c in FM_FWD_CASES if best.get(class_key(c)) is c]


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=4)
def fwd_X(name, oob=False):
    """int64 [B, F] ids of [0, V), 0 and V - 1 among them.  ``oob``: example 0 starts with -1 and V, the last example
    ends with 2^31 + 5 and, in its last field (the last field of the last lane group that has one), 2^32 + 3."""
    c = FWD_BY_NAME[name]
    X = H_.rng(1000 + c.seed).integers(0, c.V, size=(c.B, c.F), dtype=np.int64)
    X[0, 0], X[-1, -1] = 0, c.V - 1
    if oob:
        assert c.F >= 2 and c.B >= 2 and c.V > 5
        X[0, 0], X[0, 1], X[-1, -2], X[-1, -1] = -1, c.V, (1 << 31) + 5, (1 << 32) + 3
    _freeze(X)
    return X


def quarters(r, shape):
    """int64 k in [-4, 4]: the value is k / 4"""
    return r.integers(-4, 5, size=shape, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def int_params(V, E, seed):
    """(K_embed [V, E], K_w [V], k_bias) int64 quarters"""
    r = H_.rng(2000 + seed)
    out = quarters(r, (V, E)), quarters(r, (V,)), int(quarters(r, ()))
    _freeze(out[0], out[1])
    return out


def fwd_params(name, kind):
    """{"embed" [V, E], "w" [V, 1], "bias" [1]} fp32"""
    c = FWD_BY_NAME[name]
    if kind == "int":
        Ke, Kw, kb = int_params(c.V, c.E, c.seed)
        return {"embed": (Ke / 4.0).astype(np.float32), "w": (Kw / 4.0).astype(np.float32).reshape(-1, 1),
                "bias": np.array([kb / 4.0], np.float32)}
    p = H_.deepfm_params(c.seed, c.V, c.F, c.E, mlp_dims=(1,), scale=c.scale)
    return {k: p[k] for k in ("embed", "w", "bias")}


def int_case_is_exact(E, F):
    """In units of 1/16 every S_d^2, Q_d and their sum over d stays below 16 E F^2, and the first-order part, the bias
    and the halving add at most 32 (F + 1) units of 1/32: below 2^24 every intermediate is an fp32 integer multiple of
    its unit, in any order of the additions."""
    return 16 * E * F * F + 32 * (F + 1) < 2 ** 24


def with_zero_row(table, X):
    """(table with a zero row V appended, X with every id outside [0, V) replaced by V)"""
    V = table.shape[0]
    Xz = np.where((X >= 0) & (X < V), X, V)
    return np.concatenate([table, np.zeros((1,) + table.shape[1:], table.dtype)]), Xz


@functools.lru_cache(maxsize=4)
def fwd_reference(name, kind, oob=False):
    """{"rows" fp32 [B, F, E], "z" [B], "S" [B, E], "prob" [B] (normal alone)}: kind 'int' -> the int64 evaluation,
    exact in fp32; 'normal' -> oracle.layers_np in fp64.  Shared: do not write to them."""
    from oracle import layers_np as L
    c = FWD_BY_NAME[name]
    X = fwd_X(name, oob)
    p = fwd_params(name, kind)
    emb_z, Xz = with_zero_row(p["embed"], X)
    out = {"rows": emb_z[Xz]}
    if kind == "int":
        Ke, Kw, kb = int_params(c.V, c.E, c.seed)
        k = with_zero_row(Ke, X)[0][Xz]
        s, q = k.sum(1), (k * k).sum(1)
        z32 = 8 * kb + 8 * with_zero_row(Kw, X)[0][Xz].sum(1) + (s * s - q).sum(1)
        out["z"], out["S"] = (z32 / 32.0).astype(np.float32), (s / 4.0).astype(np.float32)
        assert np.array_equal(out["z"].astype(np.float64) * 32, z32)
    else:
        w_z = with_zero_row(p["w"], X)[0]
        prob, z = L.fm_forward(emb_z, w_z, p["bias"], Xz, np.float64)
        out["z"], out["prob"], out["S"] = z[:, 0], prob[:, 0], L.fm_terms(emb_z, w_z, Xz, np.float64)[1]
    _freeze(*out.values())
    return out


def fwd_bounds(ref):
    """the suite's own FM-forward bounds (tests/test_gpu_ops.py, test_emb_fm_fwd): z, prob, S"""
    return {"z": 1e-5 * max(1.0, float(np.abs(ref["z"]).max())), "prob": 1e-5,
            "S": 1e-5 * max(1.0, float(np.abs(ref["S"]).max()))}


def fwd_fp32_plain(name):
    """z [B] and S [B, E] of the normal values in fp32, the fields and then the dims added one after the other"""
    c = FWD_BY_NAME[name]
    X, p = fwd_X(name), fwd_params(name, "normal")
    S, Q = np.zeros((c.B, c.E), np.float32), np.zeros((c.B, c.E), np.float32)
    first = np.zeros(c.B, np.float32)
    for f in range(c.F):
        e = p["embed"][X[:, f]]
        S, Q, first = S + e, Q + e * e, first + p["w"][X[:, f], 0]
    part = np.zeros(c.B, np.float32)
    t = S * S - Q
    for d in range(c.E):
        part = part + t[:, d]
    return p["bias"][0] + first + np.float32(0.5) * part, S


# ---- the gather table -----------------------------------------------------------------------------------------------
GatherCase = collections.namedtuple("GatherCase", "name E ld n table_off out_off V seed kernel LPR regime")
ROWS_N_REGIMES = ("n_eq_1", "n_eq_RU_minus_1", "n_eq_RU", "n_eq_2RU_plus_3")
FLAT_N_REGIMES = ("one_block_tail", "whole_blocks", "blocks_and_tail")


def _gather_cases():
    out = []

    def add(E, ld, n, kernel, regime, table_off=0, out_off=0):
        name = "e%d%s%s%s_n%d" % (E, "_ld%d" % ld if ld != E else "", "_tmis" if table_off else "",
                                  "_omis" if out_off else "", n)
        out.append(GatherCase(name, E, ld, n, table_off, out_off, 331, len(out), kernel,
                              E // 4 if kernel == "rows" else None, regime))

    for E in (4, 8, 16, 32, 64, 128, 256):
        RU = (256 // (E // 4)) * 4                             # written out: R UNR rows per workgroup
        for ld in (E, 2 * E):
            for n, regime in zip((1, RU - 1, RU, 2 * RU + 3), ROWS_N_REGIMES):
                add(E, ld, n, "rows", regime)
    flat_n = tuple(zip((1, 256, 259), FLAT_N_REGIMES))         # n (E or E/4) elements: < 256, k 256, k 256 + tail
    for E in (12, 20, 100, 260, 512):
        for n, regime in flat_n:
            add(E, E, n, "vec4", regime)
    add(12, 24, 259, "vec4", "blocks_and_tail")
    for E, ld, toff, ooff in ((1, 1, 0, 0), (3, 3, 0, 0), (7, 7, 0, 0), (33, 33, 0, 0), (16, 17, 0, 0), (16, 16, 4, 0),
                              (16, 16, 0, 4), (3, 8, 0, 0)):
        for n, regime in flat_n:
            add(E, ld, n, "scalar", regime, toff, ooff)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


GATHER_CASES = _gather_cases()
GATHER_BY_NAME = {c.name: c for c in GATHER_CASES}


def flat_regime(units):
    return "one_block_tail" if units < 256 else "whole_blocks" if units % 256 == 0 else "blocks_and_tail"


def gather_regime(c, th=TH):
    cls = gather_class(c.E, c.ld, not c.table_off, not c.out_off, th)
    if cls.kernel == "rows":
        RU = cls.rows_per_wg
        return {1: "n_eq_1", RU - 1: "n_eq_RU_minus_1", RU: "n_eq_RU", 2 * RU + 3: "n_eq_2RU_plus_3"}.get(c.n)
    return flat_regime(c.n * (c.E // 4 if cls.kernel == "vec4" else c.E))


def table_vals(V, E, seed):
    """fp32 [V, E], standard normal, no two rows alike"""
    return H_.rng(3000 + seed).normal(size=(V, E)).astype(np.float32)


def gather_ids(c, oob=False):
    """int64 [n] of [0, V), the first 0 and the last V - 1; ``oob``: OOB_IDS spread over the list (n >= 8)"""
    idx = H_.rng(4000 + c.seed).integers(0, c.V, size=c.n, dtype=np.int64)
    idx[0] = c.V - 1
    if c.n > 1:
        idx[0], idx[-1] = 0, c.V - 1
    if oob:
        assert c.n >= 8
        at = (0, c.n // 3, c.n // 2, c.n - 1)
        idx[list(at)] = [c.V if v is None else v for v in OOB_IDS]
    return idx


def gather_reference(table, idx):
    tz, iz = with_zero_row(table, idx)
    return tz[iz]


# ---- the list gather table ------------------------------------------------------------------------------------------
ListsCase = collections.namedtuple("ListsCase", "name E ld n_lists cap V seed nc lpr counts")
LISTS_E = (4, 8, 12, 16, 20, 32, 36, 64, 100, 128, 132, 256)     # 100: nc = 25 < lpr = 32, the one lpr the rest leaves
# written out: E -> (nc, lpr)
LISTS_CLAIMS = {4: (1, 1), 8: (2, 2), 12: (3, 4), 16: (4, 4), 20: (5, 8), 32: (8, 8), 36: (9, 16), 64: (16, 16),
                100: (25, 32), 128: (32, 32), 132: (33, 64), 256: (64, 64)}
GARBAGE_WORD = 0x5A5A5A5A5A5A5A5A


def _lists_cases():
    out = []
    for E in LISTS_E:
        for ld in (E, E + 4):
            for n_lists in (1, 5):
                for cap in (1, 7, 300):
                    i = len(out)
                    pool = (cap, 0, 1, cap // 2 + 1, cap)      # drawn from {0, 1, cap} and mixed
                    counts = tuple(pool[(i + q) % 5] for q in range(n_lists))
                    out.append(ListsCase("e%d_ld%d_l%d_cap%d" % (E, ld, n_lists, cap), E, ld, n_lists, cap, 331, i,
                                         LISTS_CLAIMS[E][0], LISTS_CLAIMS[E][1], counts))
    return tuple(out)


LISTS_CASES = _lists_cases()
LISTS_BY_NAME = {c.name: c for c in LISTS_CASES}


def lists_msg(c, bad_used_slot=False):
    """int64 [n_lists, HDR + cap]: word 0 the count, word 1 garbage, the used slots ids of [0, V), every unused slot -7
    or V + 9.  ``bad_used_slot``: the last used slot of the last list that uses one holds V."""
    r = H_.rng(5000 + c.seed)
    msg = np.empty((c.n_lists, TH.HDR + c.cap), np.int64)
    msg[:, 0], msg[:, 1] = c.counts, GARBAGE_WORD
    slots = r.integers(0, c.V, size=(c.n_lists, c.cap), dtype=np.int64)
    unused = np.arange(c.cap)[None, :] >= np.asarray(c.counts)[:, None]
    bad = np.where((np.arange(c.n_lists)[:, None] + np.arange(c.cap)[None, :]) % 2 == 0, -7, c.V + 9)
    msg[:, TH.HDR:] = np.where(unused, bad, slots)
    if bad_used_slot:
        q = max(q for q in range(c.n_lists) if c.counts[q] > 0)
        msg[q, TH.HDR + c.counts[q] - 1] = c.V
    return msg


def lists_used(c):
    """bool [n_lists * cap]: slot j of list q is used"""
    return (np.arange(c.cap)[None, :] < np.asarray(c.counts)[:, None]).reshape(-1)


# ---- the backward table ---------------------------------------------------------------------------------------------
BwdCase = collections.namedtuple("BwdCase", "name E ld rows_given extra aligned B F V seed kernel")
BWD_SHAPES = ((64, 4), (37, 3))          # B F = 256 lookups: every element count a multiple of 256; 111: none is


def _bwd_cases():
    out = []
    for E, aligned, kernel in ((4, True, "vec"), (12, True, "vec"), (16, True, "vec"), (64, True, "vec"),
                               (256, True, "vec"), (1, True, "scalar"), (3, True, "scalar"), (5, True, "scalar"),
                               (16, False, "scalar")):
        for rows_given in (True, False):
            for ld in (E, 2 * E if E % 4 == 0 else E + 3):
                for extra in (True, False):
                    for B, F in BWD_SHAPES:
                        name = "e%d%s_%s_ld%d_%s_b%d" % (E, "" if aligned else "mis", "rows" if rows_given else "table",
                                                         ld, "extra" if extra else "noextra", B)
                        out.append(BwdCase(name, E, ld, rows_given, extra, aligned, B, F, 331, len(out), kernel))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


FM_BWD_CASES = _bwd_cases()
BWD_BY_NAME = {c.name: c for c in FM_BWD_CASES}


def bwd_units(c):
    """elements the kernel of a case spreads over its threads"""
    return c.B * c.F * (c.E // 4 if c.kernel == "vec" else c.E)


def bwd_inputs(c, kind, oob=False):
    """{"embed" [V, E], "X" [B, F], "gz" [B], "S" [B, E] (the exact sum of the looked-up rows, rounded to fp32 for the
    normal values), "extra" [B F, E], "ref" [B F, E]}: kind 'int' -> ref is the int64 evaluation of gz (S - e) + extra,
    exact in fp32; 'normal' -> oracle.layers_np.fm_backward in fp64 of the same fp32 inputs.  ``oob``: two ids lie
    outside [0, V) and stand for zero rows."""
    from oracle import layers_np as L
    r = H_.rng(6000 + c.seed)
    X = r.integers(0, c.V, size=(c.B, c.F), dtype=np.int64)
    X[0, 0], X[-1, -1] = 0, c.V - 1
    if oob:
        X[1, 0], X[-2, -1] = -1, (1 << 32) + 3
    if kind == "int":
        Ke, Kg, Kx = quarters(r, (c.V, c.E)), quarters(r, (c.B,)), quarters(r, (c.B * c.F, c.E))
        Kz, Xz = with_zero_row(Ke, X)
        k = Kz[Xz]
        s = k.sum(1)
        ref32 = 2 * Kg[:, None, None] * (s[:, None, :] - k) + (8 * Kx.reshape(c.B, c.F, c.E) if c.extra else 0)
        ref = (ref32 / 32.0).astype(np.float32).reshape(-1, c.E)
        assert np.array_equal(ref.astype(np.float64) * 32, ref32.reshape(-1, c.E))
        embed, gz, S, extra = (a / 4.0 for a in (Ke, Kg, s, Kx))
    else:
        embed = H_.deepfm_params(c.seed, c.V, c.F, c.E, mlp_dims=(1,), scale=0.5)["embed"]
        gz, extra = r.normal(size=(c.B,)), r.normal(size=(c.B * c.F, c.E))
        ez, Xz = with_zero_row(embed, X)
        S = ez[Xz].astype(np.float64).sum(1)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    out = {"embed": f32(embed), "X": X, "gz": f32(gz), "S": f32(S), "extra": f32(extra)}
    if kind == "int":
        out["ref"] = ref
    else:
        ez, Xz = with_zero_row(out["embed"], X)
        ref = L.fm_backward(ez, Xz, out["gz"].reshape(-1, 1), np.float64)[0]
        out["ref"] = ref + out["extra"].astype(np.float64) if c.extra else ref
    return out


def bwd_bound(ref):
    """the suite's own bound of the backward values (tests/test_gpu_ops.py, test_fm_bwd_vals_and_dedup)"""
    return 2e-6 * max(1.0, float(np.abs(ref).max()))
