"""CPU checks of the drop-in boundary: the C-ABI shared library loads without a GPU, exports every symbol that
include/mi355rec.h declares, the ctypes table generated from the header binds exactly that set with the types the header
spells, the shape limits the header defines are the ones the compiled library enforces, the operation codes ops.py binds
are the header's enumerators, and the host-side mirror keeps the reference's constructor keywords and error behaviour (no
compute calls here: nothing in this file needs a GPU)."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355rec.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rec_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from explicit_tf2_recommendation_amd import _lib
    syms = declared_symbols()
    assert len(syms) >= 40
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(_lib.SIGNATURES) == syms           # the binding table and the header agree, symbol for symbol
    assert _lib.lib.rec_version() >= 100


def test_generated_signatures_match_frozen_literals():
    """The bindings are generated from the header; these literals are not.  They are the hand-written table's entries
    for the longest and the oddest signatures, so a parser that quietly changes a type, drops an argument or a return
    type does not pass."""
    from explicit_tf2_recommendation_amd import _lib
    p, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    frozen = {
        "rec_gemm_f32": (i32, [i32, i32, i64, i64, i64, p, i64, p, i64, p, i64, i32, p, p, i64, p, i64, i32, p, p, p]),
        "rec_emb_afm_bwd_f32": (i32, [p, i64, i32, i64, p, i64, i32, i32, p, p, p, p, p, p, p, p, p, p, p, p, p, p, sz,
                                      p]),
        "rec_emb_fgcnn_bwd_f32": (i32, [i32, i64, i32, i32, p, p, p, p, p, p, p, p, p, p, sz, p]),
        "rec_dssm_fused_post_f32": (i32, [i64, i32, i32, i32, p, sz, p, p, p, p, p, p, p, p, p, p, p, p, p, p, p, i64,
                                          i64, i64, i64, p, f32, f32, f32, p]),
        "rec_adam_lr_t_f32": (f32, [f32, f32, f32, i64]),
        "rec_version": (i32, []),
        "rec_dedup_workspace_bytes": (sz, [i64]),
    }
    for name, want in frozen.items():
        assert _lib.SIGNATURES[name] == want, name
        fn = getattr(_lib.lib, name)
        assert (fn.restype, list(fn.argtypes)) == want, name
    res, args = _lib.SIGNATURES["rec_deepfm_fused_post_f32"]
    assert res is i32 and len(args) == 19 and args[17] is ctypes.POINTER(_lib.DeepFMLazyAdam)
    assert args[:17] == [i32, i64] + [p] * 14 + [i32] and args[18] is p
    assert _lib.DeepFMLazyAdam._fields_ == [
        ("table", p), ("ld", i64), ("V", i64), ("m_e", p), ("v_e", p), ("m_w", p), ("v_w", p), ("ld_state", i64),
        ("ld_wstate", i64), ("lr_t_dev", p), ("b1", f32), ("b2", f32), ("eps", f32), ("last", p), ("step_dev", p)]


def test_header_parser_is_closed_over_its_type_map():
    """A spelling outside the header's list is an error that names the declaration, never a silent pointer or int."""
    from explicit_tf2_recommendation_amd import _lib
    ok = _lib.prototypes("int rec_x(const float* const* a, int32_t n, double d, size_t s); size_t rec_y(void);")
    assert ok == {"rec_x": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t]),
                  "rec_y": (ctypes.c_size_t, [])}
    for bad in ("int rec_x(unsigned n);", "int rec_x(long long n);", "int rec_x(hipStream_t stream);",
                "int rec_x(my_struct* q);", "int rec_x(int);", "char* rec_x(int n);", "static int rec_x(int n);"):
        with pytest.raises(ImportError, match="rec_x"):
            _lib.prototypes(bad)
    with pytest.raises(ImportError, match="field n"):
        _lib.struct_fields("struct s { float* a; unsigned n; };", "s")
    text = _lib.strip_comments("#define REC_A 3 // x\n/* #define REC_B 4 */\n#define REC_C (-2)\n#define REC_D 1.5\n")
    assert _lib.constants(text) == {"REC_A": 3, "REC_C": -2}
    assert {"REC_OK": 0, "REC_E_ARG": -1, "REC_E_UNSUPPORTED": -2, "REC_E_WORKSPACE": -3,
            "REC_MAX_COLS": 128}.items() <= _lib.LIMITS.items()
    assert _lib.enums("enum { A = 3, B, C = (-2), D };") == {"A": 3, "B": 4, "C": -2, "D": -1}


def _ints(*values):
    return (ctypes.c_int * len(values))(*values)


def _limit_cases():
    """(define, f): f(v) = the family's rec_*_workspace_bytes with the limited size set to v and the others small."""
    from explicit_tf2_recommendation_amd._lib import lib
    fc = {"ccpm": lib.rec_ccpm_workspace_bytes, "fgcnn": lib.rec_fgcnn_workspace_bytes}
    cases = [
        ("REC_AFM_MAX_F", lambda v: lib.rec_afm_workspace_bytes(4, v, 4, 2)),
        ("REC_AFM_MAX_E", lambda v: lib.rec_afm_workspace_bytes(4, 3, v, 2)),
        ("REC_AFM_MAX_A", lambda v: lib.rec_afm_workspace_bytes(4, 3, 4, v)),
        ("REC_AUTOINT_MAX_F", lambda v: lib.rec_autoint_workspace_bytes(4, v, 4, 1, 0, 0)),
        ("REC_AUTOINT_MAX_E", lambda v: lib.rec_autoint_workspace_bytes(4, 3, v, 1, 0, 0)),
        ("REC_FIBINET_MAX_F", lambda v: lib.rec_fibinet_workspace_bytes(4, v, 4, 2, 0)),
        ("REC_FIBINET_MAX_E", lambda v: lib.rec_fibinet_workspace_bytes(4, 3, v, 2, 0)),
        ("REC_CIN_MAX_F", lambda v: lib.rec_cin_workspace_bytes(4, v, 4, 1, _ints(2))),
        ("REC_CIN_MAX_E", lambda v: lib.rec_cin_workspace_bytes(4, 3, v, 1, _ints(2))),
        ("REC_CIN_MAX_L", lambda v: lib.rec_cin_workspace_bytes(4, 3, 4, v, _ints(*[2] * v))),
        ("REC_CIN_MAX_H", lambda v: lib.rec_cin_workspace_bytes(4, 3, 4, 2, _ints(2, v))),
    ]
    for fam, ws in fc.items():            # pool = 1 is a k of CCPM's k-max pooling and a width of FGCNN's max pooling
        cases += [
            ("REC_FIELD_CONV_MAX_F:" + fam, lambda v, ws=ws: ws(4, v, 4, 1, _ints(2), _ints(2), _ints(1))),
            ("REC_FIELD_CONV_MAX_E:" + fam, lambda v, ws=ws: ws(4, 3, v, 1, _ints(2), _ints(2), _ints(1))),
            ("REC_FIELD_CONV_MAX_L:" + fam, lambda v, ws=ws: ws(4, 3, 4, v, _ints(*[2] * v), _ints(*[2] * v),
                                                                _ints(*[1] * v))),
            ("REC_FIELD_CONV_MAX_C:" + fam, lambda v, ws=ws: ws(4, 3, 4, 1, _ints(v), _ints(2), _ints(1))),
            ("REC_FIELD_CONV_MAX_KW:" + fam, lambda v, ws=ws: ws(4, 3, 4, 1, _ints(2), _ints(v), _ints(1))),
        ]
    # 20 fields: a pooling width one past the limit still leaves two rows, so only the limit can refuse it
    cases.append(("REC_FGCNN_MAX_PW",
                  lambda v: lib.rec_fgcnn_workspace_bytes(4, 20, 4, 1, _ints(2), _ints(2), _ints(v))))
    ln, blk = lib.rec_masknet_ln_workspace_bytes, lib.rec_masknet_block_workspace_bytes
    cases += [
        ("REC_MASKNET_MAX_F", lambda v: ln(4, v, 4)),
        ("REC_MASKNET_MAX_E", lambda v: ln(4, 3, v)),
        ("REC_MASKNET_MAX_D", lambda v: blk(4, v, 8, 4, 2)),
        ("REC_MASKNET_MAX_P", lambda v: blk(4, 8, v, 4, 2)),
        ("REC_MASKNET_MAX_O", lambda v: blk(4, 8, 8, v, 2)),
        ("REC_MASKNET_MAX_R", lambda v: blk(4, 8, 8, 4, v)),
    ]
    # The families after DIN answer through their LDS, workspace or scratch queries.  A limit that several families
    # share by design gets a case per family; a series of 32 steps holds one selected position past the limit (K <= T)
    sim, eta, sdim, esu = (lib.rec_sim_search_lds_bytes, lib.rec_eta_search_lds_bytes, lib.rec_sdim_lds_bytes,
                           lib.rec_esu_attn_lds_bytes)
    cases += [
        ("REC_CAPSULE_MAX_R:mind", lambda v: lib.rec_mind_routing_workspace_bytes(4, 2, 4, 1, 4, 2, v)),
        ("REC_CAPSULE_MAX_R:comirec", lambda v: lib.rec_comirec_dr_workspace_bytes(4, 2, 4, 1, 4, 2, v)),
        ("REC_SINE_MAX_L", lambda v: lib.rec_sine_lds_bytes(2, 4, 1, v, 1)),
        ("REC_CAN_MAX_L:layers", lambda v: lib.rec_can_lds_bytes(2, 4, v, _ints(*[1] * v), 1)),
        ("REC_CAN_MAX_L:order", lambda v: lib.rec_can_lds_bytes(2, 4, 1, _ints(1), v)),
        ("REC_SEARCH_MAX_D:sim", lambda v: sim(32, 1, v, 2)),
        ("REC_SEARCH_MAX_D:eta", lambda v: eta(32, 1, v, 4, 2)),
        ("REC_SEARCH_MAX_D:sdim", lambda v: sdim(32, 1, v, 2, 2, 2)),
        ("REC_SEARCH_MAX_K:sim", lambda v: sim(32, 1, 4, v)),
        ("REC_SEARCH_MAX_K:eta", lambda v: eta(32, 1, 4, 4, v)),
        ("REC_SEARCH_MAX_K:esu", lambda v: esu(v, 4, 1, 4)),
        ("REC_ESU_MAX_H", lambda v: esu(2, 4, v, 4)),
        ("REC_ETA_MAX_M", lambda v: eta(32, 1, 4, v, 2)),
        ("REC_SDIM_MAX_BITS:one group", lambda v: sdim(32, 1, 4, 1, v, 2)),
        ("REC_SDIM_MAX_S", lambda v: sdim(32, 1, 4, 2, 2, v)),
    ]
    return cases


def _last_fit(nbytes, cap):
    """the largest T >= 1 with nbytes(T) <= cap, for an nbytes that grows with T (by bisection)"""
    lo, hi = 1, 2
    assert nbytes(lo) <= cap
    while nbytes(hi) <= cap:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if nbytes(mid) <= cap else (lo, mid)
    return lo


def _cap_cases():
    """(define, nbytes, query): a launch cap of the header, the Python formula of a kernel's LDS as a function of the
    series length T (ops.py's *_lds_bytes, which the family host tests hold against the library's own answers) and the
    family's size query at that T, every other size small enough that only the cap can refuse the shape."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import lib
    tile, search = "REC_TILE_LDS_CAP", "REC_SEARCH_LDS_CAP"
    return [
        (tile + ":mind routing", lambda T: ops.mind_routing_lds_bytes(T, 48, 48, 4, 3),
         lambda T: lib.rec_mind_routing_workspace_bytes(4, T, 48, 1, 48, 4, 3)),
        (tile + ":mind attention", lambda Ns: ops.mind_laa_lds_bytes(Ns, 48, 4),
         lambda Ns: lib.rec_mind_laa_lds_bytes(Ns, 48, 1, 4)),
        (tile + ":comirec routing", lambda T: ops.comirec_dr_lds_bytes(T, 48, 3),
         lambda T: lib.rec_comirec_dr_workspace_bytes(4, T, 48, 1, 48, 4, 3)),
        (tile + ":comirec self-attentive", lambda T: ops.comirec_sa_lds_bytes(T, 48, 48, 4),
         lambda T: lib.rec_comirec_sa_workspace_bytes(4, T, 48, 1, 48, 4)),
        (tile + ":comirec hard attention", lambda Ns: ops.mind_laa_lds_bytes(Ns, 48, 4),
         lambda Ns: lib.rec_comirec_select_lds_bytes(Ns, 48, 1, 4)),
        (tile + ":sine", lambda T: ops.sine_lds_bytes(T, 48, 100, 5),
         lambda T: lib.rec_sine_lds_bytes(T, 48, 1, 100, 5)),
        (tile + ":can", lambda T: ops.can_lds_bytes(T, 16, (1, 1, 1), 3),
         lambda T: lib.rec_can_lds_bytes(T, 16, 3, _ints(1, 1, 1), 3)),
        (tile + ":dmr", lambda T: ops.dmr_lds_bytes(T, 48, 48, 6), lambda T: lib.rec_dmr_lds_bytes(T, 48, 1, 48, 6)),
        (tile + ":dien", lambda T: ops.dien_lds_bytes(T, 128, ops.DIEN_AUGRU),
         lambda T: lib.rec_dien_augru_lds_bytes(T, 128, ops.DIEN_AUGRU)),
        (search + ":sim", lambda T: ops.sim_search_lds_bytes(T, 1, 48),
         lambda T: lib.rec_sim_search_lds_bytes(T, 1, 48, 2)),
        (search + ":eta", lambda T: ops.eta_search_lds_bytes(T, 48, 4),
         lambda T: lib.rec_eta_search_lds_bytes(T, 1, 48, 4, 2)),
        (search + ":sdim", lambda T: ops.sdim_lds_bytes(T, 48, 2, 2),
         lambda T: lib.rec_sdim_lds_bytes(T, 1, 48, 2, 2, 2)),
    ]


def test_header_limits_are_the_compiled_library_s():
    """Every shape limit include/mi355rec.h defines, against the library the kernel files were compiled into: at the
    limit the family's workspace query answers a size, one past it 0 (unsupported).  Fails when a kernel file and the
    header disagree, in either direction."""
    from explicit_tf2_recommendation_amd._lib import lib, LIMITS
    seen = set()
    for key, f in _limit_cases():
        name = key.split(":")[0]
        seen.add(name)
        limit = LIMITS[name]
        assert f(limit) > 0, (key, limit)
        assert f(limit + 1) == 0, (key, limit + 1)
    # FiBiNet's workspace does not depend on the continuous features: with B == 0 the forward checks the shape and
    # returns before it looks at a pointer or launches anything
    def fibinet_c(c):
        return lib.rec_fibinet_fwd_f32(None, None, None, None, None, 0, 3, 4, c, 2, 0, None, None, None, None)
    assert fibinet_c(LIMITS["REC_FIBINET_MAX_C"]) == 0 and fibinet_c(LIMITS["REC_FIBINET_MAX_C"] + 1) == -2
    # the backward grid of the field-conv stacks: a slot of NW = kw C + C floats per workgroup, and no more slots than
    # the limit however many columns there are (B E / 16 columns per workgroup at the least)
    grid = LIMITS["REC_FIELD_CONV_BWD_GRID"]
    for ws in (lib.rec_ccpm_workspace_bytes, lib.rec_fgcnn_workspace_bytes):
        sizes = [ws(B, 3, 16, 1, _ints(2), _ints(2), _ints(1)) for B in (1, 64 * grid, 128 * grid)]
        assert sizes[0] < sizes[1] == sizes[2] == -(-grid * (2 * 2 + 2) * 4 // 256) * 256, sizes
    # DIN attention has no workspace either: with B == 0 both directions answer from the sizes alone.  Key width D = E C
    # and hidden units H; beyond D = WIDE_D only H <= WIDE_MAX_H
    def din(D, H):
        head = (None, D, 10, D, 1, None, 0, 5, None, None, H, 0, None, None, None, None, None, 0, 1)
        fwd = lib.rec_din_attn_fwd_f32(*head, None, None, None, None)
        assert fwd == lib.rec_din_attn_bwd_f32(*head, *[None] * 9), (D, H)
        return fwd
    max_d, max_h, wide_d, wide_h = (LIMITS["REC_DIN_" + k] for k in ("MAX_D", "MAX_H", "WIDE_D", "WIDE_MAX_H"))
    assert din(max_d, wide_h) == 0 and din(max_d + 1, 1) == -2
    assert din(wide_d, max_h) == 0 and din(1, max_h + 1) == -2
    assert din(wide_d + 1, wide_h) == 0 and din(wide_d + 1, wide_h + 1) == -2 and din(max_d, max_h) == -2
    seen |= {"REC_DIN_MAX_D", "REC_DIN_MAX_H", "REC_DIN_WIDE_D", "REC_DIN_WIDE_MAX_H"}
    seen |= {"REC_FIBINET_MAX_C", "REC_FIELD_CONV_BWD_GRID"}
    # SINE's aux kernels have no size query: with NULL pointers they answer -2 from the sizes alone, and -1 for the
    # pointers once the sizes are inside the limits
    max_l, aux_d = LIMITS["REC_SINE_MAX_L"], LIMITS["REC_SINE_AUX_MAX_D"]
    for aux in (lambda L, D: lib.rec_sine_aux_fwd_f32(None, L, D, None, None),
                lambda L, D: lib.rec_sine_aux_bwd_f32(None, L, D, None, None, None)):
        assert aux(max_l, aux_d) == -1 and aux(max_l, aux_d + 1) == -2 and aux(max_l + 1, aux_d) == -2
    # the ESU attention's widths are even: two past the limit is the next width only the limit refuses.  D and dk alike
    esu, esu_d = lib.rec_esu_attn_lds_bytes, LIMITS["REC_ESU_MAX_D"]
    assert esu(2, esu_d, 1, 4) > 0 and esu(2, esu_d + 2, 1, 4) == 0
    assert esu(2, 4, 1, esu_d) > 0 and esu(2, 4, 1, esu_d + 2) == 0
    # SDIM's hash bits are those of all groups together
    bits = LIMITS["REC_SDIM_MAX_BITS"]
    assert bits % 4 == 0 and lib.rec_sdim_lds_bytes(32, 1, 4, 4, bits // 4, 2) > 0
    assert lib.rec_sdim_lds_bytes(32, 1, 4, 3, bits // 3 + 1, 2) == 0                     # 3 groups of 11 bits at 32
    seen |= {"REC_SINE_AUX_MAX_D", "REC_ESU_MAX_D"}
    # The launch caps: the longest series whose LDS, by the formula the header gives, stays within the cap is accepted
    # and the next one refused.  (The ESU attention cannot reach its cap inside its other limits; the DIN attention's
    # tiles are held to theirs by the static_asserts of csrc/din.hip and show above as WIDE_D / WIDE_MAX_H.)
    for key, nbytes, query in _cap_cases():
        name = key.split(":")[0]
        seen.add(name)
        T = _last_fit(nbytes, LIMITS[name])
        assert query(T) > 0, (key, T)
        assert query(T + 1) == 0, (key, T + 1)
    # POSO-MLP's tile grows with the widths, not with a length: two chained layers of U units behind inputs as wide as
    # they come.  The widest U ops.py accepts under the cap is the widest the library accepts
    from explicit_tf2_recommendation_amd import ops
    wide = LIMITS["REC_MASKNET_MAX_D"]

    def poso(U):
        try:
            ops.poso_mlp_check_shape(wide, wide, 1, [U, U], 1)
        except NotImplementedError as e:
            assert "a tile of %d bytes of LDS" % LIMITS["REC_POSO_LDS_CAP"] in str(e)
            return False
        return True
    U = max(u for u in range(1, LIMITS["REC_MASKNET_MAX_O"]) if poso(u))
    assert not poso(U + 1) and U + 1 <= LIMITS["REC_MASKNET_MAX_O"]         # the cap refused it, no other limit
    assert lib.rec_poso_mlp_scratch_bytes(4, wide, wide, 1, 2, _ints(U, U), 1) > 0
    assert lib.rec_poso_mlp_scratch_bytes(4, wide, wide, 1, 2, _ints(U + 1, U + 1), 1) == 0
    seen.add("REC_POSO_LDS_CAP")
    status = {"REC_OK", "REC_E_ARG", "REC_E_UNSUPPORTED", "REC_E_WORKSPACE", "REC_MAX_COLS"}
    assert seen == set(LIMITS) - status                                # a limit added to the header gets a case here


def test_ops_limits_are_the_header_s():
    """ops.py keeps its public names and no literal of its own: each is the header's define."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import LIMITS
    for prefix, family, dims in (("AFM", "AFM", "FEA"), ("AUTOINT", "AUTOINT", "FE"), ("FIBINET", "FIBINET", "FEC"),
                                 ("CIN", "CIN", "FELH"), ("CCPM", "FIELD_CONV", ("F", "E", "L", "C", "KW")),
                                 ("FGCNN", "FIELD_CONV", ("F", "E", "L", "C", "KW")), ("FGCNN", "FGCNN", ("PW",)),
                                 ("MASKNET", "MASKNET", "FEDPOR")):
        for d in dims:
            assert getattr(ops, "%s_MAX_%s" % (prefix, d)) == LIMITS["REC_%s_MAX_%s" % (family, d)], (prefix, d)
    assert ops.FGCNN_BWD_GRID == LIMITS["REC_FIELD_CONV_BWD_GRID"]
    with pytest.raises(NotImplementedError, match="fields <= %d" % LIMITS["REC_AFM_MAX_F"]):
        ops.afm_check_shape(LIMITS["REC_AFM_MAX_F"] + 1, 4, 2)
    ops.afm_check_shape(LIMITS["REC_AFM_MAX_F"], 4, 2)
    for name, define in (("MIND_MAX_ROUNDS", "CAPSULE_MAX_R"), ("SINE_MAX_L", "SINE_MAX_L"), ("CAN_MAX_W", "AFM_MAX_E"),
                         ("CAN_MAX_LAYERS", "CAN_MAX_L"), ("CAN_MAX_ORDER", "CAN_MAX_L"), ("SIM_MAX_D", "ESU_MAX_D"),
                         ("SIM_MAX_K", "SEARCH_MAX_K"), ("SIM_MAX_H", "ESU_MAX_H"), ("ETA_MAX_M", "ETA_MAX_M"),
                         ("SDIM_MAX_BITS", "SDIM_MAX_BITS"), ("SDIM_MAX_S", "SDIM_MAX_S"),
                         ("SDIM_MAX_D", "SEARCH_MAX_D")):
        assert getattr(ops, name) == LIMITS["REC_" + define], name
    rounds, concepts, can_l = LIMITS["REC_CAPSULE_MAX_R"], LIMITS["REC_SINE_MAX_L"], LIMITS["REC_CAN_MAX_L"]
    key, top, bits = LIMITS["REC_SEARCH_MAX_D"], LIMITS["REC_SEARCH_MAX_K"], LIMITS["REC_ETA_MAX_M"]
    esu_d, esu_h = LIMITS["REC_ESU_MAX_D"], LIMITS["REC_ESU_MAX_H"]
    sd_bits, sd_s = LIMITS["REC_SDIM_MAX_BITS"], LIMITS["REC_SDIM_MAX_S"]
    # (message, check, arguments one past the limit, arguments at the limit)
    pairs = [
        ("routing rounds <= %d" % rounds, ops.mind_check_shape, (8, 8, 2, rounds + 1), (8, 8, 2, rounds)),
        ("routing rounds <= %d" % rounds, ops.comirec_check_shape, (8, 8, 2, rounds + 1), (8, 8, 2, rounds)),
        ("L <= %d" % concepts, ops.sine_check_shape, (8, concepts + 1, 2), (8, concepts, 2)),
        ("at most %d layers" % can_l, ops.can_check_shape, (4, [1] * (can_l + 1), 1), (4, [1] * can_l, 1)),
        ("order <= %d" % can_l, ops.can_check_shape, (4, [1], can_l + 1), (4, [1], can_l)),
        ("coef <= %d" % LIMITS["REC_AFM_MAX_E"], ops.can_check_shape, (LIMITS["REC_AFM_MAX_E"] + 1, [1], 1),
         (LIMITS["REC_AFM_MAX_E"], [1], 1)),
        ("series features <= %d" % key, ops.sim_check_shape, (key + 1,), (key,)),
        ("k <= %d selected" % top, ops.sim_check_shape, (8, 32, top + 1), (8, 32, top)),
        ("key_dim <= %d and" % esu_d, ops.sim_check_shape, (esu_d + 2, 32, 2, 1), (esu_d, 32, 2, 1)),
        ("key_dim <= %d and" % esu_d, ops.sim_check_shape, (8, 32, 2, 1, esu_d + 2), (8, 32, 2, 1, esu_d)),
        ("num_heads <= %d" % esu_h, ops.sim_check_shape, (8, 32, 2, esu_h + 1), (8, 32, 2, esu_h)),
        ("series features <= %d" % key, ops.eta_check_shape, (key + 1,), (key,)),
        ("lsh_topk <= %d" % top, ops.eta_check_shape, (8, 32, top + 1), (8, 32, top)),
        ("lsh_dim <= %d" % bits, ops.eta_check_shape, (8, 32, 2, bits + 1), (8, 32, 2, bits)),
        ("series features <= %d" % key, ops.sdim_check_shape, (key + 1,), (key,)),
        ("candidates <= %d" % sd_s, ops.sdim_check_shape, (8, 32, sd_s + 1), (8, 32, sd_s)),
        ("<= %d hash bits" % sd_bits, ops.sdim_check_shape, (8, 32, 2, 1, sd_bits + 1), (8, 32, 2, 1, sd_bits)),
    ]
    # and the launch caps, one family each: the longest series the Python formula fits, and the next
    tile, search = LIMITS["REC_TILE_LDS_CAP"], LIMITS["REC_SEARCH_LDS_CAP"]
    T = _last_fit(lambda T: ops.can_lds_bytes(T, 16, (1, 1, 1), 3), tile)
    pairs.append(("<= %d bytes" % tile, ops.can_check_shape, (16, (1, 1, 1), 3, T + 1), (16, (1, 1, 1), 3, T)))
    T = _last_fit(lambda T: ops.sim_search_lds_bytes(T, 1, 48), search)
    pairs.append(("<= %d bytes" % search, ops.sim_check_shape, (48, T + 1), (48, T)))
    T = _last_fit(lambda T: ops.eta_search_lds_bytes(T, 48, 4), search)
    pairs.append(("<= %d bytes" % search, ops.eta_check_shape, (48, T + 1, 2, 4), (48, T, 2, 4)))
    T = _last_fit(lambda T: ops.sdim_lds_bytes(T, 48, 2, 2), search)
    pairs.append(("<= %d bytes" % search, ops.sdim_check_shape, (48, T + 1, 2, 2, 2), (48, T, 2, 2, 2)))
    for message, check_shape, past, at in pairs:
        with pytest.raises(NotImplementedError, match=re.escape(message)):
            check_shape(*past)
        check_shape(*at)


def test_ops_codes_are_the_header_s_and_the_header_s_are_frozen():
    """The operation codes are the header's enumerators, and ops.py binds its names to them.  The literal below is
    deliberate: saved graphs, recorded profiles and outside callers hold these numbers, so renumbering the header fails
    here.  Shape limits are defines (LIMITS, the tables above): none may come in as an enumerator."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import ENUMS
    frozen = {"REC_EPI_NONE": 0, "REC_EPI_BIAS": 1, "REC_EPI_BIAS_RELU": 2, "REC_EPI_BIAS_SIGMOID": 3,
              "REC_EPI_BIAS_TANH": 4, "REC_EPI_CROSS": 5, "REC_EPI_ADD": 6,
              "REC_ACT_NONE": 0, "REC_ACT_RELU": 1, "REC_ACT_SIGMOID": 2, "REC_ACT_TANH": 3,
              "REC_DACT_NONE": 0, "REC_DACT_RELU": 1, "REC_DACT_SIGMOID": 2, "REC_DACT_TANH": 3, "REC_DACT_DICE": 4,
              "REC_DACT_PRELU": 5,
              "REC_FIBINET_TYPE_ALL": 0, "REC_FIBINET_TYPE_EACH": 1, "REC_FIBINET_TYPE_INTERACTION": 2,
              "REC_AUTOINT_RES_NONE": 0, "REC_AUTOINT_RES_ADD": 1, "REC_AUTOINT_RES_LEARNED": 2,
              "REC_DIEN_GRU": 0, "REC_DIEN_AUGRU": 1, "REC_DIEN_AGRU": 2,
              "REC_SDIM_MODE_REFERENCE": 0, "REC_SDIM_MODE_VALID": 1}
    modes = ("REC_FIBINET_TYPE_", "REC_AUTOINT_RES_", "REC_SDIM_MODE_")    # bound as the values of a dict of ops.py
    codes = {k: v for k, v in ENUMS.items() if k.startswith(("REC_EPI_", "REC_ACT_", "REC_DACT_", "REC_DIEN_") + modes)}
    assert codes == frozen
    bound = {n: getattr(ops, n) for n in dir(ops)
             if n.startswith(("EPI_", "ACT_", "DACT_", "DIEN_")) and isinstance(getattr(ops, n), int)}
    assert bound == {k[len("REC_"):]: v for k, v in frozen.items() if not k.startswith(modes)}
    for n, v in bound.items():                                         # every code has its name in ops.py, and no other
        assert v == ENUMS["REC_" + n], n
    assert ops.DIEN_MODE == {"AUGRU": ENUMS["REC_DIEN_AUGRU"], "AGRU": ENUMS["REC_DIEN_AGRU"]}
    assert ops.FIBINET_TYPES == {k: ENUMS["REC_FIBINET_TYPE_" + k.upper()] for k in ("all", "each", "interaction")}
    assert ops.SDIM_MODES == {k: ENUMS["REC_SDIM_MODE_" + k.upper()] for k in ("reference", "valid")}
    none, add, learned = (ENUMS["REC_AUTOINT_RES_" + k] for k in ("NONE", "ADD", "LEARNED"))
    assert ops.AUTOINT_RES == {(False, False): none, (False, True): none, (True, False): add, (True, True): learned}
    assert not [k for k in ENUMS if k.startswith("REC_MASKNET_") or re.search(r"_MAX_\w+$", k)]
    assert set(ENUMS) == set(frozen)                                   # an enumerator added to the header gets a line here


def test_argument_errors_do_not_need_a_gpu():
    """Status codes of the ABI: invalid arguments are rejected on the host before anything is enqueued."""
    from explicit_tf2_recommendation_amd._lib import lib, check
    assert lib.rec_emb_gather_f32(None, 10, 4, 4, None, 5, None, None, None) == -1          # null table, n > 0
    assert lib.rec_emb_gather_f32(None, 10, 4, 2, None, 0, None, None, None) == -1          # ld < E
    assert lib.rec_emb_gather_f32(None, 10, 4, 4, None, 0, None, None, None) == 0           # empty batch is a no-op
    assert lib.rec_gemm_f32(0, 0, 4, 4, 4, None, 4, None, 4, None, 4, 0, None, None, 0, None, 0, 1, None, None,
                            None) == -1
    assert lib.rec_dedup_workspace_bytes(0) > 0
    with pytest.raises(ValueError):
        check(-1, "x")
    with pytest.raises(NotImplementedError):
        check(-2, "x")


def test_fused_deepfm_entry_points_validate_their_option_groups():
    """The merged entry points of the fused DeepFM step (one per launch): which optional groups go together is decided on
    the host, before anything is launched.  Every required pointer is a non-NULL dummy: validation reads only values."""
    from explicit_tf2_recommendation_amd._lib import lib, DeepFMLazyAdam
    d = ctypes.c_void_p(4096)                                           # 16-byte aligned, never dereferenced
    F, B, V = 3, 64, 1000
    cols = (ctypes.c_void_p * F)(*[4096] * F)
    w = (ctypes.c_void_p * 8)(*[4096] * 8)

    def main(ld=32, dloc=None, col_nu=None, g_rows=None, clock=(None, None, 0, None)):
        return lib.rec_deepfm_fused3_main_f32(d, ld, V, cols, F, B, w, d, d, d, None, d, d, dloc, col_nu, g_rows, *clock,
                                              None)
    assert main(dloc=d, col_nu=None, g_rows=d) == -1                    # a partial direct group
    assert main(dloc=None, col_nu=d) == -1 and main(dloc=None, g_rows=d) == -1
    assert main(clock=(d, None, 4, d)) == -1                            # a partial clock group
    assert main(clock=(d, d, 0, d)) == -1 and main(clock=(d, d, 4, None)) == -1
    assert main(ld=18) == -2 and main(ld=22) == -2                      # plain: ld >= 20, a multiple of 4
    assert main(ld=20, dloc=d, col_nu=d, g_rows=d) == -2                # direct: ld = 32
    assert main(ld=20, dloc=d, col_nu=None, g_rows=d) == -2             # (the ld rule is judged before the pointers)

    g = (ctypes.c_void_p * 7)(*[4096] * 7)
    adam = DeepFMLazyAdam(4096, 32, V, 4096, 4096, 4096, 4096, 16, 1, 4096, 0.9, 0.999, 1e-7, None, None)

    def post(uniq=d, g_w=d, n_uniq=d, slot_map=None, direct=0, adam=None):
        return lib.rec_deepfm_fused_post_f32(F, B, d, d, g, d, d, d, d, d, d, uniq, d, g_w, n_uniq, slot_map, direct,
                                             adam, None)
    assert post(uniq=None, g_w=None, n_uniq=None, slot_map=d, direct=1) == -2
    assert post(direct=0, adam=adam) == -2
    assert post(uniq=None) == -1 and post(n_uniq=None) == -1 and post(g_w=None) == -1
    assert post(slot_map=d) == -1                                       # packed rows: uniq_ids / g_w_rows / n_uniq stay NULL
    adam.ld = 20
    assert post(direct=1, adam=adam) == -2                              # the table must be the fused [V,32] rows
    adam.ld, adam.m_e = 32, None
    assert post(direct=1, adam=adam) == -1


def test_layer_signatures_match_the_reference():
    """Constructor keywords of 2.FM/CustomLayers.py:117,167,220-222,255-256; 3.DCN/CustomLayers.py:171,220-224,273;
    5.DIN/CustomLayers.py:164,200-205 (reference spelling kept, e.g. `is_dropput`)."""
    from explicit_tf2_recommendation_amd import layers as CL
    want = {
        CL.MLPLayer: ["units", "activation", "use_bias", "is_batch_norm", "is_dropput", "kernel_initializer",
                      "bias_initializer"],
        CL.FMRankingLayer: ["feature_names", "feature_dims", "embedding_dims"],
        CL.DeepFMRankingLayer: ["feature_names", "feature_dims", "embedding_dims", "mlp_dims"],
        CL.DSSMSingleTowerLayer: ["feature_names", "feature_dims", "embedding_dims", "mlp_dims", "final_dim"],
        CL.DSSMTwoTowerRetrievalLayer: ["u_feature_names", "i_feature_names", "u_feature_dims", "i_feature_dims",
                                        "u_embedding_dims", "i_embedding_dims", "u_mlp_dims", "i_mlp_dims", "final_dim"],
        CL.CrossLayer: ["layer_num", "reg_w", "reg_b"],
        CL.MatrixCrossLayer: ["layer_num", "reg_w", "reg_b"],
        CL.DeepCrossNetworkLayer: ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                   "units", "activation", "layer_num", "reg_w", "reg_b", "type"],
        CL.DinActivationLayer: ["activation"],
        CL.DINLayer: ["user_and_context_categorical_features", "item_categorical_features",
                      "behavior_series_features", "continuous_features", "feature_dims", "embedding_dims", "activation",
                      "padding_index"],
    }
    for cls, names in want.items():
        params = list(inspect.signature(cls.__init__).parameters)[1:]
        assert params[: len(names)] == names, (cls.__name__, params)
    # reference defaults
    assert inspect.signature(CL.DSSMSingleTowerLayer.__init__).parameters["embedding_dims"].default == 8
    assert inspect.signature(CL.DeepFMRankingLayer.__init__).parameters["mlp_dims"].default == [32, 8]
    assert inspect.signature(CL.DeepCrossNetworkLayer.__init__).parameters["type"].default == "vec"
    assert inspect.signature(CL.DINLayer.__init__).parameters["activation"].default == "Dice"


def test_host_side_errors_match_the_reference():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(ValueError):                      # 2.FM/CustomLayers.py:27-30
        CL.MLPLayer(units=[])
    with pytest.raises(AssertionError):                  # 5.DIN/CustomLayers.py:209-210
        CL.DINLayer(item_categorical_features=["a", "b"], behavior_series_features=["x"], feature_dims=10)
    layer = CL.FMRankingLayer(feature_names=["a"], feature_dims=10)
    import torch
    with pytest.raises(RuntimeError):                    # the HIP path has no CPU fallback: CPU tensors are refused
        from explicit_tf2_recommendation_amd import ops
        ops.emb_gather(torch.zeros(4, 4), torch.zeros(2, dtype=torch.int64))
    assert [n for n, _ in layer.named_parameters()] == ["bias", "embed.embeddings", "w.embeddings"]


def test_synthetic_generator_honours_the_datagenerator_contract():
    """2.FM/DataGenerator.py:76-88,126-134: one global id space, field f owns [offset_f, offset_f + dim_f)."""
    import numpy as np
    from explicit_tf2_recommendation_amd import data
    V, names = 1003, ["a", "b", "c"]
    info = data.data_info(V, 3)
    assert info[-1] == V and sum(info[0]) == V and info[1] == [0, info[0][0], info[0][0] + info[0][1]]
    for dist in ("uniform", "zipf"):
        g = data.SyntheticGenerator(names, V, dist=dist, seed=1)
        b = g.batch(500)
        assert b["label"].dtype == np.float32 and b["label"].shape == (500, 1)
        for f, n in enumerate(names):
            x = b[n]
            assert x.dtype == np.int64 and x.shape == (500, 1)
            assert x.min() >= info[1][f] and x.max() < info[1][f] + info[0][f]
    g = data.SyntheticGenerator(["u"], 900, series=["s1", "s2"], seq_len=7, seed=2)
    b = g.batch(64)
    assert b["s1"].shape == (64, 7)
    pad = b["s1"] == 0
    assert np.array_equal(pad, b["s2"] == 0)            # right padding with padding_index on every series feature
    assert np.all(pad[:, 1:] >= pad[:, :-1])            # once padded, padded to the end
    a = data.SyntheticGenerator(names, V, seed=5).batch(10)
    c = data.SyntheticGenerator(names, V, seed=5).batch(10)
    assert all(np.array_equal(a[k], c[k]) for k in a)   # seeded


def test_torch_library_registration():
    """the hot operators are registered with the PyTorch dispatcher as TORCH_LIBRARY(mi355rec, ...)
    (csrc/torch_ops.cpp, a host-only wrapper over the same C ABI); ops.py calls them as torch.ops.mi355rec.<op>."""
    import torch
    from explicit_tf2_recommendation_amd import _lib, ops  # noqa: F401  (importing the package loads the library)
    assert os.path.exists(_lib.TORCH_LIB_PATH)
    names = ["index_pack", "emb_gather", "emb_fm_fwd", "emb_fm_bwd_vals", "gemm", "act_fwd", "act_bwd", "colsum",
             "bce_fwd_bwd", "dedup_plan", "segment_sum", "cosine_fwd", "cosine_bwd", "crossnet_mat_bwd_elem", "axpby"]
    for n in names:
        op = getattr(torch.ops.mi355rec, n)
        assert "mi355rec::" + n in str(op.default._schema)
    assert "Tensor A, Tensor B, bool transA, bool transB" in str(torch.ops.mi355rec.gemm.default._schema)
    # no CPU kernel is registered: the dispatcher refuses CPU tensors (the HIP path has no fallback)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.mi355rec.cosine_fwd(torch.zeros(2, 4), torch.zeros(2, 4))

