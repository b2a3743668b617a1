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
    return cases


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
              "REC_DACT_PRELU": 5}
    codes = {k: v for k, v in ENUMS.items() if k.startswith(("REC_EPI_", "REC_ACT_", "REC_DACT_"))}
    assert codes == frozen
    bound = {n: getattr(ops, n) for n in dir(ops)
             if n.startswith(("EPI_", "ACT_", "DACT_")) and isinstance(getattr(ops, n), int)}
    assert bound == {k[len("REC_"):]: v for k, v in frozen.items()}    # every code has its name in ops.py, and no other
    for n, v in bound.items():
        assert v == ENUMS["REC_" + n], n
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

