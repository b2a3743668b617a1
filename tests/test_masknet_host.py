"""CPU checks of MaskNet: the numpy and torch restatements against each other in fp64 (tests/masknet_ref.py), the
LayerNorm edge cases of the input stage, the header's declarations and limits and the library's exports, the C-ABI status
codes and the ops.py guards without a GPU, the layers' parameter names and shapes in both stacking modes, and
ModelManager(layer='MaskNet')."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

from tests import masknet_ref as MR

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
ENTRY_POINTS = ["rec_masknet_ln_workspace_bytes", "rec_emb_masknet_ln_fwd_f32", "rec_emb_masknet_ln_bwd_f32",
                "rec_masknet_block_workspace_bytes", "rec_mask_block_fwd_f32", "rec_mask_block_bwd_f32"]
LIMITS = {"F": 64, "E": 64, "D": 512, "P": 512, "O": 128, "R": 4}


@pytest.mark.parametrize("B,Fc,Fk,E", [(1, 1, 0, 1), (2, 1, 1, 3), (5, 10, 3, 16), (4, 3, 2, 40), (3, 0, 2, 5)])
def test_input_stage_restatements_agree(B, Fc, Fk, E):
    r = np.random.default_rng(B * 10 + Fc)
    table, X, values, gamma, beta = MR.make_input(r, B, Fc, Fk, E, 7)
    F = Fc + Fk
    dn, de = r.uniform(-1, 1, (B, F * E)), r.uniform(-1, 1, (B, F * E))
    ref = MR.input_stage_numpy(table, X, values, gamma, beta, dn, de)
    xe, xn, dt, dg, db = MR.input_stage_torch_grads(table, X, values, gamma, beta, dn, de, torch.float64)
    for got, want in ((xe, ref["x_emb"]), (xn, ref["x_norm"]), (dt, ref["dtable"]), (dg, ref["dgamma"]),
                      (db, ref["dbeta"])):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    # the IndexedSlices values carry the continuous fields' value; without the direct gradient they are that much less
    ref0 = MR.input_stage_numpy(table, X, values, gamma, beta, dn)
    scale = np.concatenate([np.ones((B, Fc)), values], 1)
    np.testing.assert_allclose(ref["vals"] - ref0["vals"], (de.reshape(B, F, E) * scale[:, :, None]).reshape(B * F, E),
                               rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,D,P,O,R", [(1, 1, 1, 1, 1), (2, 3, 3, 5, 2), (5, 130, 130, 33, 3), (6, 208, 32, 32, 3),
                                       (7, 20, 7, 7, 3)])
def test_block_restatements_agree(B, D, P, O, R):
    r = np.random.default_rng(B + D)
    params = MR.make_block(r, D, P, O, R)
    xe, v, dy = r.normal(0, 0.5, (B, D)), r.normal(0, 1, (B, P)), r.uniform(-1, 1, (B, O))
    ref = MR.block_numpy(xe, v, params, dy)
    y, dv, dx, dp = MR.block_torch_grads(xe, v, params, dy, torch.float64)
    np.testing.assert_allclose(y, ref["y"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dv, ref["dv"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dx, ref["dx_emb"], rtol=1e-9, atol=1e-12)
    for got, want in zip(dp, ref["dparams"]):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("mode,NB", [("serial", 3), ("parallel", 2), ("serial", 1)])
def test_layer_restatements_agree(mode, NB):
    r = np.random.default_rng(NB)
    B, Fc, Fk, E, O = 6, 3, 2, 4, 5
    table, X, values, gamma, beta = MR.make_input(r, B, Fc, Fk, E, 9)
    blocks = MR.make_stack(r, Fc + Fk, E, O, NB, mode)
    head = MR.make_head(r, O if mode == "serial" else NB * O, 4)
    dout = r.uniform(-1, 1, (B, 1))
    ref = MR.masknet_numpy(table, X, values, gamma, beta, blocks, head, mode, dout)
    out, dt, dg, db, dbl, dh = MR.masknet_torch_grads(table, X, values, gamma, beta, blocks, head, mode, dout,
                                                      torch.float64)
    assert ref["output"].shape == (B, 1)
    np.testing.assert_allclose(out, ref["output"], rtol=1e-9, atol=1e-12)
    pairs = [(dt, ref["dtable"]), (dg, ref["dgamma"]), (db, ref["dbeta"])] + list(zip(dh, ref["dhead"]))
    for k in range(NB):
        pairs += list(zip(dbl[k], ref["dblocks"][k]))
    for got, want in pairs:
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-11)


def test_layernorm_of_a_one_element_field_and_of_a_zero_row_returns_beta():
    r = np.random.default_rng(3)
    # E = 1: every field is its own mean
    table, X, values, gamma, beta = MR.make_input(r, 4, 2, 1, 1, 5)
    dn = r.uniform(-1, 1, (4, 3))
    ref = MR.input_stage_numpy(table, X, values, gamma, beta, dn)
    np.testing.assert_allclose(ref["x_norm"], np.tile(beta.reshape(1, 3), (4, 1)), rtol=0, atol=1e-15)
    assert np.isfinite(ref["vals"]).all() and np.count_nonzero(ref["vals"]) == 0
    _, xn, dt, dg, _ = MR.input_stage_torch_grads(table, X, values, gamma, beta, dn, None, torch.float32)
    np.testing.assert_allclose(xn, np.tile(beta.reshape(1, 3), (4, 1)), rtol=0, atol=1e-7)
    assert np.isfinite(dt).all() and np.isfinite(dg).all()
    # value = 0: an all-zero row
    table, X, values, gamma, beta = MR.make_input(r, 3, 2, 2, 8, 5)
    values[:, 0] = 0.0
    dn = r.uniform(-1, 1, (3, 32))
    ref = MR.input_stage_numpy(table, X, values, gamma, beta, dn, dn)
    got = ref["x_norm"].reshape(3, 4, 8)[:, 2]
    np.testing.assert_allclose(got, np.tile(beta[2], (3, 1)), rtol=0, atol=1e-15)
    assert np.isfinite(ref["vals"]).all() and np.isfinite(ref["dgamma"]).all()
    assert np.count_nonzero(ref["vals"].reshape(3, 4, 8)[:, 2]) == 0            # the values carry value = 0
    assert np.count_nonzero(ref["dgamma"][2]) == 0                              # xhat of a zero row is zero
    _, xn, dt, dg, _ = MR.input_stage_torch_grads(table, X, values, gamma, beta, dn, dn, torch.float32)
    assert np.isfinite(xn).all() and np.isfinite(dt).all() and np.isfinite(dg).all()


def test_header_declares_the_entry_points_and_limits_and_the_library_exports_them():
    from explicit_tf2_recommendation_amd import _lib
    with open(_lib.HEADER_PATH) as f:
        text = _lib.strip_comments(f.read())
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name) is not None
    for k, v in LIMITS.items():
        assert _lib.LIMITS["REC_MASKNET_MAX_" + k] >= v
    assert _lib.ENUMS["REC_EPI_ADD"] == 6 and _lib.ENUMS["REC_DACT_PRELU"] == 5 and _lib.ENUMS["REC_ACT_NONE"] == 0
    assert _lib.SIGNATURES["rec_masknet_ln_workspace_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["rec_mask_block_bwd_f32"][1]) == 31
    from explicit_tf2_recommendation_amd import ops
    assert (ops.MASKNET_MAX_F, ops.MASKNET_MAX_E, ops.MASKNET_MAX_D, ops.MASKNET_MAX_P, ops.MASKNET_MAX_O,
            ops.MASKNET_MAX_R) == tuple(_lib.LIMITS["REC_MASKNET_MAX_" + k] for k in "FEDPOR")


def test_abi_rejects_bad_arguments_without_a_gpu():
    from explicit_tf2_recommendation_amd._lib import lib, LIMITS as L
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    MF, ME, MD, MP, MO, MR_ = (L["REC_MASKNET_MAX_" + k] for k in "FEDPOR")

    def lf(tab=d, V=100, E=16, ld=16, X=d, val=d, B=4, F=13, Fk=3, g=d, b=d, xe=d, xn=d, st=d):
        return lib.rec_emb_masknet_ln_fwd_f32(tab, V, E, ld, X, val, B, F, Fk, g, b, xe, xn, st, None, None)

    def lb(xe=d, st=d, val=d, g=d, dn=d, de=d, B=4, F=13, Fk=3, E=16, vals=d, dg=d, db=d, ws=d, nbytes=1 << 30):
        return lib.rec_emb_masknet_ln_bwd_f32(xe, st, val, g, dn, de, B, F, Fk, E, vals, dg, db, ws, nbytes, None)

    def bf(B=4, D=208, P=208, O=32, R=3, y=d, save=(d, d, d, d), x=d):
        return lib.rec_mask_block_fwd_f32(x, d, d, d, d, d, d, d, d, d, B, D, P, O, R, y, *save, None)

    def bb(B=4, D=208, P=208, O=32, R=3, dv=d, ws=d, nbytes=1 << 30):
        return lib.rec_mask_block_bwd_f32(d, d, d, d, d, d, d, d, d, d, d, d, B, D, P, O, R, dv, d, 0, d, d, d, d, d, d, d,
                                          d, ws, nbytes, None)

    for k in ("tab", "X", "val", "g", "b", "xe", "xn", "st"):
        assert lf(**{k: None}) == -1, k
    for k in ("xe", "st", "val", "g", "dn", "vals", "dg", "db", "ws"):
        assert lb(**{k: None}) == -1, k
    assert lf(B=-1) == -1 and lf(F=0) == -1 and lf(E=0) == -1 and lf(Fk=14) == -1 and lf(Fk=-1) == -1
    assert lf(V=0) == -1 and lf(ld=8) == -1 and lb(B=-1) == -1 and lb(Fk=14) == -1
    assert lf(F=MF + 1) == -2 and lf(E=ME + 1, ld=ME + 1) == -2 and lb(F=MF + 1) == -2 and lb(E=ME + 1) == -2
    assert lf(B=0, tab=None, X=None, val=None, g=None, b=None, xe=None, xn=None, st=None) == 0
    assert lb(B=0, xe=None, st=None, val=None, g=None, dn=None, de=None, vals=None, dg=None, db=None, ws=None) == 0
    assert lb(nbytes=16) == -3
    assert lib.rec_masknet_ln_workspace_bytes(4, 13, 16) > 0 and lib.rec_masknet_ln_workspace_bytes(4, MF, ME) > 0
    assert lib.rec_masknet_ln_workspace_bytes(4, MF + 1, 16) == 0 and lib.rec_masknet_ln_workspace_bytes(-1, 13, 16) == 0

    assert bf(x=None) == -1 and bf(y=None) == -1 and bf(save=(d, None, d, d)) == -1 and bb(dv=None) == -1
    assert bb(ws=None) == -1 and bf(B=-1) == -1 and bf(D=0) == -1 and bf(R=0) == -1 and bb(O=0) == -1
    assert bf(D=MD + 1) == -2 and bf(P=MP + 1) == -2 and bf(O=MO + 1) == -2 and bf(R=MR_ + 1) == -2
    assert bb(D=MD + 1) == -2 and bb(P=MP + 1) == -2 and bb(O=MO + 1) == -2 and bb(R=MR_ + 1) == -2
    assert bf(B=0) == 0 and bb(B=0, ws=None) == 0 and bb(nbytes=16) == -3
    ws = lib.rec_masknet_block_workspace_bytes
    assert ws(4, MD + 1, 208, 32, 3) == 0 and ws(4, 208, 208, 32, MR_ + 1) == 0 and ws(-1, 208, 208, 32, 3) == 0
    # per example 4 (R P + 2 P + O) bytes, the tiles' slots, and weight-sized terms that do not grow with the batch
    D, P, O, R = 208, 208, 32, 3
    per = 4 * (R * P + 2 * P + O)
    w1, w2 = ws(8192, D, P, O, R), ws(16384, D, P, O, R)
    assert 8192 * per < w1 and w2 - w1 < 8192 * (per + 4 * (3 * O + P + R * P) // 32 + 64)
    assert w1 - 8192 * per <= 4 * 16 * D * R * P + 8192 * 4 * (3 * O + P + R * P) // 32 + 4096
    assert ws(17, MD, MP, MO, MR_) > 0 and ws(1, 1, 1, 1, 1) > 0


def test_ops_guards_raise_before_any_launch():
    from explicit_tf2_recommendation_amd import ops
    ops.masknet_ln_check_shape(13, 16, 3)
    ops.masknet_ln_check_shape(64, 64, 0)
    ops.mask_block_check_shape(512, 512, 128, 4)
    for args in ((0, 16, 0), (13, 0, 0), (13, 16, 14), (13, 16, -1)):
        with pytest.raises(ValueError):
            ops.masknet_ln_check_shape(*args)
    for args in ((65, 16, 0), (13, 65, 3)):
        with pytest.raises(NotImplementedError):
            ops.masknet_ln_check_shape(*args)
    with pytest.raises(ValueError):
        ops.mask_block_check_shape(208, 0, 32, 3)
    for args in ((513, 208, 32, 3), (208, 513, 32, 3), (208, 208, 129, 3), (208, 208, 32, 5)):
        with pytest.raises(NotImplementedError):
            ops.mask_block_check_shape(*args)
    # there is no CPU path: CPU tensors are refused before anything else
    t = torch.zeros(4, 16)
    with pytest.raises(RuntimeError):
        ops.emb_masknet_ln_fwd(torch.zeros(10, 4), torch.zeros(4, 4, dtype=torch.int64), None, t, t)
    with pytest.raises(RuntimeError):
        ops.mask_block_fwd(t, t, t, t, t, t, t, t, t, t)
    with pytest.raises(RuntimeError):
        ops.mask_block_bwd(t, t, t, t, t, t, t, (t, t, t, t), t)
    with pytest.raises(RuntimeError):
        ops.emb_masknet_ln_bwd(t, t, None, t, t)


def test_signatures_keep_the_reference_keywords():
    """11.FiBiNet++/CustomLayers.py:246-249, :314, :323, :341-345, :368-372, :389-393."""
    from explicit_tf2_recommendation_amd import layers as CL
    sig = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())]
    common = [("categorical_features", CAT), ("continuous_features", CONT), ("feature_dims", 160000),
              ("embedding_dims", 16)]
    assert sig(CL.LayerNormInputFeaturesEmbeddingLayer.__init__)[1:] == common
    stack = common + [("block_output_dim", 32), ("block_num", 6)]
    assert sig(CL.SerialMaskNetLayer.__init__)[1:] == stack and sig(CL.ParralledMaskNetLayer.__init__)[1:] == stack
    assert sig(CL.MaskNetLayer.__init__)[1:] == stack + [("stacking_mode", "serial"), ("final_mlp_units", [32])]
    assert sig(CL.MaskBlockLayer.__init__)[1:] == [("fields_num", 13), ("input_type", "feature"), ("embedding_dims", 16),
                                                   ("block_output_dim", 32)]
    assert sig(CL.make_instance_guided_mask)[:2] == [("output_dim", inspect.Parameter.empty), ("reduction_rate", 3)]
    assert "not reference behaviour" in " ".join(CL.ParralledMaskNetLayer.__doc__.lower().split())


def _block_shapes(prefix, D, P, O):
    return {prefix + "instance_guided_mask.layers.0.kernel": (D, 3 * P), prefix + "instance_guided_mask.layers.0.bias": (3 * P,),
            prefix + "instance_guided_mask.layers.2.kernel": (3 * P, P), prefix + "instance_guided_mask.layers.2.bias": (P,),
            prefix + "ln_hid.layers.0.kernel": (P, O), prefix + "ln_hid.layers.0.bias": (O,),
            prefix + "ln_hid.layers.1.gamma": (O,), prefix + "ln_hid.layers.1.beta": (O,)}


def test_both_stacking_modes_produce_the_documented_parameter_shapes():
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.MaskNetLayer(feature_dims=100)
    assert isinstance(lay.mask_net, CL.SerialMaskNetLayer)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    want = {"mask_net.norm_embedding_layer.embedding_layer.embeddings": (100, 16),
            "final_mlp.layers.0.kernel": (32, 32), "final_mlp.layers.0.bias": (32,), "final_mlp.layers.1.alpha": (32,),
            "final_mlp.layers.2.kernel": (32, 1), "final_mlp.layers.2.bias": (1,)}
    for f in range(13):
        want["mask_net.norm_embedding_layer.emb_layernorm_list.%d.gamma" % f] = (16,)
        want["mask_net.norm_embedding_layer.emb_layernorm_list.%d.beta" % f] = (16,)
    want.update(_block_shapes("mask_net.mask_block_on_feature.", 208, 208, 32))
    for k in range(5):
        want.update(_block_shapes("mask_net.mask_block_on_block_list.%d." % k, 208, 32, 32))
    assert shapes == want
    emb = lay.mask_net.norm_embedding_layer
    assert emb.continuous_features_keys == [c + "_key" for c in CONT]
    assert emb.continuous_features_values == [c + "_value" for c in CONT]
    amax = lambda t: float(t.detach().abs().max())
    blk = lay.mask_net.mask_block_on_feature
    assert 0 < amax(blk.instance_guided_mask.layers[0].kernel) <= np.sqrt(6.0 / (208 + 624))
    assert amax(blk.ln_hid.layers[0].bias) == 0 and amax(emb.emb_layernorm_list[3].gamma) == 1.0

    lay = CL.MaskNetLayer(categorical_features=CAT[:4], continuous_features=CONT[:1], feature_dims=50, embedding_dims=8,
                          block_output_dim=7, block_num=2, stacking_mode="parallel", final_mlp_units=[5, 3])
    assert isinstance(lay.mask_net, CL.ParralledMaskNetLayer)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    want = {"mask_net.norm_embedding_layer.embedding_layer.embeddings": (50, 8),
            "final_mlp.layers.0.kernel": (14, 5), "final_mlp.layers.0.bias": (5,), "final_mlp.layers.1.alpha": (5,),
            "final_mlp.layers.2.kernel": (5, 3), "final_mlp.layers.2.bias": (3,), "final_mlp.layers.3.alpha": (3,),
            "final_mlp.layers.4.kernel": (3, 1), "final_mlp.layers.4.bias": (1,)}
    for f in range(5):
        want["mask_net.norm_embedding_layer.emb_layernorm_list.%d.gamma" % f] = (8,)
        want["mask_net.norm_embedding_layer.emb_layernorm_list.%d.beta" % f] = (8,)
    for k in range(2):
        want.update(_block_shapes("mask_net.mask_block_on_feature_list.%d." % k, 40, 40, 7))
    assert shapes == want
    with pytest.raises(NotImplementedError):
        CL.MaskNetLayer(feature_dims=10, embedding_dims=40)                    # D = 520
    with pytest.raises(NotImplementedError):
        CL.MaskNetLayer(feature_dims=10, block_output_dim=129)
    with pytest.raises(ValueError):
        CL.MaskNetLayer(feature_dims=10, block_num=0)


def test_model_manager_builds_masknet_and_honours_model_params():
    from explicit_tf2_recommendation_amd import data, layers as CL
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(5000, len(CAT)),
                      embedding_dims=16, layer="MaskNet", device="cpu")
    lay = mm.layer
    assert isinstance(lay, CL.MaskNetLayer) and isinstance(lay.mask_net, CL.SerialMaskNetLayer)
    assert lay.categorical_features == CAT and lay.continuous_features_keys == [c + "_key" for c in CONT]
    assert tuple(lay.mask_net.norm_embedding_layer.embedding_layer.embeddings.shape) == (mm.feature_dims, 16)
    assert len(lay.mask_net.mask_block_on_block_list) == 5 and lay.mask_net.block_output_dim == 32
    mm2 = ModelManager(feature_names=CAT[:5], continuous_features=CONT[:2], data_info=data.data_info(5000, 5),
                       embedding_dims=8, layer="MaskNet", device="cpu",
                       model_params={"block_output_dim": 12, "block_num": 3, "stacking_mode": "parallel",
                                     "final_mlp_units": [6]})
    net = mm2.layer.mask_net
    assert isinstance(net, CL.ParralledMaskNetLayer) and len(net.mask_block_on_feature_list) == 3
    assert tuple(net.mask_block_on_feature_list[2].ln_hid.layers[0].kernel.shape) == (56, 12)
    assert tuple(mm2.layer.final_mlp.layers[0].kernel.shape) == (36, 6)
    # batches for it come from the existing generator: the key columns are categorical, the values continuous
    gen = data.SyntheticGenerator(CAT + [c + "_key" for c in CONT], 5000, continuous=[c + "_value" for c in CONT])
    b = gen.batch(4)
    assert b["itag4_square_key"].dtype == np.int64 and b["itag4_square_value"].dtype == np.float32


def test_the_dx_emb_sink_hands_on_once_rearms_and_refuses_an_incomplete_pass():
    from explicit_tf2_recommendation_amd import functional as Fn
    sink = Fn.MaskDxSink(3)
    add = lambda buf: 1 if buf is None else buf + 1
    assert [sink.add(k, add) for k in "abc"] == [None, None, 3]
    assert [sink.add(k, add) for k in "cba"] == [None, None, 3]        # a second backward starts from a fresh buffer
    assert sink.add("a", add) is None
    with pytest.raises(RuntimeError):
        sink.add("a", add)                                              # a block again before the others: one was cut out
