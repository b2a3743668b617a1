"""CPU checks of ContextNet: the numpy and torch restatements against each other in fp64 (tests/contextnet_ref.py), the
layers' constructor keywords against the reference signature, the state-dict keys in both modes,
ModelManager(layer='ContextNet'), and the C-ABI status codes and the ops.py guards without a GPU.  The limits are
MaskNet's: the header has no constant of this family's own."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import contextnet_ref as CR

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
ENTRY_POINTS = ["rec_emb_contextnet_in_fwd_f32", "rec_emb_contextnet_in_bwd_f32", "rec_contextnet_block_workspace_bytes",
                "rec_contextnet_block_fwd_f32", "rec_contextnet_block_bwd_f32"]
MODES = ["pointwise", "single"]


def close(got, want):
    """1e-12 of the tensor's largest magnitude, or of 1 where that is smaller: with E = 1 the LayerNorm makes whole
    gradients exactly zero in the hand-written backward and rounding residue (1e-17) in autograd"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= 1e-12 * max(float(np.abs(want).max()) if want.size else 0.0, 1.0), err


@pytest.mark.parametrize("B,Fc,Fk,E", [(1, 1, 0, 1), (2, 1, 1, 3), (5, 10, 3, 16), (3, 0, 2, 5)])
def test_input_stage_restatements_agree(B, Fc, Fk, E):
    r = np.random.default_rng(B * 10 + Fc)
    table, X, values = CR.make_input(r, B, Fc, Fk, E, 7)
    dx = r.uniform(-1, 1, (B, (Fc + Fk) * E))
    ref = CR.input_stage_numpy(table, X, values, dx)
    x, dt = CR.input_stage_torch_grads(table, X, values, dx, torch.float64)
    close(x, ref["x"])
    close(dt, ref["dtable"])
    scale = np.concatenate([np.ones((B, Fc)), values], 1)
    close(ref["vals"], (dx.reshape(B, Fc + Fk, E) * scale[:, :, None]).reshape(-1, E))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,F,E,R", [(1, 1, 1, 1), (2, 3, 5, 2), (5, 13, 10, 3), (4, 7, 33, 1), (3, 64, 1, 3)])
def test_block_backward_equals_fp64_autograd(B, F, E, R, mode):
    r = np.random.default_rng(B + F)
    params = CR.make_block(r, F, E, R, mode)
    assert len(params) == (8 if mode == "pointwise" else 7)
    x, dy = r.normal(0, 1, (B, F * E)), r.uniform(-1, 1, (B, F * E))
    ref = CR.block_numpy(x, params, mode, dy)
    y, dx, dp = CR.block_torch_grads(x, params, mode, dy, torch.float64)
    close(y, ref["y"])
    close(dx, ref["dx"])
    assert len(dp) == len(ref["dparams"])
    for got, want in zip(dp, ref["dparams"]):
        assert got.shape == want.shape
        close(got, want)
    assert ref["pre"].shape == (B,) and (ref["pre"] >= 0).all()


@pytest.mark.parametrize("mode,NB", [("pointwise", 2), ("single", 3), ("pointwise", 1)])
def test_layer_backward_equals_fp64_autograd(mode, NB):
    r = np.random.default_rng(NB)
    B, Fc, Fk, E = 6, 3, 2, 4
    table, X, values = CR.make_input(r, B, Fc, Fk, E, 9)
    blocks = [CR.make_block(r, Fc + Fk, E, 3, mode) for _ in range(NB)]
    head = CR.make_head(r, (Fc + Fk) * E, 4)
    dout = r.uniform(-1, 1, (B, 1))
    ref = CR.contextnet_numpy(table, X, values, blocks, head, mode, dout)
    out, dt, dbl, dh = CR.contextnet_torch_grads(table, X, values, blocks, head, mode, dout, torch.float64)
    assert ref["output"].shape == (B, 1)
    close(out, ref["output"])
    pairs = [(dt, ref["dtable"])] + list(zip(dh, ref["dhead"]))
    for k in range(NB):
        pairs += list(zip(dbl[k], ref["dblocks"][k]))
    for got, want in pairs:
        close(got, want)


def test_the_residual_is_the_masked_input_and_single_mode_has_no_second_matrix():
    r = np.random.default_rng(2)
    F, E = 2, 3
    p = CR.make_block(r, F, E, 2, "pointwise")
    p[4] = np.zeros((F, E, E))                              # a = 0: r = u, so y = LN(x * m)
    x = r.normal(0, 1, (4, F * E))
    Wa, ba, Wb, bb = p[:4]
    u = (x * (np.maximum(x @ Wa + ba, 0) @ Wb + bb)).reshape(4, F, E)
    close(CR.block_numpy(x, p)["y"], CR._ln(u, p[6], p[7])[0].reshape(4, -1))
    ps = CR.make_block(r, F, E, 2, "single")
    ps[4] = np.stack([np.eye(E)] * F)                       # single with W1 = I: the same
    ps[:4] = p[:4]
    close(CR.block_numpy(x, ps, "single")["y"], CR._ln(u, ps[5], ps[6])[0].reshape(4, -1))


def test_signatures_keep_the_reference_keywords():
    """11.FiBiNet++/CustomLayers.py:413, :429, :450, :475-479."""
    from explicit_tf2_recommendation_amd import layers as CL
    sig = lambda f: [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())]
    assert sig(CL.ContextNetLayer.__init__)[1:] == [
        ("categorical_features", CAT), ("continuous_features", CONT), ("feature_dims", 160000), ("embedding_dims", 16),
        ("block_num", 6), ("final_mlp_units", [32]), ("nonlinear_type", "pointwise")]
    assert sig(CL.ContextualEmbeddingLayer.__init__)[1:] == [("fields_num", 13), ("embedding_dims", 16)]
    assert sig(CL.NonLinearFeedforwardLayer.__init__)[1:] == [("embedding_dims", 16), ("mode", "pointwise")]
    # the reference builds the block lazily; fields_num and embedding_dims are the documented extension
    assert sig(CL.ContextNetBlockLayer.__init__)[1:] == [("nonlinear_type", "pointwise"), ("fields_num", 13),
                                                         ("embedding_dims", 16)]
    assert "extension" in CL.ContextNetBlockLayer.__doc__
    for name in ("ContextualEmbeddingLayer", "NonLinearFeedforwardLayer", "ContextNetBlockLayer", "ContextNetLayer"):
        assert name in CL.__doc__


@pytest.mark.parametrize("mode", MODES)
def test_state_dict_keys_read_like_the_reference_s(mode):
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.ContextNetLayer(feature_dims=100, block_num=2, nonlinear_type=mode)
    shapes = {k: tuple(v.shape) for k, v in lay.state_dict().items()}
    want = {"embedding_layer.embeddings": (100, 16), "final_mlp.layers.0.kernel": (208, 32),
            "final_mlp.layers.0.bias": (32,), "final_mlp.layers.1.alpha": (32,), "final_mlp.layers.2.kernel": (32, 1),
            "final_mlp.layers.2.bias": (1,)}
    for k in range(2):
        ce = "context_block_list.%d.ce_layer.contextual_embedding_transform.layers." % k
        want.update({ce + "0.kernel": (208, 624), ce + "0.bias": (624,), ce + "2.kernel": (624, 208),
                     ce + "2.bias": (208,)})
        for f in range(13):
            nl = "context_block_list.%d.nonlinear_layer_list.%d." % (k, f)
            want.update({nl + "W1": (16, 16), nl + "ln.gamma": (16,), nl + "ln.beta": (16,)})
            if mode == "pointwise":
                want[nl + "W2"] = (16, 16)
    assert shapes == want
    assert not any(k.endswith("W2") for k in shapes) or mode == "pointwise"
    assert lay.continuous_features_keys == [c + "_key" for c in CONT]
    assert lay.continuous_features_values == [c + "_value" for c in CONT]
    assert len(lay.context_block_list) == 2 and lay.embedding_layer is not None and lay.final_mlp is not None
    W1 = lay.context_block_list[0].nonlinear_layer_list[3].W1.detach()
    sd = np.sqrt(2.0 / 32) / 0.87962566                     # glorot-normal, truncated at two sigma
    assert 0 < float(W1.abs().max()) <= 2 * sd + 1e-6 and float(W1.std()) < sd
    with pytest.raises(NotImplementedError):
        CL.ContextNetLayer(feature_dims=10, embedding_dims=40)                  # F E = 520
    with pytest.raises(ValueError):
        CL.ContextNetLayer(feature_dims=10, block_num=0)


def test_model_manager_builds_contextnet_and_honours_model_params():
    from explicit_tf2_recommendation_amd import data, layers as CL
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(5000, len(CAT)),
                      embedding_dims=16, layer="ContextNet", device="cpu")
    mm.make_layer_choice("ContextNet", {})
    lay = mm.layer
    assert isinstance(lay, CL.ContextNetLayer) and len(lay.context_block_list) == 6
    assert lay.categorical_features == CAT and lay.continuous_features_keys == [c + "_key" for c in CONT]
    assert tuple(lay.embedding_layer.embeddings.shape) == (mm.feature_dims, 16)
    assert lay.context_block_list[0].nonlinear_type == "pointwise"
    mm2 = ModelManager(feature_names=CAT[:5], continuous_features=CONT[:2], data_info=data.data_info(5000, 5),
                       embedding_dims=8, layer="ContextNet", device="cpu",
                       model_params={"block_num": 3, "final_mlp_units": [6], "nonlinear_type": "single"})
    lay = mm2.layer
    assert len(lay.context_block_list) == 3 and lay.context_block_list[2].nonlinear_type == "single"
    assert not hasattr(lay.context_block_list[2].nonlinear_layer_list[0], "W2")
    assert tuple(lay.final_mlp.layers[0].kernel.shape) == (56, 6)


def test_header_declares_the_entry_points_and_adds_no_constant():
    from explicit_tf2_recommendation_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.SIGNATURES["rec_contextnet_block_workspace_bytes"] == (C.c_size_t, [C.c_int64] + [C.c_int] * 4)
    assert len(_lib.SIGNATURES["rec_contextnet_block_fwd_f32"][1]) == 21
    assert len(_lib.SIGNATURES["rec_contextnet_block_bwd_f32"][1]) == 29
    assert not [k for k in list(_lib.LIMITS) + list(_lib.ENUMS) if "CONTEXT" in k.upper()]


SUPPORTED = [(64, 8, 4), (8, 64, 4), (1, 1, 1)]
UNSUPPORTED = [(27, 19, 3), (65, 1, 3), (1, 65, 3), (13, 16, 5)]           # F E = 513, F = 65, E = 65, R = 5


def test_abi_status_codes_without_a_gpu():
    from explicit_tf2_recommendation_amd._lib import lib
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    ws = lib.rec_contextnet_block_workspace_bytes

    def bf(B=4, F=13, E=16, R=3, pw=1, x=d, W2=d, y=d, save=(d, d, d, d, d)):
        return lib.rec_contextnet_block_fwd_f32(x, d, d, d, d, d, W2, d, d, B, F, E, R, pw, y, *save, None)

    def bb(B=4, F=13, E=16, R=3, pw=1, a=d, dx=d, dW2=d, ws_=d, nbytes=1 << 30):
        return lib.rec_contextnet_block_bwd_f32(d, d, d, d, d, d, d, d, d, d, a, d, B, F, E, R, pw, dx, d, d, d, d, d,
                                                dW2, d, d, ws_, nbytes, None)

    def inf(tab=d, V=100, E=16, ld=16, X=d, val=d, B=4, F=13, Fk=3, x=d):
        return lib.rec_emb_contextnet_in_fwd_f32(tab, V, E, ld, X, val, B, F, Fk, x, None, None)

    def inb(val=d, dx=d, B=4, F=13, Fk=3, E=16, vals=d):
        return lib.rec_emb_contextnet_in_bwd_f32(val, dx, B, F, Fk, E, vals, None)

    for F, E, R in SUPPORTED:
        for pw in (0, 1):
            assert ws(17, F, E, R, pw) > 0
            assert bf(B=0, F=F, E=E, R=R, pw=pw) == 0 and bb(B=0, F=F, E=E, R=R, pw=pw, ws_=None) == 0
    for F, E, R in UNSUPPORTED:
        assert ws(17, F, E, R, 1) == 0 and ws(17, F, E, R, 0) == 0
        assert bf(B=0, F=F, E=E, R=R) == -2 and bf(F=F, E=E, R=R) == -2 and bb(F=F, E=E, R=R) == -2
    assert ws(-1, 13, 16, 3, 1) == 0 and ws(4, 13, 16, 3, 2) == 0 and ws(4, 0, 16, 3, 1) == 0
    assert bf(x=None) == -1 and bf(y=None) == -1 and bf(W2=None) == -1
    assert bf(save=(d, None, d, d, d)) == -1 and bf(save=(d, d, d, d, None)) == -1
    assert bf(B=-1) == -1 and bf(F=0) == -1 and bf(E=-3) == -1 and bf(R=0) == -1 and bf(pw=2) == -1 and bf(pw=-1) == -1
    assert bb(dx=None) == -1 and bb(a=None) == -1 and bb(dW2=None) == -1 and bb(ws_=None) == -1 and bb(B=-1) == -1
    assert bb(nbytes=16) == -3
    # per example 4 (R D + 4 D) bytes in pointwise mode, one D less in single; the rest does not grow with the batch
    F, E, R = 13, 16, 3
    D = F * E
    w1, w2 = ws(8192, F, E, R, 1), ws(16384, F, E, R, 1)
    per = 4 * (R * D + 4 * D)
    assert 8192 * per < w1 and w2 - w1 < 8192 * (per + 4 * (3 * D + R * D) // 32 + 64)
    assert w1 - ws(8192, F, E, R, 0) >= 8192 * 4 * D

    for k in ("tab", "X", "val", "x"):
        assert inf(**{k: None}) == -1, k
    for k in ("val", "dx", "vals"):
        assert inb(**{k: None}) == -1, k
    assert inf(B=-1) == -1 and inf(F=0) == -1 and inf(Fk=14) == -1 and inf(V=0) == -1 and inf(ld=8) == -1
    assert inf(F=65) == -2 and inf(E=65, ld=65) == -2 and inb(F=65) == -2 and inb(E=65) == -2 and inb(Fk=-1) == -1
    assert inf(F=27, E=19, ld=19) == -2 and inb(F=27, E=19) == -2           # F E = 513: the family's limit, here too
    assert inf(B=0, F=27, E=19, ld=19) == -2 and inf(B=0, F=64, E=8, ld=8) == 0 and inb(B=0, F=8, E=64) == 0
    assert inf(B=0, tab=None, X=None, val=None, x=None) == 0 and inb(B=0, val=None, dx=None, vals=None) == 0


def test_ops_guards_raise_before_any_launch():
    from explicit_tf2_recommendation_amd import ops
    for F, E, R in SUPPORTED + [(13, 16, 3)]:
        ops.contextnet_check_shape(F, E, R)
    for (F, E, R), word in zip(UNSUPPORTED, ("512", "64", "64", "4")):
        with pytest.raises(NotImplementedError, match=word):
            ops.contextnet_check_shape(F, E, R)
    with pytest.raises(NotImplementedError, match=r"fields \* embedding_dims <= 512"):
        ops.contextnet_check_shape(27, 19, 3)
    for args in ((0, 16, 3), (13, 0, 3), (13, 16, 0), (13, 16, 3, 14), (13, 16, 3, -1)):
        with pytest.raises(ValueError):
            ops.contextnet_check_shape(*args)
    # there is no CPU path: CPU tensors are refused before anything else
    t, w = torch.zeros(4, 16), torch.zeros(1, 16, 16)
    with pytest.raises(RuntimeError):
        ops.emb_contextnet_in_fwd(torch.zeros(10, 4), torch.zeros(4, 4, dtype=torch.int64), None)
    with pytest.raises(RuntimeError):
        ops.emb_contextnet_in_bwd(t, None, 1)
    with pytest.raises(RuntimeError):
        ops.contextnet_block_fwd(t, t, t, t, t, w, w, t, t)
    with pytest.raises(RuntimeError):
        ops.contextnet_block_bwd(t, t, t, w, w, t, (t, t, t, t, t), t)
