"""CPU checks of the AutoInt layer: the reference's keywords and parameter names, TF2 TruncatedNormal, the head column
split and the continuous-fields-last layout pinned by the restatements (tests/autoint_ref.py), the C-ABI status codes
of the AutoInt entry points without a GPU, and ModelManager(layer='AutoInt')."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import autoint_ref as AR

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


def test_signatures_keep_the_reference_keywords():
    """3.DCN/CustomLayers.py:1013 and :1084-1088."""
    from explicit_tf2_recommendation_amd import layers as CL
    params = list(inspect.signature(CL.AutoIntLayer.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["categorical_features", "continuous_features", "feature_dims",
                                        "embedding_dims", "units", "activation", "attention_layer_num", "num_heads"]
    d = {p.name: p.default for p in params}
    assert d["categorical_features"] == CAT and d["continuous_features"] == CONT
    assert (d["feature_dims"], d["embedding_dims"], d["units"], d["activation"], d["attention_layer_num"],
            d["num_heads"]) == (160000, 8, [128, 16], "relu", 2, 2)
    params = list(inspect.signature(CL.TransformerAttentionLayer.__init__).parameters.values())[1:5]
    assert [(p.name, p.default) for p in params] == [("num_heads", 2), ("use_res", True), ("res_learnable", False),
                                                     ("scaling", False)]


def test_parameter_names_and_shapes():
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.AutoIntLayer(feature_dims=100)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    F, E = 13, 8
    want = {"embedding_layer.embeddings": (100, E), "continuous_embedding.embeddings": (3, E),
            "dnn_layer.kernel_0": (F * E, 128), "dnn_layer.bias_0": (128,),
            "dnn_layer.kernel_1": (128, 16), "dnn_layer.bias_1": (16,),
            "output_layer.kernel": (16, 1), "output_layer.bias": (1,)}
    for k in range(2):
        want.update({"attention_layers.%d.%s" % (k, n): (E, E) for n in ("query", "key", "value")})
    assert shapes == want
    assert set(lay.state_dict()) == set(want)
    t = CL.TransformerAttentionLayer(num_heads=4, res_learnable=True, input_dim=16)
    assert {k: tuple(v.shape) for k, v in t.named_parameters()} == {n: (16, 16) for n in ("query", "key", "value",
                                                                                          "res")}
    assert t.att_embedding_size == 4 and t.res_code == 2
    assert CL.TransformerAttentionLayer(use_res=False, res_learnable=True, input_dim=8).res_code == 0
    assert not hasattr(CL.TransformerAttentionLayer(use_res=False, res_learnable=True, input_dim=8), "res")


def test_truncated_normal_is_tf2s():
    """Keras TruncatedNormal(): mean 0, stddev 0.05, redrawn beyond 2 stddev (so the draws' stddev is 0.05 x 0.8796)."""
    from explicit_tf2_recommendation_amd import layers as CL
    CL.set_init_seed(3)
    w = CL.truncated_normal((400, 16, 16)).double()
    assert float(w.abs().max()) <= 0.1
    assert abs(float(w.std()) - 0.05 * 0.87962566103423978) < 0.01 * 0.05
    assert abs(float(w.mean())) < 0.002
    assert float((w.abs() > 0.09).double().mean()) > 0.01            # truncated, not clipped or rescaled to 1 sigma
    CL.set_init_seed(3)
    assert torch.equal(CL.truncated_normal((400, 16, 16)).double(), w)
    assert CL._initializer("truncated_normal") is CL.truncated_normal


def test_heads_that_do_not_divide_the_embedding_are_rejected():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(ValueError):
        CL.AutoIntLayer(feature_dims=100, embedding_dims=8, num_heads=3)
    with pytest.raises(ValueError):
        CL.TransformerAttentionLayer(num_heads=3, input_dim=8)
    with pytest.raises(NotImplementedError):
        CL.AutoIntLayer(feature_dims=100, embedding_dims=65, num_heads=1)
    with pytest.raises(NotImplementedError):
        CL.AutoIntLayer(categorical_features=["c%d" % i for i in range(62)], feature_dims=100)


def _rand(B, F, E, seed, learn=False):
    r = np.random.default_rng(seed)
    X = r.standard_normal((B, F, E))
    Ws = [r.standard_normal((E, E)) / np.sqrt(E) for _ in range(4)]
    return X, Ws


@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("B,F,E,H", [(5, 4, 6, 2), (3, 13, 8, 2), (7, 3, 4, 4), (2, 5, 6, 1), (1, 4, 4, 2)])
def test_restatements_agree_on_values_and_gradients(B, F, E, H, res, scaling):
    X, (Wq, Wk, Wv, Wr) = _rand(B, F, E, seed=B * 7 + F + res)
    y_np, o_np = AR.attention_numpy(X, Wq, Wk, Wv, H, res, Wr, scaling)
    t = [torch.from_numpy(a).requires_grad_() for a in (X, Wq, Wk, Wv, Wr)]
    y1, o1 = AR.attention_torch(t[0], t[1], t[2], t[3], H, use_res=res > 0, res_learnable=res == 2, Wres=t[4],
                                scaling=scaling, return_o=True)
    np.testing.assert_allclose(y1.detach().numpy(), y_np, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(o1.detach().numpy(), o_np, rtol=1e-12, atol=1e-14)
    gout = torch.from_numpy(np.random.default_rng(1).standard_normal(y1.shape))
    g1 = torch.autograd.grad(y1, t, gout, allow_unused=True)
    t2 = [a.detach().clone().requires_grad_() for a in t]
    y2 = AR.attention_einsum(t2[0], t2[1], t2[2], t2[3], H, res, t2[4], scaling)
    np.testing.assert_allclose(y2.detach().numpy(), y_np, rtol=1e-12, atol=1e-14)
    g2 = torch.autograd.grad(y2, t2, gout, allow_unused=True)
    for a, b in zip(g1, g2):
        if a is None or b is None:
            assert a is None and b is None or float((a if a is not None else b).abs().max()) == 0
            continue
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-12)


def test_head_column_split_is_pinned():
    """Head h owns the columns [h d, (h+1) d): with Wq = Wk = Wv = I and H = 2, head 0's scores use only x[:, :, :2]."""
    B, F, E, H = 3, 2, 4, 2
    X = np.arange(B * F * E, dtype=np.float64).reshape(B, F, E) / 10
    I = np.eye(E)
    _, o = AR.attention_numpy(X, I, I, I, H, 0)
    for h in range(H):
        c = slice(2 * h, 2 * h + 2)
        S = np.einsum("bic,bjc->bij", X[:, :, c], X[:, :, c])
        P = np.exp(S - S.max(0)) / np.exp(S - S.max(0)).sum(0)
        np.testing.assert_allclose(o[:, :, c], np.einsum("bij,bjc->bic", P, X[:, :, c]), rtol=1e-12)
    # interleaved columns (a wrong split) give other numbers
    perm = [0, 2, 1, 3]
    _, o_wrong = AR.attention_numpy(X[:, :, perm], I, I, I, H, 0)
    assert np.abs(o_wrong[:, :, np.argsort(perm)] - o).max() > 1e-3


def test_softmax_runs_over_the_batch_axis():
    B, F, E, H = 4, 3, 4, 2
    X, (Wq, Wk, Wv, _) = _rand(B, F, E, seed=2)
    _, o = AR.attention_numpy(X, Wq, Wk, Wv, H, 0)
    t = [torch.from_numpy(a) for a in (X, Wq, Wk, Wv)]
    key = AR.attention_keyaxis(*t, H).numpy()
    assert np.abs(key - o).max() > 0.1 * np.abs(o).max()
    # one example's output changes when another example of the batch changes
    X2 = X.copy()
    X2[3] += 1.0
    _, o2 = AR.attention_numpy(X2, Wq, Wk, Wv, H, 0)
    assert np.abs(o2[0] - o[0]).max() > 1e-6


def test_continuous_fields_come_last_on_the_reference_main_input():
    """The reference's docstring input (ids 0 .. 29, three continuous columns): X_emb rows 10 .. 12 are
    cemb[c] * x_cont[:, c]; the restatements agree on the whole layer, values and gradients."""
    names, X_cate, X_cont = AR.reference_main_input()
    assert X_cate[:, 0].tolist() == [0, 1, 2] and X_cate[:, 9].tolist() == [27, 28, 29]
    r = np.random.default_rng(4)
    E = 8
    embed = torch.from_numpy(r.uniform(-0.05, 0.05, (30, E))).requires_grad_()
    cemb = torch.from_numpy(r.uniform(-0.05, 0.05, (3, E))).requires_grad_()
    x = AR.assemble(embed, torch.from_numpy(X_cate), cemb, torch.from_numpy(X_cont))
    assert x.shape == (3, 13, E)
    np.testing.assert_allclose(x[:, 10:].detach().numpy(), cemb.detach().numpy()[None] * X_cont[:, :, None])
    np.testing.assert_allclose(x[:, :10].detach().numpy(), embed.detach().numpy()[X_cate])
    Ws = [r.standard_normal((E, E)) * 0.5 for _ in range(6)]
    xt = [torch.from_numpy(w).requires_grad_() for w in Ws]
    y = x
    for k in range(2):
        y = AR.attention_torch(y, xt[3 * k], xt[3 * k + 1], xt[3 * k + 2], 2)
    ynp = x.detach().numpy()
    for k in range(2):
        ynp, _ = AR.attention_numpy(ynp, Ws[3 * k], Ws[3 * k + 1], Ws[3 * k + 2], 2)
    np.testing.assert_allclose(y.detach().numpy(), ynp, rtol=1e-12, atol=1e-14)
    gout = torch.from_numpy(r.standard_normal(y.shape))
    g1 = torch.autograd.grad(y, [embed, cemb] + xt, gout)
    x2 = AR.assemble(embed, torch.from_numpy(X_cate), cemb, torch.from_numpy(X_cont))
    y2 = x2
    for k in range(2):
        y2 = AR.attention_einsum(y2, xt[3 * k], xt[3 * k + 1], xt[3 * k + 2], 2)
    g2 = torch.autograd.grad(y2, [embed, cemb] + xt, gout)
    for a, b in zip(g1, g2):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-13)


def _ABI():
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


def test_autoint_abi_rejects_bad_arguments_without_a_gpu():
    lib = _ABI()
    d = C.c_void_p(16)                                   # never dereferenced: every call below fails its checks

    def fwd(x=d, xc=d, ce=d, q=d, k=d, v=d, r=d, B=4, F=13, E=8, H=2, Cc=3, res=1, sc=0, y=d, o=d, st=d, ws=d,
            nbytes=1 << 30):
        return lib.rec_autoint_fwd_f32(x, xc, ce, q, k, v, r, B, F, E, H, Cc, res, sc, y, o, st, ws, nbytes, None)

    def bwd(x=d, xc=d, ce=d, q=d, k=d, v=d, r=d, y=d, dy=d, st=d, B=4, F=13, E=8, H=2, Cc=3, res=1, sc=0, dx=d, dq=d,
            dk=d, dv=d, dr=d, dce=d, ws=d, nbytes=1 << 30):
        return lib.rec_autoint_bwd_f32(x, xc, ce, q, k, v, r, y, dy, st, B, F, E, H, Cc, res, sc, dx, dq, dk, dv, dr,
                                       dce, ws, nbytes, None)

    # null pointers
    assert fwd(x=None) == -1 and fwd(q=None) == -1 and fwd(xc=None) == -1 and fwd(ce=None) == -1
    assert fwd(y=None) == -1 and fwd(st=None) == -1 and fwd(ws=None) == -1 and fwd(res=2, r=None) == -1
    assert bwd(dy=None) == -1 and bwd(dx=None) == -1 and bwd(dce=None) == -1 and bwd(res=2, dr=None) == -1
    # NULL is fine where it is not read: o, Wres / dWres without a learnable residual, continuous inputs at C = 0
    assert fwd(B=0, o=None, r=None) == 0 and fwd(B=0, xc=None, ce=None, Cc=0) == 0 and bwd(B=0, dce=None, Cc=0) == 0
    # negative sizes, bad flags
    assert fwd(B=-1) == -1 and fwd(F=-1) == -1 and fwd(E=-2) == -1 and fwd(H=-1) == -1 and fwd(Cc=-1) == -1
    assert fwd(res=3) == -1 and fwd(res=-1) == -1 and fwd(sc=2) == -1 and bwd(B=-5) == -1 and bwd(sc=-1) == -1
    # unsupported shapes: E % H, H > E, F or E out of range, every field continuous
    assert fwd(H=3) == -2 and fwd(E=4, H=8) == -2 and fwd(F=65) == -2 and fwd(E=65, H=5) == -2 and fwd(E=0) == -2
    assert fwd(F=3, Cc=3) == -2 and fwd(F=0, Cc=0) == -2 and bwd(H=3) == -2 and bwd(F=65) == -2
    # a workspace below rec_autoint_workspace_bytes
    assert fwd(nbytes=16) == -3 and bwd(nbytes=16) == -3
    assert lib.rec_autoint_workspace_bytes(4, 13, 8, 3, 3, 1) == 0
    assert lib.rec_autoint_workspace_bytes(-1, 13, 8, 2, 3, 1) == 0
    assert lib.rec_autoint_workspace_bytes(4, 13, 8, 2, 3, 5) == 0


@pytest.mark.parametrize("B,Fc,E", [(16384, 10, 8), (8192, 26, 16)])
@pytest.mark.parametrize("res", [0, 1, 2])
def test_autoint_workspace_is_positive_for_the_bench_configs(B, Fc, E, res):
    """AI (10 cat + 3 cont, E = 8, B = 16384) and AI26 (26 cat + 3 cont, E = 16, B = 8192), H = 2."""
    lib = _ABI()
    n = lib.rec_autoint_workspace_bytes(B, Fc + 3, E, 2, 3, res)
    assert n > 0
    assert n < 64 << 20
    assert lib.rec_autoint_workspace_bytes(1, 64, 64, 1, 63, 2) > 0


def test_model_manager_builds_autoint_with_the_reference_width():
    """3.DCN/ModelManager.py:94-95 calls AutoIntLayer() with no arguments: E = 8 whatever the manager's
    embedding_dims; the manager's feature lists and vocabulary are used; model_params may set the rest."""
    from explicit_tf2_recommendation_amd import data, layers as CL
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    mm = ModelManager(feature_names=CAT, data_info=data.data_info(5000, len(CAT)), embedding_dims=16, layer="AutoInt",
                      continuous_features=CONT, device="cpu")
    lay = mm.layer
    assert isinstance(lay, CL.AutoIntLayer)
    assert lay.embedding_dims == 8 and tuple(lay.embedding_layer.embeddings.shape) == (mm.feature_dims, 8)
    assert lay.categorical_features == CAT and lay.continuous_features == CONT
    assert tuple(lay.continuous_embedding.embeddings.shape) == (3, 8)
    assert len(lay.attention_layers) == 2 and lay.attention_layers[0].num_heads == 2
    mm2 = ModelManager(feature_names=CAT, data_info=data.data_info(5000, len(CAT)), embedding_dims=16,
                       layer="AutoInt", continuous_features=CONT, device="cpu",
                       model_params={"embedding_dims": 16, "units": [32, 8], "attention_layer_num": 3,
                                     "num_heads": 4, "activation": "relu"})
    lay2 = mm2.layer
    assert lay2.embedding_dims == 16 and len(lay2.attention_layers) == 3 and lay2.attention_layers[2].num_heads == 4
    assert tuple(lay2.dnn_layer.kernel_0.shape) == (13 * 16, 32)
