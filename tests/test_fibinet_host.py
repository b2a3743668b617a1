"""CPU checks of the FiBiNet layer: the reference's keywords and parameter names, the pair order and dnn_in layout, the
two fp64 restatements (tests/fibinet_ref.py) agreeing on values and gradients, TF2 glorot_normal, and the C-ABI status
codes of the FiBiNet entry points without a GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import fibinet_ref as FR

TYPES = ["all", "each", "interaction"]


def test_signatures_keep_the_reference_keywords():
    """3.DCN/CustomLayers.py:902-905, :960 and :985."""
    from explicit_tf2_recommendation_amd import layers as CL
    params = list(inspect.signature(CL.FiBiNetLayer.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["categorical_features", "continuous_features", "feature_dims",
                                        "embedding_dims", "units", "activation", "bilinear_type", "reduction_ratio"]
    d = {p.name: p.default for p in params}
    assert d["categorical_features"] == ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3",
                                         "itag4"]
    assert d["continuous_features"] == ["itag4_origin", "itag4_square", "itag4_cube"]
    assert (d["feature_dims"], d["embedding_dims"], d["units"], d["activation"], d["bilinear_type"],
            d["reduction_ratio"]) == (160000, 16, [128, 16], "relu", "interaction", 3)
    assert inspect.signature(CL.SENetLayer.__init__).parameters["reduction_ratio"].default == 3
    assert inspect.signature(CL.BilinearInteractionLayer.__init__).parameters["bilinear_type"].default == "interaction"


@pytest.mark.parametrize("bilinear_type", TYPES)
def test_parameter_names_and_shapes(bilinear_type):
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.FiBiNetLayer(feature_dims=100, bilinear_type=bilinear_type)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    F, E, P = 10, 16, 45
    want = {"embedding_layer.embeddings": (100, E),
            "dnn_layer.kernel_0": (2 * P * E + 3, 128), "dnn_layer.bias_0": (128,),
            "dnn_layer.kernel_1": (128, 16), "dnn_layer.bias_1": (16,),
            "output_layer.kernel": (16, 1), "output_layer.bias": (1,),
            "SENet.excitation.kernel_0": (F, 3), "SENet.excitation.kernel_1": (3, F)}
    if bilinear_type == "all":
        names = ["bilinear_weight"]
    elif bilinear_type == "each":
        names = ["bilinear_weight%d" % i for i in range(F - 1)]
    else:
        names = ["bilinear_weight%d_%d" % (i, j) for i, j in FR.pairs(F)]
    want.update({"Bilinear." + n: (E, E) for n in names})
    assert shapes == want
    assert set(lay.state_dict()) == set(want)
    # the bilinear weights are views of one packed array, in parameter order
    ws = lay.Bilinear.weights()
    base = ws[0].data_ptr()
    assert [w.data_ptr() - base for w in ws] == [4 * E * E * k for k in range(len(ws))]
    W = lay.Bilinear.packed_weight(ws)
    assert W.shape == (len(ws), E, E) and W.data_ptr() == base
    assert torch.equal(W[-1], ws[-1])


def test_packing_survives_outside_replacement():
    from explicit_tf2_recommendation_amd import layers as CL
    b = CL.BilinearInteractionLayer("each", input_shape=(4, 3))
    b.bilinear_weight1 = torch.nn.Parameter(torch.ones(3, 3))
    W = b.packed_weight(b.weights())
    assert W.shape == (3, 3, 3) and torch.equal(W[1], torch.ones(3, 3))
    b._post_apply()
    assert b._is_packed() and torch.equal(b.packed_weight(b.weights())[1], torch.ones(3, 3))


def test_unknown_bilinear_type_raises():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(NotImplementedError):
        CL.FiBiNetLayer(feature_dims=100, bilinear_type="outer")


def test_senet_mid_units():
    from explicit_tf2_recommendation_amd import layers as CL
    assert CL.SENetLayer(3, input_dim=10).mid_unit_num == 3
    assert CL.SENetLayer(3, input_dim=2).mid_unit_num == 1
    assert CL.SENetLayer(1, input_dim=26).mid_unit_num == 26


def test_glorot_normal_is_tf2s_truncated_normal():
    from explicit_tf2_recommendation_amd import layers as CL
    CL.set_init_seed(5)
    w = CL.glorot_normal((400, 16, 16)).double()
    std = np.sqrt(2.0 / 32) / 0.87962566103423978
    assert float(w.abs().max()) <= 2 * std
    assert abs(float(w.std()) - np.sqrt(2.0 / 32)) < 0.02 * np.sqrt(2.0 / 32)
    assert abs(float(w.mean())) < 0.01 * std
    CL.set_init_seed(5)
    assert torch.equal(CL.glorot_normal((400, 16, 16)).double(), w)
    assert CL._initializer("glorot_normal") is CL.glorot_normal


def test_pair_order_and_column_layout():
    """Raw pairs, then SENet pairs, then the continuous columns; (s, pair, e) at column (s P + pair) E + e."""
    B, F, E = 2, 4, 3
    r = np.random.default_rng(0)
    x = r.uniform(0.5, 1.5, (B, F, E))
    xc = np.array([[7.0, 8.0], [9.0, 10.0]])
    S0 = np.full((F, 1), 0.5)
    S1 = np.arange(1, F + 1, dtype=np.float64).reshape(1, F) / 4
    Ws = [np.eye(E)] * 6
    got = FR.fibinet_numpy(x, xc, S0, S1, Ws, "interaction")
    A, _ = FR.senet_numpy(x, S0, S1)
    assert got.shape == (B, 2 * 6 * E + 2)
    for k, (i, j) in enumerate([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]):
        for e in range(E):
            np.testing.assert_allclose(got[:, k * E + e], x[:, i, e] * x[:, j, e])
            np.testing.assert_allclose(got[:, (6 + k) * E + e], A[:, i] * A[:, j] * x[:, i, e] * x[:, j, e])
    np.testing.assert_array_equal(got[:, -2:], xc)


def _rand_case(B, F, E, C, mid, bilinear_type, seed):
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, F, E))
    xc = r.standard_normal((B, C))
    S0 = r.uniform(0.1, 1.0, (F, mid)) * r.choice([-1, 1], (F, mid))
    S1 = r.standard_normal((mid, F))
    nW = {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[bilinear_type]
    Ws = [r.standard_normal((E, E)) for _ in range(nW)]
    return x, xc, S0, S1, Ws


def _einsum_autograd(x, xc, S0, S1, Ws, bilinear_type, gout):
    """Gradients of the A_i A_j p_ij reading (the kernel's algebra) through torch autograd."""
    xt = torch.from_numpy(x).requires_grad_()
    s0, s1 = torch.from_numpy(S0).requires_grad_(), torch.from_numpy(S1).requires_grad_()
    wt = [torch.from_numpy(w).requires_grad_() for w in Ws]
    A = torch.relu(torch.relu(xt.mean(-1) @ s0) @ s1)
    raw, sen = [], []
    for k, (i, j) in enumerate(FR.pairs(x.shape[1])):
        p = torch.einsum("bd,de,be->be", xt[:, i], wt[FR.weight_of(bilinear_type, k, i)], xt[:, j])
        raw.append(p)
        sen.append((A[:, i] * A[:, j]).unsqueeze(1) * p)
    out = torch.cat(raw + sen + [torch.from_numpy(xc)], dim=1)
    out.backward(torch.from_numpy(gout))
    return out.detach().numpy(), xt.grad.numpy(), s0.grad.numpy(), s1.grad.numpy(), [w.grad.numpy() for w in wt]


@pytest.mark.parametrize("bilinear_type", TYPES)
@pytest.mark.parametrize("B,F,E,C,mid", [(5, 4, 3, 2, 1), (3, 10, 16, 3, 3), (2, 2, 5, 0, 1), (4, 7, 4, 1, 7)])
def test_restatements_agree_on_values_and_gradients(bilinear_type, B, F, E, C, mid):
    x, xc, S0, S1, Ws = _rand_case(B, F, E, C, mid, bilinear_type, seed=B * 31 + F)
    want = FR.fibinet_numpy(x, xc, S0, S1, Ws, bilinear_type)
    xt = torch.from_numpy(x).requires_grad_()
    s0, s1 = torch.from_numpy(S0).requires_grad_(), torch.from_numpy(S1).requires_grad_()
    wt = [torch.from_numpy(w).requires_grad_() for w in Ws]
    got = FR.fibinet_torch(xt, torch.from_numpy(xc), s0, s1, wt, bilinear_type)
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-12, atol=1e-12)
    gout = np.random.default_rng(1).standard_normal(got.shape)
    got.backward(torch.from_numpy(gout))
    out2, dx2, ds02, ds12, dw2 = _einsum_autograd(x, xc, S0, S1, Ws, bilinear_type, gout)
    np.testing.assert_allclose(out2, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xt.grad.numpy(), dx2, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(s0.grad.numpy(), ds02, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(s1.grad.numpy(), ds12, rtol=1e-10, atol=1e-10)
    for a, b in zip(wt, dw2):
        np.testing.assert_allclose(a.grad.numpy(), b, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("bilinear_type", TYPES)
def test_restatements_on_the_reference_main_input(bilinear_type):
    """np.arange(72).reshape(3,6,4), the input of 3.DCN/CustomLayers.py's __main__, with asymmetric weights."""
    x = np.arange(72, dtype=np.float64).reshape(3, 6, 4)
    F, E = 6, 4
    S0 = np.cos(np.arange(F * 2, dtype=np.float64)).reshape(F, 2) + 0.3
    S1 = np.sin(np.arange(2 * F, dtype=np.float64)).reshape(2, F) + 0.2
    nW = {"all": 1, "each": F - 1, "interaction": 15}[bilinear_type]
    Ws = [np.arange(E * E, dtype=np.float64).reshape(E, E) / (7.0 + k) - 1.0 for k in range(nW)]
    xc = np.zeros((3, 0))
    want = FR.fibinet_numpy(x, xc, S0, S1, Ws, bilinear_type)
    xt = torch.from_numpy(x).requires_grad_()
    got = FR.fibinet_torch(xt, torch.from_numpy(xc), torch.from_numpy(S0), torch.from_numpy(S1),
                           [torch.from_numpy(w) for w in Ws], bilinear_type)
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-12)
    # by hand: example 1, pair (1, 3) = pair index 5 + 1 = 6, e = 2: (v_1 W) [2] * v_3[2]
    k = 6
    w = Ws[FR.weight_of(bilinear_type, k, 1)]
    hand = sum(x[1, 1, d] * w[d, 2] for d in range(E)) * x[1, 3, 2]
    assert abs(want[1, k * E + 2] - hand) <= 1e-12 * abs(hand)
    # the transposed weight gives other numbers
    swapped = FR.fibinet_numpy(x, xc, S0, S1, [wi.T for wi in Ws], bilinear_type)
    assert np.abs(swapped - want).max() > 1.0


def _ABI():
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


def test_fibinet_abi_rejects_bad_arguments_without_a_gpu():
    lib = _ABI()
    d = C.c_void_p(16)                                   # never dereferenced: every call below fails its checks

    def fwd(x=d, xc=d, s0=d, s1=d, w=d, B=4, F=10, E=16, Cc=3, mid=3, t=2, out=d, a=d, h=d):
        return lib.rec_fibinet_fwd_f32(x, xc, s0, s1, w, B, F, E, Cc, mid, t, out, a, h, None)

    def bwd(x=d, g=d, a=d, h=d, s0=d, s1=d, w=d, B=4, F=10, E=16, Cc=3, mid=3, t=2, dx=d, dw=d, ds0=d, ds1=d, ws=d,
            nbytes=1 << 30):
        return lib.rec_fibinet_bwd_f32(x, g, a, h, s0, s1, w, B, F, E, Cc, mid, t, dx, dw, ds0, ds1, ws, nbytes, None)

    # null pointers
    assert fwd(x=None) == -1 and fwd(w=None) == -1 and fwd(xc=None) == -1 and fwd(h=None) == -1
    assert bwd(g=None) == -1 and bwd(ws=None) == -1 and bwd(ds1=None) == -1
    # negative sizes, bad type
    assert fwd(B=-1) == -1 and fwd(F=-1) == -1 and fwd(E=-2) == -1 and fwd(Cc=-1) == -1 and fwd(mid=-1) == -1
    assert fwd(t=3) == -1 and fwd(t=-1) == -1 and bwd(B=-5) == -1
    # unsupported shapes
    assert fwd(F=1, mid=1) == -2 and fwd(F=33) == -2 and fwd(E=0) == -2 and fwd(E=65) == -2 and fwd(Cc=65) == -2
    assert fwd(mid=0) == -2 and fwd(mid=11) == -2 and bwd(F=33) == -2 and bwd(E=65) == -2
    # B = 0 is a no-op; C = 0 needs no x_cont
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and fwd(B=0, xc=None, Cc=0) == 0
    # a workspace below rec_fibinet_workspace_bytes
    assert bwd(nbytes=16) == -3
    assert lib.rec_fibinet_workspace_bytes(4, 33, 16, 3, 2) == 0
    assert lib.rec_fibinet_workspace_bytes(4, 10, 16, 3, 5) == 0
    assert lib.rec_fibinet_workspace_bytes(-1, 10, 16, 3, 2) == 0


@pytest.mark.parametrize("F,B", [(10, 16384), (26, 8192)])
@pytest.mark.parametrize("t", [0, 1, 2])
def test_fibinet_workspace_is_positive_for_the_bench_configs(F, B, t):
    lib = _ABI()
    n = lib.rec_fibinet_workspace_bytes(B, F, 16, max(1, F // 3), t)
    assert n > 0
    assert n < 64 << 20                                  # bounded: far below g = B * 2PE * 4 bytes at FB26 (341 MB)
    assert lib.rec_fibinet_workspace_bytes(1, 32, 64, 32, 2) > 0


def test_layer_reports_unsupported_shapes():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(NotImplementedError, match="fields"):
        CL.FiBiNetLayer(categorical_features=["c%d" % i for i in range(33)], feature_dims=100)
    with pytest.raises(NotImplementedError, match="embedding_dims"):
        CL.FiBiNetLayer(feature_dims=100, embedding_dims=65)
    with pytest.raises(NotImplementedError):
        CL.FiBiNetLayer(categorical_features=["a"], feature_dims=100)
    with pytest.raises(NotImplementedError):
        CL.FiBiNetLayer(feature_dims=100, continuous_features=["x%d" % i for i in range(65)])


def test_model_manager_knows_fibinet():
    from explicit_tf2_recommendation_amd import model_manager
    src = inspect.getsource(model_manager.ModelManager.make_layer_choice)
    assert '"FiBiNet"' in src and "FiBiNetLayer" in src
