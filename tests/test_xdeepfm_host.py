"""CPU checks of the xDeepFM layer: the reference's constructor keywords, the C-ABI status codes of the CIN entry points
without a GPU, and the two fp64 restatements of CINLayer (tests/xdeepfm_ref.py) agreeing on values and gradients."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import xdeepfm_ref as XR


def _H(*h):
    return (C.c_int * len(h))(*h)


def test_signatures_keep_the_reference_keywords():
    """3.DCN/CustomLayers.py:323-327 and :384."""
    from explicit_tf2_recommendation_amd import layers as CL
    want = {CL.XDeepFMRankingLayer: ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                     "units", "activation", "cin_size"],
            CL.CINLayer: ["cin_size"]}
    for cls, kws in want.items():
        params = list(inspect.signature(cls.__init__).parameters)[1:]
        assert params[:len(kws)] == kws, (cls.__name__, params)
    sig = inspect.signature(CL.XDeepFMRankingLayer.__init__).parameters
    assert sig["cin_size"].default == [16, 32, 64] and sig["units"].default == [64, 8]
    assert sig["embedding_dims"].default == 16 and sig["activation"].default == "relu"


def test_cin_abi_rejects_bad_arguments_without_a_gpu():
    from explicit_tf2_recommendation_amd._lib import lib
    dummy = C.c_void_p(16)                                  # never dereferenced: every call below fails its checks
    W = (C.c_void_p * 8)(*([16] * 8))
    # null pointers
    assert lib.rec_cin_fwd_f32(None, 4, 10, 16, 3, _H(16, 32, 64), W, dummy, dummy, None) == -1
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 16, 3, _H(16, 32, 64), None, dummy, dummy, None) == -1
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 16, 3, None, W, dummy, dummy, None) == -1
    assert lib.rec_cin_bwd_f32(dummy, dummy, dummy, 4, 10, 16, 3, _H(16, 32, 64), W, dummy, W, None, 1 << 30,
                               None) == -1
    assert lib.rec_cin_bwd_f32(dummy, dummy, None, 4, 10, 16, 3, _H(16, 32, 64), W, dummy, W, dummy, 1 << 30,
                               None) == -1
    # invalid sizes
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 16, 2, _H(16, 0), W, dummy, dummy, None) == -1      # H_k = 0
    assert lib.rec_cin_fwd_f32(dummy, 0, 10, 16, 1, _H(16), W, dummy, dummy, None) == -1         # B = 0
    assert lib.rec_cin_fwd_f32(dummy, 4, 0, 16, 1, _H(16), W, dummy, dummy, None) == -1          # F = 0
    # unsupported shapes
    assert lib.rec_cin_fwd_f32(dummy, 4, 65, 16, 1, _H(16), W, dummy, dummy, None) == -2         # F = 65
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 65, 1, _H(16), W, dummy, dummy, None) == -2         # E = 65
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 16, 9, _H(*[8] * 9), W, dummy, dummy, None) == -2   # L = 9
    assert lib.rec_cin_fwd_f32(dummy, 4, 10, 16, 1, _H(257), W, dummy, dummy, None) == -2        # H_k = 257
    assert lib.rec_cin_bwd_f32(dummy, dummy, dummy, 4, 65, 16, 1, _H(16), W, dummy, W, dummy, 1 << 30, None) == -2
    assert lib.rec_cin_bwd_f32(dummy, dummy, dummy, 4, 10, 16, 9, _H(*[8] * 9), W, dummy, W, dummy, 1 << 30,
                               None) == -2
    # a workspace below rec_cin_workspace_bytes
    assert lib.rec_cin_bwd_f32(dummy, dummy, dummy, 4, 10, 16, 3, _H(16, 32, 64), W, dummy, W, dummy, 16, None) == -3
    assert lib.rec_cin_workspace_bytes(4, 65, 16, 1, _H(16)) == 0
    assert lib.rec_cin_workspace_bytes(4, 10, 16, 1, _H(0)) == 0


@pytest.mark.parametrize("F", [10, 26])
def test_cin_workspace_is_positive_for_the_bench_configs(F):
    from explicit_tf2_recommendation_amd._lib import lib
    n = lib.rec_cin_workspace_bytes(16384, F, 16, 3, _H(16, 32, 64))
    wsum = F * (F * 16 + 16 * 32 + 32 * 64) * 4               # bytes of one set of dW
    assert n > 0 and n % wsum == 0
    assert lib.rec_cin_workspace_bytes(1, 64, 64, 8, _H(*[256] * 8)) > 0    # the largest supported shape


def test_cin_layer_reports_unsupported_shapes():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(NotImplementedError, match="cin_size"):
        CL.XDeepFMRankingLayer(categorical_features=["c%d" % i for i in range(65)], feature_dims=100)
    with pytest.raises(NotImplementedError, match="cin_size"):
        CL.XDeepFMRankingLayer(feature_dims=100, cin_size=[300])
    with pytest.raises(NotImplementedError):
        CL.XDeepFMRankingLayer(feature_dims=100, cin_size=[8] * 9)


def test_cin_layer_parameter_names_and_shapes():
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.XDeepFMRankingLayer(feature_dims=100, embedding_dims=16, cin_size=[16, 32, 64])
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    assert shapes == {
        "w.embeddings": (100, 1), "embedding_layer.embeddings": (100, 16),
        "dense_layer.hidden_layer.0.kernel": (3 + 160, 64), "dense_layer.hidden_layer.0.bias": (64,),
        "dense_layer.hidden_layer.1.kernel": (64, 8), "dense_layer.hidden_layer.1.bias": (8,),
        "cin_layer.w0": (1, 100, 16), "cin_layer.w1": (1, 160, 32), "cin_layer.w2": (1, 320, 64),
        "output_layer.kernel": (1 + 8 + 112, 1), "output_layer.bias": (1,)}
    assert set(lay.state_dict()) == set(shapes)
    # Keras glorot-uniform on (1, F*H_k, H_{k+1}): fan_in F*H_k, fan_out H_{k+1}
    for k, (a, b) in enumerate([(100, 16), (160, 32), (320, 64)]):
        w = getattr(lay.cin_layer, "w%d" % k)
        assert float(w.detach().abs().max()) <= np.sqrt(6.0 / (a + b))


def _two_readings(x0, Ws):
    xt = torch.from_numpy(x0).double().requires_grad_()
    wt = [torch.from_numpy(w).double().requires_grad_() for w in Ws]
    got = XR.cin_torch_lines(xt, wt)
    want, _ = XR.cin_numpy(x0, Ws)
    return xt, wt, got, want


def test_cin_ordering_on_the_reference_docstring_input():
    """CINLayer([2,4]) on np.arange(24).reshape(2,3,4) (3.DCN/CustomLayers.py:378-382), with asymmetric weights."""
    x0 = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    Ws = [np.arange(1 * 9 * 2, dtype=np.float64).reshape(1, 9, 2) / 7.0 - 1.0,
          np.cos(np.arange(1 * 6 * 4, dtype=np.float64)).reshape(1, 6, 4)]
    xt, wt, got, want = _two_readings(x0, Ws)
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-12, atol=1e-9)
    # by hand, example 0, layer 1, unit 1: sum_e sum_{m,n} W0[m*3 + n, 1] x0[m,e] x0[n,e]
    x = x0[0]
    hand = sum(Ws[0][0, m * 3 + n, 1] * x[m, e] * x[n, e] for e in range(4) for m in range(3) for n in range(3))
    assert abs(want[0, 1] - hand) <= 1e-9 * abs(hand)
    # the transposed reading (n*F + m) of layer 1's rows gives other numbers (layer 0 is symmetric in m, n: X^0 = X0)
    swapped = [Ws[0], Ws[1].reshape(1, 3, 2, 4).transpose(0, 2, 1, 3).reshape(1, 6, 4)]
    assert np.abs(XR.cin_numpy(x0, swapped)[0] - want).max() > 1e-3


@pytest.mark.parametrize("B,F,E,cin", [(3, 5, 4, [3, 6]), (2, 1, 1, [1]), (4, 7, 3, [5, 2, 4])])
def test_cin_restatements_agree_on_values_and_gradients(B, F, E, cin):
    r = np.random.default_rng(B * 100 + F)
    x0 = r.standard_normal((B, F, E))
    hs = [F] + cin
    Ws = [r.standard_normal((1, F * hs[k], hs[k + 1])) for k in range(len(cin))]
    xt, wt, got, want = _two_readings(x0, Ws)
    np.testing.assert_allclose(got.detach().numpy(), want, rtol=1e-10, atol=1e-10)
    gout = r.standard_normal(got.shape)
    got.backward(torch.from_numpy(gout))
    # autograd of the einsum reading
    x2 = torch.from_numpy(x0).requires_grad_()
    w2 = [torch.from_numpy(w).requires_grad_() for w in Ws]
    xk, outs = x2, []
    for W in w2:
        xk = torch.einsum("bme,bne,mnh->bhe", x2, xk, W.reshape(F, xk.shape[1], W.shape[-1]))
        outs.append(xk)
    torch.cat(outs, dim=1).sum(-1).backward(torch.from_numpy(gout))
    np.testing.assert_allclose(xt.grad.numpy(), x2.grad.numpy(), rtol=1e-10, atol=1e-10)
    for a, b in zip(wt, w2):
        np.testing.assert_allclose(a.grad.numpy(), b.grad.numpy(), rtol=1e-10, atol=1e-10)


def test_model_manager_knows_xdeepfm():
    from explicit_tf2_recommendation_amd import model_manager
    src = inspect.getsource(model_manager.ModelManager.make_layer_choice)
    assert '"xDeepFM"' in src and "XDeepFMRankingLayer" in src
