"""CPU checks of the FGCNN layer: the heights of the VALID poolings and the Dense units with their original-field-count
quirk, the dropped trailing rows, the tie rule of the pooling in numpy and in torch, the Flatten and concat order, the two
restatements against each other (tests/fgcnn_ref.py), the C-ABI status codes of the FGCNN entry points without a GPU, the
layer's parameter names and shapes, and ModelManager(layer='FGCNN')."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import ccpm_ref as CR
from tests import fgcnn_ref as FR

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


@pytest.mark.parametrize("F,E,maps,pws,H,U,N", [
    (10, 16, [3, 3], [2, 2], [5, 2], [240, 240], [15, 15]),        # the defaults
    (26, 16, [3, 3], [2, 2], [13, 6], [624, 624], [39, 39]),
    (11, 16, [3, 3], [2, 2], [5, 2], [264, 264], [16, 16]),        # F odd: the last row is dropped, U still counts 11
    (27, 16, [3, 2], [2, 3], [13, 4], [648, 288], [40, 18]),       # U_2 = 2 * 27 * 16 // 3, not from H_1 = 13
    (9, 4, [1], [3], [3], [12], [3]),
    (12, 12, [2], [5], [2], [57], [4]),                            # 57 % 12 != 0: the layer refuses it, see below
])
def test_heights_and_dense_units_come_from_the_original_field_count(F, E, maps, pws, H, U, N):
    from explicit_tf2_recommendation_amd import ops
    assert ops.fgcnn_heights(F, pws) == H and FR.heights(F, pws) == H
    assert ops.fgcnn_dense_units(F, E, maps, pws) == U and FR.dense_units(F, E, maps, pws) == U
    assert [u // E for u in U] == N


def test_dropped_trailing_rows_get_zero_gradient():
    """F = 5, pw = 2: H_1 = 2, field 4 is outside every window.  kw = 1, so nothing else reaches it either."""
    r = np.random.default_rng(0)
    rows = r.standard_normal((3, 5, 4))
    params = [(np.full((1, 1, 1, 2), 0.7), np.zeros(2))]
    ref = FR.fgcnn_numpy(rows, params, [2], [np.ones((3, 2 * 4 * 2))])
    assert ref["pooled"][0].shape == (3, 2 * 4 * 2)
    assert np.count_nonzero(ref["drows"][:, 4]) == 0 and np.count_nonzero(ref["drows"][:, :4]) == 3 * 2 * 4
    _, drows, _ = FR.fgcnn_torch_grads(rows, params, [2], [np.ones((3, 16))], None, torch.float64)
    assert np.count_nonzero(drows[:, 4]) == 0
    np.testing.assert_allclose(drows, ref["drows"], rtol=1e-13)
    # pw = 3 of 7 rows: two windows, row 6 dropped
    rows = r.standard_normal((2, 7, 3))
    ref = FR.fgcnn_numpy(rows, params, [3], [np.ones((2, 2 * 3 * 2))])
    assert np.count_nonzero(ref["drows"][:, 6]) == 0 and np.count_nonzero(ref["drows"]) == 2 * 2 * 3


def test_ties_go_to_the_lower_field_in_numpy_and_in_torch():
    y = np.array([0.1, 0.9, 0.9, 0.3, 0.5, 0.5]).reshape(1, 6, 1, 1)
    v, idx, gap = FR.pool_numpy(y, 3)
    assert v.reshape(-1).tolist() == [0.9, 0.5] and idx.reshape(-1).tolist() == [1, 1]
    assert gap[0] == 0.0
    assert FR.pool_numpy(y, 3, distinct_gap=True)[2][0] == pytest.approx(0.2)      # 0.5 - 0.3; 0.9 - 0.1 is wider
    # torch.nn.functional.max_pool2d on the CPU routes the gradient of equal values the same way
    t = torch.from_numpy(y).requires_grad_()
    FR.pool_torch(t, 3).sum().backward()
    assert t.grad.reshape(-1).tolist() == [0.0, 1.0, 0.0, 0.0, 1.0, 0.0]
    t = torch.full((1, 4, 1, 1), 0.25, dtype=torch.float32, requires_grad=True)
    FR.pool_torch(t, 2).sum().backward()
    assert t.grad.reshape(-1).tolist() == [1.0, 0.0, 1.0, 0.0]
    # and through the whole stack: identical rows, kw = 1, so every position of a window ties
    rows = np.full((1, 4, 2), 0.3)
    params = [(np.full((1, 1, 1, 1), 0.7), np.zeros(1))]
    ref = FR.fgcnn_numpy(rows, params, [2], [np.ones((1, 2 * 2))])
    assert np.count_nonzero(ref["drows"][0, [1, 3]]) == 0 and np.count_nonzero(ref["drows"][0, [0, 2]]) == 4
    _, drows, _ = FR.fgcnn_torch_grads(rows, params, [2], [np.ones((1, 4))], None, torch.float64)
    np.testing.assert_allclose(drows, ref["drows"], rtol=1e-14)


def test_flatten_order_is_h_then_e_then_c_and_the_concat_keeps_layer_order():
    """A table whose entries encode (h, e) and grow with h, kernels whose channel c scales by (c + 1), kw = 1, pw = 2:
    p[(r E + e) C + c] is channel c of embedding dim e of field 2 r + 1."""
    F, E, Cn = 4, 3, 2
    rows = np.zeros((1, F, E))
    for h in range(F):
        for e in range(E):
            rows[0, h, e] = 0.01 * (h + 1) + 0.001 * e
    K = np.zeros((1, 1, 1, Cn))
    K[0, 0, 0] = [1.0, 2.0]
    p = FR.fgcnn_numpy(rows, [(K, np.zeros(Cn))], [2])["pooled"][0][0]
    assert p.shape == (2 * E * Cn,)
    for r in range(2):
        for e in range(E):
            for c in range(Cn):
                assert p[(r * E + e) * Cn + c] == pytest.approx(np.tanh((c + 1) * rows[0, 2 * r + 1, e]), rel=1e-14)
    t = FR.fgcnn_torch(torch.from_numpy(rows), [torch.from_numpy(K), torch.zeros(Cn, dtype=torch.float64)], [2])
    np.testing.assert_allclose(t[0].numpy()[0], p, rtol=1e-14)
    # the base layer: Dense j is the identity on its first N_j E inputs, so block j of the output shows p_j in order
    params = [torch.from_numpy(K), torch.zeros(Cn, dtype=torch.float64),
              torch.from_numpy(np.full((1, 1, Cn, 1), 0.5)), torch.zeros(1, dtype=torch.float64)]
    p1, p2 = FR.fgcnn_torch(torch.from_numpy(rows), params, [2, 2])
    U = FR.dense_units(F, E, [1, 1], [2, 2])
    assert U == [6, 6] and p1.shape[1] == 12 and p2.shape[1] == 3
    dense = [torch.eye(12, 6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64),
             torch.eye(3, 6, dtype=torch.float64), torch.ones(6, dtype=torch.float64)]
    out = FR.fgcnn_base_torch(torch.from_numpy(rows), params, dense, [2, 2])
    assert tuple(out.shape) == (1, 4, E)
    np.testing.assert_allclose(out[0, :2].reshape(-1).numpy(), p1[0, :6].numpy(), rtol=1e-14)
    np.testing.assert_allclose(out[0, 2].numpy(), p2[0].numpy() + 1.0, rtol=1e-14)
    np.testing.assert_allclose(out[0, 3].numpy(), np.ones(3), rtol=1e-14)


@pytest.mark.parametrize("B,F,E,filters,kw,pws", [
    (5, 10, 16, [14, 16], [7, 7], [2, 2]), (3, 26, 16, [14, 16], [7, 7], [2, 2]), (4, 3, 1, [1], [1], [3]),
    (2, 3, 6, [4, 6], [4, 2], [1, 3]), (2, 27, 16, [16, 16], [8, 3], [2, 3]), (3, 16, 16, [4, 6, 5], [4, 3, 2], [2, 2, 2]),
    (2, 20, 40, [3, 2], [5, 6], [3, 2]), (3, 12, 12, [4], [7], [5]), (3, 11, 8, [3, 2], [3, 2], [2, 2])])
def test_restatements_agree_on_values_and_gradients(B, F, E, filters, kw, pws):
    r = np.random.default_rng(B * 100 + F)
    rows = r.standard_normal((B, F, E)) * 0.5
    params = [(np.asarray(K, np.float64), np.asarray(b, np.float64)) for K, b in CR.make_params(filters, kw, F + E)]
    hs = FR.heights(F, pws)
    dps = [r.uniform(-1, 1, (B, h * E * c)) for h, c in zip(hs, filters)]
    dd = r.uniform(-1, 1, (B, F, E))
    ref = FR.fgcnn_numpy(rows, params, pws, dps, dd)
    outs, drows, dpar = FR.fgcnn_torch_grads(rows, params, pws, dps, dd, torch.float64)
    for got, want, h, c in zip(outs, ref["pooled"], hs, filters):
        assert want.shape == (B, h * E * c)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(drows, ref["drows"], rtol=1e-9, atol=1e-12)
    for got, want in zip(dpar, [a for kb in ref["dparams"] for a in kb]):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert np.all(ref["gap"] > 0)
    # without the direct gradient the rows receive exactly that much less
    ref0 = FR.fgcnn_numpy(rows, params, pws, dps)
    np.testing.assert_allclose(ref["drows"] - ref0["drows"], dd, rtol=0, atol=1e-12)


def _ABI():
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


def _ints(v):
    return (C.c_int * len(v))(*v)


def test_fgcnn_abi_rejects_bad_arguments_without_a_gpu():
    lib = _ABI()
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    FI, KW, PW = [14, 16], [7, 7], [2, 2]

    def ptrs(n, null_at=None):
        return (C.c_void_p * n)(*[None if i == null_at else 16 for i in range(n)])

    def fwd(tab=d, V=100, E=16, ld=16, X=d, B=4, F=10, fi=FI, kw=KW, pw=PW, par=d, rows=d, pooled=0, oob=d, L=None):
        L = len(fi) if L is None else L
        pooled = ptrs(max(L, 1)) if pooled == 0 else pooled
        return lib.rec_emb_fgcnn_fwd_f32(tab, V, E, ld, X, B, F, L, _ints(fi), _ints(kw), _ints(pw), par, rows, pooled,
                                         oob, None)

    def bwd(E=16, B=4, F=10, fi=FI, kw=KW, pw=PW, par=d, rows=d, dp=0, dd=d, vals=d, dpar=d, ws=d, nbytes=1 << 30,
            L=None):
        L = len(fi) if L is None else L
        dp = ptrs(max(L, 1)) if dp == 0 else dp
        return lib.rec_emb_fgcnn_bwd_f32(E, B, F, L, _ints(fi), _ints(kw), _ints(pw), par, rows, dp, dd, vals, dpar, ws,
                                         nbytes, None)

    for k in ("tab", "X", "par", "rows", "pooled"):
        assert fwd(**{k: None}) == -1, k
    assert fwd(pooled=ptrs(2, null_at=1)) == -1
    for k in ("par", "rows", "dp", "vals", "dpar", "ws"):
        assert bwd(**{k: None}) == -1, k
    assert bwd(dp=ptrs(2, null_at=0)) == -1
    assert lib.rec_emb_fgcnn_fwd_f32(d, 100, 16, 16, d, 4, 10, 2, None, _ints(KW), _ints(PW), d, d, ptrs(2), d, None) == -1
    # NULL is fine where it is not read: the flag, the direct gradient, and everything at B = 0
    assert fwd(B=0, tab=None, X=None, par=None, rows=None, pooled=None, oob=None) == 0
    assert bwd(B=0, par=None, rows=None, dp=None, dd=None, vals=None, dpar=None, ws=None) == 0
    # negative sizes, an empty table, a row stride below E
    assert fwd(B=-1) == -1 and fwd(F=-1) == -1 and fwd(E=-2) == -1 and fwd(L=-1) == -1 and fwd(V=0) == -1
    assert fwd(fi=[14, -6]) == -1 and fwd(kw=[-4, 2]) == -1 and fwd(ld=8) == -1 and bwd(B=-5) == -1 and bwd(F=-1) == -1
    # a pooling width below 1, or one that leaves no row
    assert fwd(pw=[0, 2]) == -1 and fwd(pw=[2, -1]) == -1 and bwd(pw=[0, 2]) == -1
    assert fwd(F=3) == -1 and bwd(F=3) == -1 and fwd(pw=[2, 6]) == -1 and fwd(F=1) == -1
    assert lib.rec_fgcnn_workspace_bytes(4, 3, 16, 2, _ints(FI), _ints(KW), _ints(PW)) == 0
    # unsupported shapes
    assert fwd(F=0) == -2 and fwd(F=65) == -2 and fwd(E=65, ld=65) == -2 and fwd(E=0) == -2
    assert fwd(fi=[17, 6]) == -2 and fwd(kw=[9, 2]) == -2 and fwd(fi=[0, 6]) == -2 and fwd(kw=[7, 0]) == -2
    assert fwd(F=64, pw=[9, 2]) == -2 and fwd(V=1 << 31) == -2 and fwd(L=0) == -2
    assert fwd(F=64, fi=[4] * 4, kw=[2] * 4, pw=[2] * 4) == -2
    assert bwd(fi=[17, 6]) == -2 and bwd(F=65) == -2 and bwd(L=0) == -2 and bwd(F=64, pw=[2, 9]) == -2
    # a workspace below rec_fgcnn_workspace_bytes
    assert bwd(nbytes=16) == -3
    assert lib.rec_fgcnn_workspace_bytes(-1, 10, 16, 2, _ints(FI), _ints(KW), _ints(PW)) == 0
    assert lib.rec_fgcnn_workspace_bytes(4, 10, 16, 2, _ints([14, 17]), _ints(KW), _ints(PW)) == 0
    assert lib.rec_fgcnn_workspace_bytes(4, 10, 16, 2, None, None, None) == 0


@pytest.mark.parametrize("B,F", [(16384, 10), (8192, 26)])
def test_fgcnn_workspace_is_positive_for_the_bench_configs(B, F):
    """FG (10 fields, B = 16384) and FG26 (26 fields, B = 8192), E = 16, default filters."""
    lib = _ABI()
    n = lib.rec_fgcnn_workspace_bytes(B, F, 16, 2, _ints([14, 16]), _ints([7, 7]), _ints([2, 2]))
    assert 0 < n < 64 << 20
    # the corners of the tested envelope, and of the limits: the widest state of one column still fits
    assert lib.rec_fgcnn_workspace_bytes(17, 64, 64, 2, _ints([2, 3]), _ints([4, 2]), _ints([2, 2])) > 0
    assert lib.rec_fgcnn_workspace_bytes(1000, 27, 16, 2, _ints([16, 16]), _ints([8, 3]), _ints([2, 3])) > 0
    assert lib.rec_fgcnn_workspace_bytes(2, 16, 16, 3, _ints([4, 6, 5]), _ints([4, 3, 2]), _ints([2, 2, 2])) > 0
    assert lib.rec_fgcnn_workspace_bytes(1, 3, 1, 1, _ints([1]), _ints([1]), _ints([3])) > 0
    assert lib.rec_fgcnn_workspace_bytes(4, 64, 64, 3, _ints([16] * 3), _ints([8] * 3), _ints([1] * 3)) > 0


def test_signatures_keep_the_reference_keywords():
    """3.DCN/CustomLayers.py:729 and :776-779."""
    from explicit_tf2_recommendation_amd import layers as CL
    params = list(inspect.signature(CL.FGCNNLayer.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                        "units", "activation", "is_batch_norm", "filters", "kernel_width", "dnn_maps",
                                        "pooling_width"]
    d = {p.name: p.default for p in params}
    assert d["categorical_features"] == CAT and d["continuous_features"] == CONT
    assert (d["feature_dims"], d["embedding_dims"], d["units"], d["activation"], d["is_batch_norm"], d["filters"],
            d["kernel_width"], d["dnn_maps"], d["pooling_width"]) == (150000, 16, [64, 8], "relu", True, [14, 16], [7, 7],
                                                                      [3, 3], [2, 2])
    base = list(inspect.signature(CL.FGCNNBaseLayer.__init__).parameters.values())[1:5]
    assert [(p.name, p.default) for p in base] == [("filters", [14, 16]), ("kernel_width", [7, 7]), ("dnn_maps", [3, 3]),
                                                   ("pooling_width", [2, 2])]


def test_parameter_names_shapes_and_initialisers():
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.FGCNNLayer(feature_dims=100)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    want = {"embedding_layer.embeddings": (100, 16),
            "fgcnn_layer.conv_layers.0.kernel": (7, 1, 1, 14), "fgcnn_layer.conv_layers.0.bias": (14,),
            "fgcnn_layer.conv_layers.1.kernel": (7, 1, 14, 16), "fgcnn_layer.conv_layers.1.bias": (16,),
            "fgcnn_layer.dense_layers.0.kernel": (5 * 16 * 14, 240), "fgcnn_layer.dense_layers.0.bias": (240,),
            "fgcnn_layer.dense_layers.1.kernel": (2 * 16 * 16, 240), "fgcnn_layer.dense_layers.1.bias": (240,),
            "MLP_layer2.kernel_0": (8, 1), "MLP_layer2.bias_0": (1,)}
    for i, (a, b) in enumerate([(10 * 16 + 240 + 240 + 3, 64), (64, 8)]):
        want.update({"MLP_layer1.kernel_%d" % i: (a, b), "MLP_layer1.bias_%d" % i: (b,),
                     "MLP_layer1.bn_%d.gamma" % i: (b,), "MLP_layer1.bn_%d.beta" % i: (b,)})
    assert shapes == want
    assert shapes["MLP_layer1.kernel_0"][0] == 643
    assert shapes["fgcnn_layer.dense_layers.0.kernel"][0] == 1120 and shapes["fgcnn_layer.dense_layers.1.kernel"][0] == 512
    base = lay.fgcnn_layer
    assert isinstance(base, CL.FGCNNBaseLayer)
    assert base.heights == [5, 2] and base.dense_units == [240, 240] and base.new_fields == [15, 15]
    amax = lambda t: float(t.detach().abs().max())
    c0, c1 = base.conv_layers
    assert 0 < amax(c0.kernel) <= np.sqrt(6.0 / (7 + 7 * 14)) and 0 < amax(c1.kernel) <= np.sqrt(6.0 / (7 * 14 + 7 * 16))
    d0, d1 = base.dense_layers
    assert 0 < amax(d0.kernel) <= np.sqrt(6.0 / (1120 + 240)) and 0 < amax(d1.kernel) <= np.sqrt(6.0 / (512 + 240))
    assert amax(c0.bias) == 0 and amax(c1.bias) == 0 and amax(d0.bias) == 0 and amax(d1.bias) == 0
    assert lay.MLP_layer1.is_batch_norm and lay.MLP_layer2.activation == "sigmoid"
    # no continuous features, 11 fields (odd), three layers: U_j counts the 11 fields at every layer
    lay = CL.FGCNNLayer(continuous_features=[], feature_dims=100, filters=[4, 6, 5], kernel_width=[4, 3, 2],
                        dnn_maps=[2, 4, 6], pooling_width=[2, 2, 2], categorical_features=["c%d" % i for i in range(11)])
    assert lay.fgcnn_layer.heights == [5, 2, 1] and lay.fgcnn_layer.dense_units == [176, 352, 528]
    assert tuple(lay.fgcnn_layer.dense_layers[2].kernel.shape) == (1 * 16 * 5, 528)
    assert tuple(lay.MLP_layer1.kernel_0.shape) == (11 * 16 + 176 + 352 + 528, 64)


def test_sublayers_called_alone_raise_and_bad_shapes_are_rejected():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(NotImplementedError):
        CL.FGCNNBaseLayer(input_shape=(10, 16))(torch.zeros(2, 10, 16))
    with pytest.raises(ValueError):
        CL.FGCNNLayer(categorical_features=CAT[:3], feature_dims=10)                  # H = 3 -> 1 -> 0
    with pytest.raises(ValueError):
        CL.FGCNNLayer(feature_dims=10, pooling_width=[2, 6])                          # H_2 = 5 // 6 = 0
    with pytest.raises(ValueError):
        CL.FGCNNLayer(feature_dims=10, pooling_width=[0, 2])
    with pytest.raises(ValueError):                                                   # U = 2 * 12 * 12 // 5 = 57, 57 % 12 != 0
        CL.FGCNNBaseLayer([4], [7], [2], [5], input_shape=(12, 12))
    with pytest.raises(ValueError):
        CL.FGCNNLayer(feature_dims=10, filters=[14, 16], kernel_width=[7])
    with pytest.raises(ValueError):
        CL.FGCNNLayer(feature_dims=10, dnn_maps=[3])
    with pytest.raises(NotImplementedError):
        CL.FGCNNLayer(feature_dims=10, filters=[17, 6])
    with pytest.raises(NotImplementedError):
        CL.FGCNNLayer(feature_dims=10, kernel_width=[9, 2])
    with pytest.raises(NotImplementedError):
        CL.FGCNNLayer(categorical_features=["c%d" % i for i in range(66)], feature_dims=10, pooling_width=[9, 2])
    with pytest.raises(NotImplementedError):
        CL.FGCNNLayer(categorical_features=["c%d" % i for i in range(66)], feature_dims=10)


def test_model_manager_builds_fgcnn_and_honours_model_params():
    """3.DCN/ModelManager.py:85-88."""
    from explicit_tf2_recommendation_amd import data, layers as CL
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(5000, len(CAT)),
                      embedding_dims=16, layer="FGCNN", device="cpu")
    lay = mm.layer
    assert isinstance(lay, CL.FGCNNLayer)
    assert lay.categorical_features == CAT and lay.continuous_features == CONT
    assert tuple(lay.embedding_layer.embeddings.shape) == (mm.feature_dims, 16)
    base = lay.fgcnn_layer
    assert lay.units == [64, 8] and base.filters == [14, 16] and base.kernel_width == [7, 7]
    assert base.dnn_maps == [3, 3] and base.pooling_width == [2, 2]
    assert tuple(lay.MLP_layer1.kernel_0.shape) == (643, 64)
    mm2 = ModelManager(feature_names=CAT + ["a", "b"], data_info=data.data_info(5000, 12), embedding_dims=8,
                       layer="FGCNN", device="cpu",
                       model_params={"units": [16, 4], "filters": [4, 6], "kernel_width": [4, 3], "dnn_maps": [2, 1],
                                     "pooling_width": [3, 2]})
    base = mm2.layer.fgcnn_layer
    assert base.heights == [4, 2] and base.dense_units == [64, 48]
    assert tuple(base.conv_layers[1].kernel.shape) == (3, 1, 4, 6)
    assert tuple(base.dense_layers[1].kernel.shape) == (2 * 8 * 6, 48)
    assert tuple(mm2.layer.MLP_layer1.kernel_0.shape) == (12 * 8 + 64 + 48, 16)
    assert tuple(mm2.layer.MLP_layer2.kernel_0.shape) == (4, 1)
