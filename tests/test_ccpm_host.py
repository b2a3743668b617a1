"""CPU checks of the CCPM layer: the k formula with its embedding-width quirk, TF's SAME padding, the sorted-by-value
pooling and its tie rule, the Flatten order, the two restatements against each other (tests/ccpm_ref.py), the C-ABI status
codes of the CCPM entry points without a GPU, the layer's parameter names and shapes, and ModelManager(layer='CCPM')."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import ccpm_ref as CR

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


@pytest.mark.parametrize("E,L,want", [(16, 2, [8, 3]), (16, 3, [14, 5, 3]), (16, 1, [3]), (8, 1, [3]), (32, 2, [16, 3])])
def test_k_comes_from_the_embedding_width(E, L, want):
    from explicit_tf2_recommendation_amd import ops
    assert ops.ccpm_k(E, L) == want
    assert CR.ccpm_k(E, L) == want


def test_same_padding_puts_the_extra_row_at_the_end():
    """kw = 4 pads 1 / 2 and kw = 2 pads 0 / 1: a kernel that picks tap j gives y[h] = tanh(x[h - top + j])."""
    assert CR.same_pad(4) == (1, 2) and CR.same_pad(2) == (0, 1) and CR.same_pad(6) == (2, 3) and CR.same_pad(1) == (0, 0)
    x = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    shifted = {0: [0, 0.1, 0.2, 0.3, 0.4], 1: x, 2: [0.2, 0.3, 0.4, 0.5, 0], 3: [0.3, 0.4, 0.5, 0, 0]}
    for j, want in shifted.items():
        K = np.zeros((4, 1, 1, 1))
        K[j] = 1.0
        y, _ = CR.conv_numpy(x.reshape(1, 5, 1, 1), K, np.zeros(1))
        np.testing.assert_allclose(y.reshape(-1), np.tanh(want), rtol=1e-15)
        yt = CR.conv_torch(torch.from_numpy(x).reshape(1, 5, 1, 1), torch.from_numpy(K), torch.zeros(1, dtype=torch.float64))
        np.testing.assert_allclose(yt.numpy().reshape(-1), np.tanh(want), rtol=1e-15)
    for j, want in {0: x, 1: [0.2, 0.3, 0.4, 0.5, 0]}.items():
        K = np.zeros((2, 1, 1, 1))
        K[j] = 1.0
        y, _ = CR.conv_numpy(x.reshape(1, 5, 1, 1), K, np.zeros(1))
        np.testing.assert_allclose(y.reshape(-1), np.tanh(want), rtol=1e-15)
        yt = CR.conv_torch(torch.from_numpy(x).reshape(1, 5, 1, 1), torch.from_numpy(K), torch.zeros(1, dtype=torch.float64))
        np.testing.assert_allclose(yt.numpy().reshape(-1), np.tanh(want), rtol=1e-15)


def test_pooling_sorts_by_value_and_ties_go_to_the_lower_field():
    y = np.array([0.1, 0.9, 0.3, 0.9, 0.5]).reshape(1, 5, 1, 1)
    v, idx, _ = CR.kmax_numpy(y, 3)
    assert v.reshape(-1).tolist() == [0.9, 0.9, 0.5]                  # by value, not in field order (0.9, 0.9, 0.5 sits
    assert idx.reshape(-1).tolist() == [1, 3, 4]                      # at fields 1, 3, 4; field order would agree here)
    y2 = np.array([0.5, 0.1, 0.9]).reshape(1, 3, 1, 1)
    assert CR.kmax_numpy(y2, 2)[0].reshape(-1).tolist() == [0.9, 0.5]  # field order would give [0.5, 0.9]
    t = torch.from_numpy(y2).requires_grad_()
    assert CR.kmax_torch(t, 2).reshape(-1).tolist() == [0.9, 0.5]
    # equal values: k = 1 of [a, a, a] routes the gradient to field 0
    t = torch.full((1, 3, 1, 1), 0.25, dtype=torch.float64, requires_grad=True)
    CR.kmax_torch(t, 1).sum().backward()
    assert t.grad.reshape(-1).tolist() == [1.0, 0.0, 0.0]
    # and through the whole stack: identical rows, kw = 1, so every position ties
    rows = np.full((1, 4, 2), 0.3)
    params = [(np.full((1, 1, 1, 1), 0.7), np.zeros(1))]
    ref = CR.ccpm_numpy(rows, params, [3], np.ones((1, 3 * 2)))
    assert np.count_nonzero(ref["drows"][0, 3]) == 0 and np.count_nonzero(ref["drows"][0, :3]) == 6
    _, drows, _ = CR.ccpm_torch_grads(rows, params, [3], np.ones((1, 6)), torch.float64)
    np.testing.assert_allclose(drows, ref["drows"], rtol=1e-14)


def test_flatten_order_is_h_then_e_then_c():
    """A table whose entries encode (h, e), identity-like kernels whose channel c scales by (c + 1), kw = 1 and k = F:
    out[(r E + e) C + c] is channel c of embedding dim e of the r-th largest field."""
    F, E, Cn = 3, 4, 2
    rows = np.zeros((1, F, E))
    for h in range(F):
        for e in range(E):
            rows[0, h, e] = 0.01 * (h + 1) + 0.001 * e
    K = np.zeros((1, 1, 1, Cn))
    K[0, 0, 0] = [1.0, 2.0]
    out = CR.ccpm_numpy(rows, [(K, np.zeros(Cn))], [F])["out"][0]
    assert out.shape == (F * E * Cn,)
    for r in range(F):
        h = F - 1 - r                                               # descending: the last field is the largest
        for e in range(E):
            for c in range(Cn):
                assert out[(r * E + e) * Cn + c] == pytest.approx(np.tanh((c + 1) * rows[0, h, e]), rel=1e-14)
    t = CR.ccpm_torch(torch.from_numpy(rows), [torch.from_numpy(K), torch.zeros(Cn, dtype=torch.float64)], [F])
    np.testing.assert_allclose(t.numpy()[0], out, rtol=1e-14)


@pytest.mark.parametrize("B,F,E,filters,kw", [(5, 10, 16, [4, 6], [4, 2]), (3, 14, 16, [4, 6, 5], [4, 3, 2]),
                                             (4, 3, 1, [1], [1]), (2, 20, 40, [3, 2], [5, 6]), (3, 12, 12, [4], [7]),
                                             (4, 8, 16, [4, 6], [1, 1]), (2, 27, 16, [16, 16], [8, 3])])
def test_restatements_agree_on_values_and_gradients(B, F, E, filters, kw):
    r = np.random.default_rng(B * 100 + F)
    rows = r.standard_normal((B, F, E)) * 0.5
    params = [(np.asarray(K, np.float64), np.asarray(b, np.float64)) for K, b in CR.make_params(filters, kw, F + E)]
    ks = CR.ccpm_k(E, len(filters))
    dout = r.uniform(-1, 1, (B, ks[-1] * E * filters[-1]))
    ref = CR.ccpm_numpy(rows, params, ks, dout)
    out, drows, dps = CR.ccpm_torch_grads(rows, params, ks, dout, torch.float64)
    assert ref["out"].shape == (B, 3 * E * filters[-1])
    np.testing.assert_allclose(out, ref["out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(drows, ref["drows"], rtol=1e-9, atol=1e-12)
    flat = [a for kb in ref["dparams"] for a in kb]
    for got, want in zip(dps, flat):
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    assert np.all(ref["gap"] > 0)
    # descending along r for every (e, c)
    x = ref["out"].reshape(B, 3, E, filters[-1])
    assert np.all(x[:, :-1] >= x[:, 1:])


def test_glorot_uniform_counts_the_receptive_field():
    from explicit_tf2_recommendation_amd import layers as CL
    CL.set_init_seed(3)
    K = CL.glorot_uniform((4, 1, 4, 6))
    lim = np.sqrt(6.0 / (4 * 4 + 4 * 6))
    assert tuple(K.shape) == (4, 1, 4, 6) and 0.8 * lim < float(K.abs().max()) <= lim
    K = CL.glorot_uniform((8, 1, 1, 16))
    lim = np.sqrt(6.0 / (8 + 8 * 16))
    assert 0.8 * lim < float(K.abs().max()) <= lim
    assert float(CL.glorot_uniform((300, 20)).abs().max()) <= np.sqrt(6.0 / 320)        # 2-D: unchanged


def _ABI():
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


def _ints(v):
    return (C.c_int * len(v))(*v)


def test_ccpm_abi_rejects_bad_arguments_without_a_gpu():
    lib = _ABI()
    assert lib.rec_version() == 105
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    FI, KW, KS = [4, 6], [4, 2], [8, 3]

    def fwd(tab=d, V=100, E=16, ld=16, X=d, B=4, F=10, fi=FI, kw=KW, ks=KS, par=d, out=d, rows=d, oob=d, L=None):
        return lib.rec_emb_ccpm_fwd_f32(tab, V, E, ld, X, B, F, len(fi) if L is None else L, _ints(fi), _ints(kw),
                                        _ints(ks), par, out, rows, oob, None)

    def bwd(tab=d, V=100, E=16, ld=16, X=d, B=4, F=10, fi=FI, kw=KW, ks=KS, par=d, rows=d, do=d, vals=d, dpar=d, ws=d,
            nbytes=1 << 30, L=None):
        return lib.rec_emb_ccpm_bwd_f32(tab, V, E, ld, X, B, F, len(fi) if L is None else L, _ints(fi), _ints(kw),
                                        _ints(ks), par, rows, do, vals, dpar, ws, nbytes, None)

    for k in ("tab", "X", "par", "out"):
        assert fwd(**{k: None}) == -1, k
    for k in ("par", "do", "vals", "dpar", "ws"):
        assert bwd(**{k: None}) == -1, k
    assert bwd(rows=None, tab=None) == -1 and bwd(rows=None, X=None) == -1
    assert lib.rec_emb_ccpm_fwd_f32(d, 100, 16, 16, d, 4, 10, 2, None, _ints(KW), _ints(KS), d, d, d, d, None) == -1
    # NULL is fine where it is not read: everything at B = 0
    assert fwd(B=0, tab=None, X=None, par=None, out=None, rows=None, oob=None) == 0
    assert bwd(B=0, tab=None, X=None, par=None, rows=None, do=None, vals=None, dpar=None, ws=None) == 0
    # negative sizes, an empty table, a row stride below E
    assert fwd(B=-1) == -1 and fwd(F=-1) == -1 and fwd(E=-2) == -1 and fwd(L=-1) == -1 and fwd(V=0) == -1
    assert fwd(fi=[4, -6]) == -1 and fwd(kw=[-4, 2]) == -1 and fwd(ks=[8, -3]) == -1
    assert fwd(ld=8) == -1 and bwd(B=-5) == -1 and bwd(V=-1) == -1 and bwd(ld=15) == -1
    # a pooling over fewer values than k, as tf.nn.top_k refuses it
    assert fwd(F=6) == -1 and bwd(F=6) == -1 and fwd(ks=[8, 9]) == -1
    # unsupported shapes
    assert fwd(F=0) == -2 and fwd(F=65, ks=[8, 3]) == -2 and fwd(E=65, ld=65) == -2 and fwd(E=0) == -2
    assert fwd(fi=[17, 6]) == -2 and fwd(kw=[9, 2]) == -2 and fwd(fi=[0, 6]) == -2 and fwd(kw=[4, 0]) == -2
    assert fwd(ks=[0, 3]) == -2 and fwd(V=1 << 31) == -2 and fwd(L=0) == -2
    assert fwd(fi=[4] * 4, kw=[2] * 4, ks=[8, 3, 3, 3]) == -2
    assert bwd(fi=[17, 6]) == -2 and bwd(F=65) == -2 and bwd(L=0) == -2
    # a column state beyond the LDS of a CU
    assert fwd(F=64, E=64, ld=64, fi=[16, 16, 16], kw=[8, 8, 8], ks=[56, 32, 3]) == -2
    assert lib.rec_ccpm_workspace_bytes(4, 64, 64, 3, _ints([16] * 3), _ints([8] * 3), _ints([56, 32, 3])) == 0
    # a workspace below rec_ccpm_workspace_bytes
    assert bwd(nbytes=16) == -3
    assert lib.rec_ccpm_workspace_bytes(4, 6, 16, 2, _ints(FI), _ints(KW), _ints(KS)) == 0
    assert lib.rec_ccpm_workspace_bytes(-1, 10, 16, 2, _ints(FI), _ints(KW), _ints(KS)) == 0
    assert lib.rec_ccpm_workspace_bytes(4, 10, 16, 2, _ints([4, 17]), _ints(KW), _ints(KS)) == 0
    assert lib.rec_ccpm_workspace_bytes(4, 10, 16, 2, None, None, None) == 0


@pytest.mark.parametrize("B,F", [(16384, 10), (8192, 26)])
def test_ccpm_workspace_is_positive_for_the_bench_configs(B, F):
    """CC (10 fields, B = 16384) and CC26 (26 fields, B = 8192), E = 16, default filters."""
    lib = _ABI()
    n = lib.rec_ccpm_workspace_bytes(B, F, 16, 2, _ints([4, 6]), _ints([4, 2]), _ints([8, 3]))
    assert 0 < n < 64 << 20
    # the corners of the tested envelope
    assert lib.rec_ccpm_workspace_bytes(17, 64, 64, 2, _ints([4, 6]), _ints([4, 2]), _ints([32, 3])) > 0
    assert lib.rec_ccpm_workspace_bytes(1000, 27, 16, 2, _ints([16, 16]), _ints([8, 3]), _ints([8, 3])) > 0
    assert lib.rec_ccpm_workspace_bytes(2, 14, 16, 3, _ints([4, 6, 5]), _ints([4, 3, 2]), _ints([14, 5, 3])) > 0
    assert lib.rec_ccpm_workspace_bytes(1, 3, 1, 1, _ints([1]), _ints([1]), _ints([3])) > 0


@pytest.mark.parametrize("filters,kw", [([1], [1]), ([4, 6], [4, 2]), ([4, 6, 5], [4, 3, 2])])
def test_flat_params_round_trip_through_the_weights_shapes(filters, kw):
    """The pair CCPM and FGCNN share: _flatten_weights lays [K_1, b_1, K_2, ...] out as the kernels read them,
    field_conv_param_count counts that layout, and _split_like gives every weight back in its own shape."""
    from explicit_tf2_recommendation_amd import functional as Fn, ops
    params = CR.make_params(filters, kw, 7)
    weights = [torch.from_numpy(a) for kb in params for a in kb]
    flat, shapes = Fn._flatten_weights(weights)
    assert flat.dim() == 1 and flat.numel() == ops.field_conv_param_count(filters, kw)
    assert shapes == [s for k, cin, c in zip(kw, [1] + filters[:-1], filters) for s in ((k, 1, cin, c), (c,))]
    np.testing.assert_array_equal(flat.numpy(), CR.flat_params(params))
    back = Fn._split_like(flat, shapes)
    assert len(back) == len(weights)
    for got, want in zip(back, weights):
        assert got.shape == want.shape and torch.equal(got, want)


def test_signatures_keep_the_reference_keywords():
    """3.DCN/CustomLayers.py:622, :646 and :681-684."""
    from explicit_tf2_recommendation_amd import layers as CL
    params = list(inspect.signature(CL.CCPMLayer.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                        "units", "activation", "is_batch_norm", "filters", "kernel_width"]
    d = {p.name: p.default for p in params}
    assert d["categorical_features"] == CAT and d["continuous_features"] == CONT
    assert (d["feature_dims"], d["embedding_dims"], d["units"], d["activation"], d["is_batch_norm"], d["filters"],
            d["kernel_width"]) == (150000, 16, [64, 32, 8], "relu", True, [4, 6], [4, 2])
    base = list(inspect.signature(CL.CCPMBaseLayer.__init__).parameters.values())[1:3]
    assert [(p.name, p.default) for p in base] == [("filters", [4, 6]), ("kernel_width", [4, 2])]
    assert list(inspect.signature(CL.KMaxPool.__init__).parameters)[1] == "k"


def test_parameter_names_shapes_and_initialisers():
    from explicit_tf2_recommendation_amd import layers as CL
    lay = CL.CCPMLayer(feature_dims=100)
    shapes = {k: tuple(v.shape) for k, v in lay.named_parameters()}
    want = {"embedding_layer.embeddings": (100, 16),
            "ccpm_layer.conv_layers.0.kernel": (4, 1, 1, 4), "ccpm_layer.conv_layers.0.bias": (4,),
            "ccpm_layer.conv_layers.1.kernel": (2, 1, 4, 6), "ccpm_layer.conv_layers.1.bias": (6,),
            "MLP_layer2.kernel_0": (8, 1), "MLP_layer2.bias_0": (1,)}
    for i, (a, b) in enumerate([(3 * 16 * 6 + 3, 64), (64, 32), (32, 8)]):
        want.update({"MLP_layer1.kernel_%d" % i: (a, b), "MLP_layer1.bias_%d" % i: (b,),
                     "MLP_layer1.bn_%d.gamma" % i: (b,), "MLP_layer1.bn_%d.beta" % i: (b,)})
    assert shapes == want
    assert shapes["MLP_layer1.kernel_0"][0] == 291
    for n in ("ccpm_layer", "embedding_layer", "MLP_layer1", "MLP_layer2"):
        assert hasattr(lay, n)
    assert isinstance(lay.ccpm_layer, CL.CCPMBaseLayer) and [p.k for p in lay.ccpm_layer.kmax_layers] == [8, 3]
    assert all(isinstance(p, CL.KMaxPool) for p in lay.ccpm_layer.kmax_layers)
    amax = lambda t: float(t.detach().abs().max())
    c0, c1 = lay.ccpm_layer.conv_layers
    assert 0 < amax(c0.kernel) <= np.sqrt(6.0 / (4 + 16)) and 0 < amax(c1.kernel) <= np.sqrt(6.0 / (8 + 12))
    assert amax(c0.bias) == 0 and amax(c1.bias) == 0
    assert lay.MLP_layer1.is_batch_norm and lay.MLP_layer2.activation == "sigmoid"
    # no continuous features: as FiBiNetLayer, the block is simply absent
    lay = CL.CCPMLayer(continuous_features=[], feature_dims=100, filters=[4, 6, 5], kernel_width=[4, 3, 2],
                       categorical_features=["c%d" % i for i in range(14)])
    assert tuple(lay.MLP_layer1.kernel_0.shape) == (3 * 16 * 5, 64)
    assert [p.k for p in lay.ccpm_layer.kmax_layers] == [14, 5, 3]


def test_sublayers_called_alone_raise_and_bad_shapes_are_rejected():
    from explicit_tf2_recommendation_amd import layers as CL
    with pytest.raises(NotImplementedError):
        CL.KMaxPool(3)(torch.zeros(2, 5, 4, 1))
    with pytest.raises(NotImplementedError):
        CL.CCPMBaseLayer(input_shape=(10, 16))(torch.zeros(2, 10, 16))
    with pytest.raises(ValueError):
        CL.CCPMLayer(categorical_features=CAT[:6], feature_dims=10)                  # k_1 = 8 of 6 fields
    with pytest.raises(ValueError):
        CL.CCPMLayer(feature_dims=10, embedding_dims=1)                              # k_1 = 1, k_2 = 3 of 1
    with pytest.raises(ValueError):
        CL.CCPMLayer(feature_dims=10, filters=[4, 6], kernel_width=[4])
    with pytest.raises(NotImplementedError):
        CL.CCPMLayer(feature_dims=10, filters=[17, 6])
    with pytest.raises(NotImplementedError):
        CL.CCPMLayer(feature_dims=10, kernel_width=[9, 2])
    with pytest.raises(NotImplementedError):
        CL.CCPMLayer(categorical_features=["c%d" % i for i in range(65)], feature_dims=10)


def test_model_manager_builds_ccpm_and_honours_model_params():
    """3.DCN/ModelManager.py:82-84."""
    from explicit_tf2_recommendation_amd import data, layers as CL
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(5000, len(CAT)),
                      embedding_dims=16, layer="CCPM", device="cpu")
    lay = mm.layer
    assert isinstance(lay, CL.CCPMLayer)
    assert lay.categorical_features == CAT and lay.continuous_features == CONT
    assert tuple(lay.embedding_layer.embeddings.shape) == (mm.feature_dims, 16)
    assert lay.units == [64, 32, 8] and lay.ccpm_layer.filters == [4, 6] and lay.ccpm_layer.kernel_width == [4, 2]
    assert tuple(lay.MLP_layer1.kernel_0.shape) == (291, 64)
    mm2 = ModelManager(feature_names=CAT + ["a", "b", "c", "d"], data_info=data.data_info(5000, 14), embedding_dims=16,
                       layer="CCPM", device="cpu",
                       model_params={"units": [16, 4], "filters": [4, 6, 5], "kernel_width": [4, 3, 2]})
    assert tuple(mm2.layer.ccpm_layer.conv_layers[2].kernel.shape) == (2, 1, 6, 5)
    assert tuple(mm2.layer.MLP_layer1.kernel_0.shape) == (3 * 16 * 5, 16)
    assert tuple(mm2.layer.MLP_layer2.kernel_0.shape) == (4, 1)
