"""ETA without a GPU: the oracle of tests/eta_ref.py on a hand-worked case and on its own two kinds of input, the ABI of
csrc/eta.hip from the sizes alone (names, signatures, the size query, the return codes in their documented order),
ops.eta_check_shape, and eta.ETALayer(fused=False) on CPU tensors against the torch transcription: shapes, state-dict
keys, the frozen projection, which table rows receive a gradient, both mask modes, the untouched input dict and the
constructor's signature."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import eta_ref as ER

F32 = np.float32


# ---- the oracle -------------------------------------------------------------------------------------------------------
def test_the_oracle_on_a_hand_worked_case():
    """H = I: the code of a row is the sign of its two coordinates.  Rows: 0 (0,0), 1 (1,-1), 2 (1,1), 3 (0,-1),
    4 (-1,1).  Example 0, item row 1 = (+,-): steps 2, 1, pad, 1 score 1, 2, 0, 2 and rank 1, 2, -inf, 2 -> 1, 3, 0.
    Example 1, item row 0 = (0,0): steps 3, pad, pad, 4 score 1, 2, 2, 0; the padded ones rank last, in index order."""
    table = np.array([[0, 0], [1, -1], [2, 3], [0, -1], [-4, 0.5]], F32)
    series = np.array([[[2], [1], [0], [1]], [[3], [0], [0], [4]]])
    q = table[[1, 0]]
    r = ER.search_numpy(table, series, q, np.eye(2, dtype=F32), 0, 3)
    assert r["scores"].tolist() == [[1, 2, 0, 2], [1, 2, 2, 0]]
    assert r["chosen"].tolist() == [[1, 3, 0], [0, 3, 1]]
    assert r["sel_valid"].tolist() == [[1, 1, 1], [1, 1, 0]]
    assert r["sel_ids"].tolist() == [[[1], [1], [2]], [[3], [4], [0]]]
    assert np.array_equal(r["sel"][1], table[[3, 4, 0]])
    assert r["scores"].dtype == np.int32 and r["chosen"].dtype == np.int32 and r["sel_ids"].dtype == np.int64
    # a NaN row equals nothing, not even itself; an id out of range reads the zero row
    table[2] = np.nan
    r = ER.search_numpy(table, np.array([[[2], [7], [-1]]]), table[[2]], np.eye(2, dtype=F32), 0, 3)
    assert r["scores"].tolist() == [[0, 0, 0]] and r["chosen"].tolist() == [[0, 1, 2]]
    r = ER.search_numpy(table, np.array([[[2], [7], [-1]]]), table[[0]], np.eye(2, dtype=F32), 0, 3)
    assert r["scores"].tolist() == [[0, 2, 2]] and r["chosen"].tolist() == [[1, 2, 0]]
    assert not r["sel"][0, :2].any() and r["sel_ids"].tolist() == [[[7], [-1], [2]]]


@pytest.mark.parametrize("case", ER.CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_inputs_are_exact_in_fp32_and_make_the_rows_the_tests_need(case):
    B, T, Cn, E, m, K, D = ER.dims(case)
    c = ER.inputs(case)
    x = ER.keys_of(c["table"], c["series"])
    p64 = ER.projections(x, c["H"])
    for order in (slice(None), slice(None, None, -1)):                       # fp32, summed forwards and backwards
        p32 = np.zeros(p64.shape, F32)
        for d in range(D)[order]:
            p32 = (p32 + x[..., d, None] * c["H"][d]).astype(F32)
        assert np.array_equal(p32.astype(np.float64), p64)
    r = ER.reference(case)
    assert r["chosen"].shape == (B, K) and all(len(set(row)) == K for row in r["chosen"].tolist())
    if B >= 4:
        assert r["valid"][0].all() and r["chosen"][0].tolist() == list(range(K))           # all steps identical
        assert not r["valid"][1].any() and r["chosen"][1].tolist() == list(range(K)) and not r["sel_valid"][1].any()
        assert r["valid"][2].sum() == 1 and r["sel_valid"][2].tolist() == [1] + [0] * (K - 1)
        assert not c["q"][3].any() and (r["scores"][3] == (np.sign(p64[3]) == 0).sum(-1)).all()
    if B * T >= 300:
        pad0 = c["series"][:, :, 0] == 0
        assert (pad0 & (c["series"][:, :, 1:] != 0).any(-1)).any() or Cn == 1              # padded by the first column alone
        assert (p64 == 0).any() and (c["series"] == ER.ZERO_ROW).all(-1).any()


def test_random_inputs_leave_out_at_most_a_tenth():
    for case in ER.RANDOM_CASES:
        c = ER.inputs(case, "random")
        share = ER.undecided(c["table"], c["series"], c["q"], c["H"], 0).mean()
        print(case, "left out: %.3f" % share)
        assert share <= ER.MAX_LEFT_OUT
    for seed in (1, 2, 3, 4):
        sd = ER.layer_state(seed)
        for T, S in ((20, 5), (6, 20), (2, 3)):
            assert ER.layer_undecided(sd, ER.layer_inputs(seed, ER.LAYER_B, T, S)).mean() <= ER.MAX_LEFT_OUT


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_names_and_signatures():
    from explicit_tf2_recommendation_amd import _lib
    p, i, l, z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    want = {"rec_eta_search_lds_bytes": (z, [i, i, i, i, i]),
            "rec_eta_search_fwd_f32": (i, [p, l, l, i, i, p, l, i, p, l, p, i, l, i, p, p, p, p, p, p, p])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert hasattr(_lib.lib, name)
    assert not [n for n in _lib.SIGNATURES if n.startswith("rec_eta_") and n not in want]      # no backward kernel
    # the family's one limit of its own is a define of the header (key width, top-k and launch cap are the searches')
    assert {k: v for k, v in _lib.LIMITS.items() if "ETA" in k} == {"REC_ETA_MAX_M": 32}


def test_size_query_and_the_supported_range():
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import lib
    for T, Cn, E, m, K in ((1, 1, 2, 1, 1), (10, 3, 16, 16, 3), (2048, 3, 16, 16, 3), (2048, 3, 16, 32, 16),
                           (257, 1, 256, 32, 16), (15000, 3, 16, 16, 3), (14000, 3, 16, 17, 3)):
        assert lib.rec_eta_search_lds_bytes(T, Cn, E, m, K) == ops.eta_search_lds_bytes(T, Cn * E, m) <= 64 * 1024
    assert lib.rec_eta_search_lds_bytes(2048, 3, 16, 16, 3) == 4 * (48 * 16 + 2048 + 16)
    assert lib.rec_eta_search_lds_bytes(2048, 3, 16, 17, 3) == 4 * (48 * 32 + 2048 + 16)
    assert lib.rec_eta_search_lds_bytes(16384, 3, 16, 16, 3) == 0                # the LDS rule
    assert lib.rec_eta_search_lds_bytes(10, 3, 86, 16, 3) == 0                   # D = 258
    assert lib.rec_eta_search_lds_bytes(100, 3, 16, 33, 3) == 0                  # m = 33
    assert lib.rec_eta_search_lds_bytes(100, 3, 16, 16, 17) == 0                 # K = 17
    assert lib.rec_eta_search_lds_bytes(2, 3, 16, 16, 3) == 0 and lib.rec_eta_search_lds_bytes(0, 3, 16, 16, 1) == 0


def _search(lib, **kw):
    d = C.c_void_p(4096)                                                       # never dereferenced
    a = dict(embed=d, ld=16, V=10, E=16, C=3, series=d, B=4, T=6, q=d, ld_q=48, Hm=d, m=16, pad=0, K=3, scores=d,
             chosen=d, sel=d, sel_valid=d, sel_ids=d, oob=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib.rec_eta_search_fwd_f32(*a.values(), None)


def test_abi_errors_in_the_documented_order():
    """On a CPU-only load of the library every call returns before any launch."""
    from explicit_tf2_recommendation_amd._lib import lib
    for kw in (dict(T=0), dict(B=-1), dict(K=0), dict(E=0), dict(C=0), dict(V=0), dict(m=0), dict(T=0, K=17),
               dict(m=-1, E=86)):
        assert _search(lib, **kw) == -1, kw                                    # a size below 1 first, whatever else
    for kw in (dict(K=17, T=20), dict(E=86, ld=86, ld_q=258), dict(m=33), dict(T=16384), dict(B=2 ** 31), dict(V=2 ** 31),
               dict(K=17, T=20, q=None), dict(m=33, ld=15), dict(B=0, m=33)):
        assert _search(lib, **kw) == -2, kw                                    # one shape past each limit, from the sizes
    for kw in (dict(ld=15), dict(ld_q=47), dict(K=7), dict(embed=None), dict(series=None), dict(q=None), dict(Hm=None),
               dict(chosen=None), dict(sel=None), dict(sel_valid=None), dict(sel_ids=None), dict(B=0, ld=15)):
        assert _search(lib, **kw) == -1, kw
    assert _search(lib, B=0) == 0
    assert _search(lib, B=0, embed=None, series=None, q=None, Hm=None, chosen=None, sel=None, sel_ids=None) == 0
    for kw in (dict(m=32, K=6, B=0), dict(m=1, B=0), dict(E=64, C=4, ld=64, ld_q=256, B=0), dict(T=15000, B=0)):
        assert _search(lib, **kw) == 0, kw                                     # at the limits


def test_check_shape_names_the_limit():
    from explicit_tf2_recommendation_amd import ops
    with pytest.raises(ValueError, match="positive"):
        ops.eta_check_shape(0)
    with pytest.raises(ValueError, match="positive"):
        ops.eta_check_shape(48, T=0)
    with pytest.raises(ValueError, match="D=50 with C=3"):
        ops.eta_check_shape(50, C=3)
    ops.eta_check_shape(48, T=2048, K=3, m=16, C=3)
    ops.eta_check_shape(256, T=2048, K=16, m=32, C=1)
    ops.eta_check_shape(2)
    with pytest.raises(NotImplementedError, match="<= 256"):
        ops.eta_check_shape(257)
    with pytest.raises(NotImplementedError, match="lsh_topk <= 16"):
        ops.eta_check_shape(48, K=17)
    with pytest.raises(NotImplementedError, match="lsh_dim <= 32"):
        ops.eta_check_shape(48, m=33)
    with pytest.raises(NotImplementedError, match="LDS.*T=16000"):
        ops.eta_check_shape(48, T=16000, m=17, C=3)
    z = torch.zeros
    with pytest.raises(RuntimeError):                                          # no CPU fallback
        ops.eta_search_fwd(z(5, 4), z(1, 2, 1, dtype=torch.int64), z(1, 4), z(4, 3), 0, 1)


# ---- the layer ----------------------------------------------------------------------------------------------------------
ETA_SIGNATURE = [("user_and_context_categorical_features", ["uid", "utag1", "utag2", "utag3", "utag4"]),
                 ("item_categorical_features", ["label_goods_ids", "label_shop_ids", "label_cate_ids"]),
                 ("longterm_series_features", ["longterm_goods_ids", "longterm_shop_ids", "longterm_cate_ids"]),
                 ("shortterm_series_features", ["shortterm_goods_ids", "shortterm_shop_ids", "shortterm_cate_ids"]),
                 ("feature_dims", 160000), ("embedding_dims", 16), ("padding_index", 0), ("num_heads", 8), ("key_dim", 4),
                 ("activation", "ReLU"), ("lsh_dim", 16), ("lsh_topk", 3), ("mask_mode", "reference"), ("fused", True)]


def test_constructor_signature_defaults_and_limits():
    from explicit_tf2_recommendation_amd import eta, functional, layers
    sig = [(n, q.default) for n, q in list(inspect.signature(eta.ETALayer.__init__).parameters.items())[1:]]
    assert sig == ETA_SIGNATURE
    assert hasattr(functional, "EtaSearch") and not hasattr(layers, "LSHAttention") and not hasattr(eta, "LSHAttention")
    with pytest.raises(AssertionError):
        eta.ETALayer(item_categorical_features=["a", "b"], feature_dims=10)
    with pytest.raises(ValueError):
        eta.ETALayer(mask_mode="padded", feature_dims=10)
    with pytest.raises(NotImplementedError, match="lsh_dim"):
        eta.ETALayer(feature_dims=10, lsh_dim=33)
    with pytest.raises(NotImplementedError, match="<= 64"):
        eta.ETALayer(feature_dims=10, embedding_dims=32)                    # D = 96: the attention kernel's limit
    eta.ETALayer(feature_dims=10, embedding_dims=32, lsh_dim=33, fused=False)           # the composition has none
    lay = eta.ETALayer(feature_dims=50)
    assert lay.fused and lay.mask_mode == "reference" and lay.lsh_topk == 3 and lay.lsh_dim == 16
    assert lay.shortterm_mha.num_heads == 8 and lay.longterm_mha.key_dim == 4 and lay.longterm_mha.input_dim == 48
    assert lay.final_mlp.layers[0].kernel.shape[0] == 8 * 16 + 2 * 48


def _layer(seed, mask_mode="reference", **kw):
    from explicit_tf2_recommendation_amd import eta
    lay = eta.ETALayer(feature_dims=ER.LAYER_V, mask_mode=mask_mode, fused=False, **kw)
    sd = ER.layer_state(seed)
    lay.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return lay, sd


def test_state_dict_keys_initialisation_and_the_frozen_projection():
    from explicit_tf2_recommendation_amd import eta, layers
    layers.set_init_seed(3)
    lay = eta.ETALayer(feature_dims=ER.LAYER_V, fused=False)
    sd = lay.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == ER.state_shapes()
    H = lay.H
    assert H is lay.projection_matrix and tuple(H.shape) == (48, 16) and not H.requires_grad
    assert abs(float(H.std()) - 0.05) < 0.005 and abs(float(H.mean())) < 0.01             # Keras' random_normal
    assert "projection_matrix" not in dict(lay.named_parameters())
    assert all(q is not H for q in lay.trainable_variables) and len(lay.trainable_variables) == len(sd) - 1
    ins = ER.layer_inputs(1, 8, 12, 4)
    ins.pop("weight")
    lay(ins)["output"].sum().backward()
    assert H.grad is None and torch.equal(H, sd["projection_matrix"])


@pytest.mark.parametrize("mask_mode", ("reference", "valid"))
@pytest.mark.parametrize("T,S,k", ((20, 5, 3), (6, 20, 3), (2, 3, 3)), ids=lambda v: str(v))
def test_composed_layer_on_cpu_equals_the_transcription(mask_mode, T, S, k):
    seed, B = 2, ER.LAYER_B
    lay, sd = _layer(seed, mask_mode, lsh_topk=k)
    ins = ER.layer_inputs(seed, B, T, S)
    keep = ~ER.layer_undecided(sd, ins)
    assert keep.mean() >= 1 - ER.MAX_LEFT_OUT
    weight = ins.pop("weight") * keep[:, None]
    t64, t32 = (ER.eta_layer_torch(sd, ins, dt, mask_mode, k, weight) for dt in (torch.float64, torch.float32))
    assert np.array_equal(t64["chosen"][keep], t32["chosen"][keep])
    before = {n: np.array(v, copy=True) for n, v in ins.items()}
    res = lay({n: torch.from_numpy(v) for n, v in ins.items()})
    assert res.keys() == {"output"} and tuple(res["output"].shape) == (B, 1)
    assert ins.keys() == before.keys() and all(np.array_equal(ins[n], before[n]) for n in ins)     # not mutated
    assert ER.rel_err(res["output"].detach().numpy()[keep], t64["output"][keep]) <= 1e-5
    (res["output"] * torch.from_numpy(weight)).sum().backward()
    grads = {n: q.grad.numpy() for n, q in lay.named_parameters()}
    assert grads.keys() == t64["grads"].keys()
    for n, g in grads.items():
        scale = np.abs(t64["grads"][n.replace("_key_dense", "_query_dense")]).max() if n.endswith("_key_dense.bias") else None
        err = np.abs(g - t64["grads"][n]).max() / (scale or np.abs(t64["grads"][n]).max() or 1.0)
        assert err <= 3e-5, (n, err)
    # only the item, user, short-term and SELECTED long-term ids receive a gradient
    long_ids = np.stack([ins[n] for n in ER.LONG], -1)
    chosen = t64["chosen"][keep]
    touched = set(long_ids[keep][np.arange(len(chosen))[:, None], chosen].reshape(-1).tolist())
    for names in (ER.ITEM, ER.USER, ER.SHORT):
        touched |= set(np.stack([ins[n] for n in names], -1)[keep].reshape(-1).tolist())
    got = set(np.flatnonzero(np.abs(grads["embed.embeddings"]).sum(1)).tolist())
    assert got <= touched                                  # (a masked position's row is touched and gets exactly zero)
    assert set(np.stack([ins[n] for n in ER.ITEM + ER.USER], -1)[keep].reshape(-1).tolist()) <= got
    unselected = set(long_ids.reshape(-1).tolist()) - touched
    assert (unselected or T < 20) and not got & unselected


def test_mask_modes_differ_on_left_padded_series_only():
    seed, B = 3, ER.LAYER_B
    outs = {}
    for left in (True, False):
        ins = ER.layer_inputs(seed, B, 8, 6, left_padded=left)
        ins.pop("weight")
        for mode in ("reference", "valid"):
            lay, _ = _layer(seed, mode)
            outs[left, mode] = lay({n: torch.from_numpy(v) for n, v in ins.items()})["output"].detach()
    assert not torch.equal(outs[True, "reference"], outs[True, "valid"])
    assert torch.equal(outs[False, "reference"], outs[False, "valid"])         # a prefix of valid steps IS the valid steps


def test_fused_layer_has_no_cpu_fallback_and_cpu_ids_out_of_range_raise():
    from explicit_tf2_recommendation_amd import eta
    ins = ER.layer_inputs(1, 4, 5, 3)
    ins.pop("weight")
    with pytest.raises(RuntimeError):
        eta.ETALayer(feature_dims=ER.LAYER_V)({n: torch.from_numpy(v) for n, v in ins.items()})
    lay, _ = _layer(1)
    ins["longterm_shop_ids"][2, 1] = ER.LAYER_V
    with pytest.raises(IndexError):
        lay({n: torch.from_numpy(v) for n, v in ins.items()})
