"""ComiRec without a GPU: the hand-derived fp64 backward of tests/comirec_ref.py against torch-fp64 autograd for the three
families, finiteness at 0, 1, 2 and T padded positions, that the generated cases really exercise the routing, the tie rule
of the hard attention, the positional table, the argument and limit errors of the C ABI (B == 0: nothing is launched), the
constructor signatures, the state-dict names, the error paths of the layer and the seed / exclusion rules of the kink."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import comirec_ref as CR

ids = lambda c: "x".join(map(str, c))
KEEPS = (0, 1)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", CR.DR_CASES, ids=ids)
def test_routing_backward_by_hand_equals_autograd_fp64(case, keep):
    ref, t64 = CR.dr_ref(case, keep), CR.dr_case_t(case, keep, torch.float64)
    for name in ("out", "gkeys", "dW"):
        assert np.all(np.isfinite(ref[name])), name
        assert CR.rel_err(ref[name], t64[name]) <= 1e-12, name


@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", CR.SA_CASES, ids=ids)
def test_self_attention_backward_by_hand_equals_autograd_fp64(case, keep, with_pos):
    ref, t64 = CR.sa_ref(case, keep, with_pos), CR.sa_case_t(case, keep, with_pos, torch.float64)
    for name in ("out", "gkeys", "dW1", "dW2"):
        assert np.all(np.isfinite(ref[name])), name
        assert CR.rel_err(ref[name], t64[name]) <= 1e-12, name


@pytest.mark.parametrize("case", CR.SELECT_CASES, ids=ids)
@pytest.mark.parametrize("way", list(CR.SELECT_WAYS) + ["both+gsel"])
def test_select_backward_by_hand_equals_autograd_fp64(case, way):
    c = CR.select_case(*case)
    up = CR.select_way(c, way.split("+")[0], way.endswith("gsel"))
    ref = CR.select_numpy(c["table"], c["items"], c["m"], *up)
    t64 = CR.select_torch_grads(c["table"], c["items"], c["m"], *up, torch.float64)
    assert np.array_equal(ref["chosen"], t64["chosen"])
    for name in ("inner", "loss", "gm", "gitems"):
        assert np.all(np.isfinite(ref[name])), name
        assert CR.rel_err(ref[name], t64[name]) <= 1e-12, name


def test_first_examples_have_0_1_2_and_T_padded_positions_and_stay_finite():
    for case in CR.DR_CASES:
        B, T = case[:2]
        c = CR.dr_inputs(*case)
        n_pad = (c["series"][:, :, 0] == 0).sum(1)
        assert list(n_pad[:4]) == [min(v, T) for v in (0, 1, 2, T)][:B]
        for keep in KEEPS:
            ref = CR.dr_ref(case, keep)
            nobody = 0 if keep else min(3, B - 1)                 # no padded position / every position padded
            if ref["valid"][nobody].sum() == 0:                   # uniform over ALL positions
                assert np.allclose(ref["W"][nobody], 1.0 / T, rtol=0, atol=1e-15)
            for name in ("out", "gkeys", "dW", "W"):
                assert np.all(np.isfinite(ref[name])), (case, keep, name)
    for case in CR.SA_CASES:
        for keep in KEEPS:
            ref = CR.sa_ref(case, keep, True)
            assert all(np.all(np.isfinite(ref[k])) for k in ("out", "gkeys", "dW1", "dW2", "A")), (case, keep)
    c = CR.dr_inputs(33, 50, 3, 16, 48, 4, 3)                     # padding sits anywhere in the row
    pad = c["series"][:, :, 0] == 0
    assert (pad[:, :-1] & ~pad[:, 1:]).any()


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", [c for c in CR.DR_CASES if c[6] >= 2 and c[0] >= 17], ids=ids)
def test_the_cases_exercise_the_routing(case, keep):
    """At least half of the (b, k) rows with two or more participating positions end with weights whose max / min over
    them is >= 2: the agreement updates moved them.  With the reference's stddev 0.05 for W the weights would stay near
    uniform and a kernel that skipped the logit update would pass."""
    share = CR.routed_share(CR.dr_ref(case, keep))
    print("rows with max / min >= 2 over the participating positions: %.2f" % share)
    assert share >= 0.5


def test_tie_rule_is_the_smallest_index_and_the_gradient_lands_on_the_chosen_capsule_alone():
    r = np.random.default_rng(7)
    table = CR.f32_exact(r.normal(0, 0.5, (20, 4)))
    items = r.integers(0, 20, (2, 3, 2)).astype(np.int64)
    m = CR.f32_exact(r.normal(0, 0.5, (2, 3, 8)))
    m[0, 1] = m[0, 2] = m[0, 0]                                   # the capsules of example 0 are equal: every item ties
    ginner, gsel = np.ones((2, 3)), CR.f32_exact(r.normal(0, 1, (2, 3, 8)))
    ref = CR.select_numpy(table, items, m, ginner, None, gsel)
    x = CR.gather(table, items)
    p = np.einsum("bkd,bsd->bsk", m, x)
    assert np.all(p[0, :, 0] == p[0, :, 1]) and not np.any(ref["chosen"][0])         # tf.argmax: the smallest index
    assert ref["gap"][0] == 0.0
    assert np.any(ref["gm"][0, 0]) and not np.any(ref["gm"][0, 1:])                   # the twins of the chosen get nothing
    for b in range(2):
        for k in range(3):
            want = sum(ginner[b, s] * x[b, s] + gsel[b, s] for s in range(3) if ref["chosen"][b, s] == k)
            assert np.allclose(ref["gm"][b, k], want, rtol=1e-13, atol=1e-15)
    t64 = CR.select_torch_grads(table, items, m, ginner, None, gsel, torch.float64)
    assert np.array_equal(t64["chosen"], ref["chosen"]) and CR.rel_err(ref["gm"], t64["gm"]) <= 1e-12


def test_positional_table_is_the_float32_reading_of_the_reference():
    from explicit_tf2_recommendation_amd import layers
    for T, D in ((6, 48), (50, 48), (9, 256), (1, 1), (5, 7)):
        got = layers.comirec_positional_table(T, D)
        assert got.dtype == torch.float32 and tuple(got.shape) == (T, D)
        assert np.array_equal(got.numpy(), CR.positional_table(T, D))
    tab = CR.positional_table(50, 48).astype(np.float64)
    pos, i = np.arange(50)[:, None], np.arange(48)[None, :]
    angle = pos / np.power(10000.0, 2 * (i // 2) / 48.0)
    assert np.abs(tab - np.where(i % 2 == 0, np.sin(angle), np.cos(angle))).max() < 1e-5
    assert np.all(tab[0, 0::2] == 0) and np.all(tab[0, 1::2] == 1)


def _buf(n=64):
    return C.cast(C.create_string_buffer(n), C.c_void_p)


def test_argument_and_limit_errors_of_the_abi():
    """B == 0 throughout (but for the workspace refusals): the entry points answer from the sizes and the pointers alone."""
    from explicit_tf2_recommendation_amd._lib import lib, LIMITS
    from explicit_tf2_recommendation_amd import ops
    max_d, max_k = LIMITS["REC_DIN_MAX_D"], LIMITS["REC_AFM_MAX_A"]
    p = _buf()
    cap = 150 * 1024

    def dr(T=6, E=16, Cn=3, Dc=48, K=4, R=3, ld=None, V=10, null=None):
        ptr = lambda name: None if name == null else p
        ld = E if ld is None else ld
        head = (ptr("embed"), ld, V, E, Cn, ptr("series"), 0, T, ptr("W"), ptr("B0"), Dc, K, R, 0, 1)
        fwd = lib.rec_comirec_dr_fwd_f32(*head, ptr("out"), None, ptr("ws"), 1 << 40, None)
        bwd = lib.rec_comirec_dr_bwd_f32(*head, ptr("out"), ptr("gkeys"), ptr("dW"), ptr("ws"), 1 << 40, None)
        return fwd, bwd, lib.rec_comirec_dr_workspace_bytes(0, T, E, Cn, Dc, K, R)

    fwd, bwd, ws = dr()
    assert (fwd, bwd) == (0, 0) and ws > 0
    assert dr(E=max_d, Cn=1, Dc=max_d, K=max_k, R=3, T=33)[:2] == (0, 0)             # at the width limits
    for kw in (dict(E=max_d + 1, Cn=1), dict(E=max_d // 2 + 1, Cn=2), dict(Dc=max_d + 1), dict(K=max_k + 1), dict(R=9)):
        assert dr(**kw) == (-2, -2, 0), kw
    assert dr(R=8)[:2] == (0, 0)
    # the LDS fit of one row: 4 (T (Dc|1) + (2 R + 3) T + 2 R (Dc|1)) <= 150 KiB; T = 226 at the MIND shape is inside
    assert dr(T=226)[:2] == (0, 0)
    for Dc, R in ((48, 3), (256, 8), (1, 1)):
        t_max = max(t for t in range(1, 40000) if ops.comirec_dr_lds_bytes(t, Dc, R) <= cap)
        assert dr(T=t_max, Dc=Dc, R=R)[:2] == (0, 0) and dr(T=t_max, Dc=Dc, R=R)[2] > 0, (Dc, R, t_max)
        assert dr(T=t_max + 1, Dc=Dc, R=R) == (-2, -2, 0), (Dc, R, t_max)
    assert max(t for t in range(1, 2000) if ops.comirec_dr_lds_bytes(t, 48, 3) <= cap) == 657
    for kw in (dict(T=0), dict(E=0), dict(Cn=0), dict(Dc=0), dict(K=0), dict(R=0), dict(ld=15), dict(V=0)):
        assert dr(**kw)[:2] == (-1, -1), kw
    for name in ("embed", "series", "W", "B0", "out", "ws"):
        assert dr(null=name)[:2] == (-1, -1), name
    for name in ("gkeys", "dW"):
        assert dr(null=name)[:2] == (0, -1), name
    assert lib.rec_comirec_dr_workspace_bytes(-1, 6, 16, 3, 48, 4, 3) == 0
    # the workspace is bounded by a slab, not by the batch
    sizes = [lib.rec_comirec_dr_workspace_bytes(B, 10, 16, 3, 48, 4, 3) for B in (1, 2048, 2049, 100000)]
    assert sizes[0] < sizes[1] and sizes[1] <= sizes[2] == sizes[3]
    head = (p, 16, 10, 16, 3, p, 5, 6, p, p, 48, 4, 3, 0, 1)
    assert lib.rec_comirec_dr_fwd_f32(*head, p, None, p, 64, None) == -3
    assert lib.rec_comirec_dr_bwd_f32(*head, p, p, p, p, 64, None) == -3

    def sa(T=6, E=16, Cn=3, Dc=48, K=4, ld=None, V=10, null=None):
        ptr = lambda name: None if name == null else p
        ld = E if ld is None else ld
        head = (ptr("embed"), ld, V, E, Cn, ptr("series"), 0, T, ptr("W1"), ptr("W2"), ptr("pos"), Dc, K, 0, 1)
        fwd = lib.rec_comirec_sa_fwd_f32(*head, ptr("out"), None, None)
        bwd = lib.rec_comirec_sa_bwd_f32(*head, ptr("out"), ptr("gkeys"), ptr("dW1"), ptr("dW2"), ptr("ws"), 64, None)
        return fwd, bwd, lib.rec_comirec_sa_workspace_bytes(0, T, E, Cn, Dc, K)

    fwd, bwd, ws = sa()
    assert (fwd, bwd) == (0, 0) and ws > 0
    assert sa(null="pos")[:2] == (0, 0)                                               # add_pos_emb=False
    assert sa(E=max_d, Cn=1, Dc=max_d, K=max_k, T=24)[:2] == (0, 0)
    for kw in (dict(E=max_d + 1, Cn=1), dict(Dc=max_d + 1), dict(K=max_k + 1)):
        assert sa(**kw) == (-2, -2, 0), kw
    for D, Dc, K in ((48, 48, 4), (256, 256, 16)):
        t_max = max(t for t in range(1, 40000) if ops.comirec_sa_lds_bytes(t, D, Dc, K) <= cap)
        assert t_max >= (226 if D == 48 else 1)
        kw = dict(E=D // 4, Cn=4, Dc=Dc, K=K)
        assert sa(T=t_max, **kw)[:2] == (0, 0) and sa(T=t_max, **kw)[2] > 0 and sa(T=t_max + 1, **kw) == (-2, -2, 0)
    for kw in (dict(T=0), dict(E=0), dict(Cn=0), dict(Dc=0), dict(K=0), dict(ld=15), dict(V=0)):
        assert sa(**kw)[:2] == (-1, -1), kw
    for name in ("embed", "series", "W1", "W2", "out"):
        assert sa(null=name)[:2] == (-1, -1), name
    for name in ("gkeys", "dW1", "dW2", "ws"):
        assert sa(null=name)[:2] == (0, -1), name
    sizes = [lib.rec_comirec_sa_workspace_bytes(B, 6, 16, 3, 48, 4) for B in (1, 1024, 100000)]
    assert sizes[0] < sizes[1] == sizes[2]
    assert lib.rec_comirec_sa_bwd_f32(p, 16, 10, 16, 3, p, 5, 6, p, p, p, 48, 4, 0, 1, p, p, p, p, p, 64, None) == -3

    def sel(Ns=11, E=16, Cn=3, K=4, ld=None, V=10, null=None, both_null=False):
        ptr = lambda name: None if name == null else p
        ld = E if ld is None else ld
        head = (ptr("embed"), ld, V, E, Cn, ptr("items"), 0, Ns, ptr("m"), K)
        fwd = lib.rec_comirec_select_fwd_f32(*head, ptr("chosen"), ptr("inner"), ptr("loss"), None, None)
        bwd = lib.rec_comirec_select_bwd_f32(*head, ptr("chosen"), None if both_null else ptr("ginner"),
                                             None if both_null else ptr("gloss"), ptr("gsel"), ptr("gm"), ptr("gitems"),
                                             None)
        return fwd, bwd, lib.rec_comirec_select_lds_bytes(Ns, E, Cn, K)

    fwd, bwd, lds = sel()
    assert (fwd, bwd) == (0, 0) and lds == lib.rec_mind_laa_lds_bytes(11, 16, 3, 4) > 0   # the limits of rec_mind_laa_*
    for kw in (dict(E=max_d + 1, Cn=1), dict(K=max_k + 1)):
        assert sel(**kw) == (-2, -2, 0), kw
    ns = max(n for n in range(1, 200) if ops.mind_laa_lds_bytes(n, 256, 16) <= cap)
    assert sel(Ns=ns, E=64, Cn=4, K=16)[:2] == (0, 0) and sel(Ns=ns + 1, E=64, Cn=4, K=16) == (-2, -2, 0)
    for kw in (dict(Ns=0), dict(E=0), dict(Cn=0), dict(K=0), dict(ld=15), dict(V=0)):
        assert sel(**kw)[:2] == (-1, -1), kw
    for name in ("embed", "items", "m", "chosen"):
        assert sel(null=name)[:2] == (-1, -1), name
    for name in ("inner", "loss"):
        assert sel(null=name)[:2] == (-1, 0), name
    for name in ("gm", "gitems"):
        assert sel(null=name)[:2] == (0, -1), name
    assert sel(null="ginner")[:2] == (0, 0) and sel(null="gloss")[:2] == (0, 0) and sel(null="gsel")[:2] == (0, 0)
    assert sel(both_null=True)[:2] == (0, -1)


def test_check_shape_names_the_limit():
    from explicit_tf2_recommendation_amd import ops
    ops.comirec_check_shape(48, 48, 4, 3, T=226, mode="DR")
    ops.comirec_check_shape(48, 48, 4, T=226, mode="SA")
    ops.comirec_check_shape(256, 256, 16, 3, T=9, Ns=33)
    with pytest.raises(NotImplementedError, match="capsule width <= 256"):
        ops.comirec_check_shape(257, 48, 4)
    with pytest.raises(NotImplementedError, match="capsules <= 16"):
        ops.comirec_check_shape(48, 48, 17)
    with pytest.raises(NotImplementedError, match="rounds <= 8"):
        ops.comirec_check_shape(48, 48, 4, 9)
    with pytest.raises(NotImplementedError, match=r"dynamic routing holds one row \(b, k\) in LDS"):
        ops.comirec_check_shape(48, 48, 4, 3, T=658, mode="DR")
    with pytest.raises(NotImplementedError, match="self-attention holds one example in LDS"):
        ops.comirec_check_shape(48, 48, 4, T=243, mode="SA")
    with pytest.raises(NotImplementedError, match="hard attention holds one example in LDS"):
        ops.comirec_check_shape(256, 256, 16, Ns=200)
    with pytest.raises(ValueError):
        ops.comirec_check_shape(48, 48, 0)


def test_constructor_signatures():
    from explicit_tf2_recommendation_amd import layers

    def sig(cls):
        return [(n, p.default, p.kind == p.KEYWORD_ONLY) for n, p in inspect.signature(cls.__init__).parameters.items()
                if n != "self"]

    E = inspect.Parameter.empty
    assert sig(layers.ComiRecDynamicRoutingLayer) == [
        ("capsules_num", E, False), ("capsules_dim", E, False), ("routing_rounds", 3, False),
        ("seq_length", None, True), ("embedding_dims", None, True)]
    assert sig(layers.ComiRecSelfAttentiveLayer) == [
        ("capsules_num", E, False), ("capsules_dim", E, False), ("add_pos_emb", True, False),
        ("seq_length", None, True), ("embedding_dims", None, True)]
    assert sig(layers.ComiRecLayer) == [
        ("item_categorical_features", ["label_goods_ids", "label_shop_ids", "label_cate_ids"], False),
        ("behavior_series_features", ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"], False),
        ("feature_dims", 160000, False), ("embedding_dims", 16, False), ("activation", "ReLU", False),
        ("padding_index", 0, False), ("capsules_num", 4, False), ("mode", "DR", False), ("routing_rounds", 3, False),
        ("add_pos_emb", True, False), ("negative_sample_type", "manual", False),
        ("seq_length", None, True), ("reference_mask", True, True)]


@pytest.mark.parametrize("mode", ["DR", "SA"])
def test_state_dict_names_and_shapes(mode):
    from explicit_tf2_recommendation_amd import layers
    lay = layers.ComiRecLayer(feature_dims=CR.LAYER_V, seq_length=6, mode=mode)
    sd = lay.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == CR.STATE_SHAPES[mode](6)
    assert {k: v.shape for k, v in CR.layer_state(1, 6, mode).items()} == CR.STATE_SHAPES[mode](6)
    assert sorted(k for k, _ in lay.named_buffers()) == (list(CR.BUFFERS) if mode == "DR" else [])
    if mode == "DR":
        assert abs(float(sd["interest_extractor.W"].std()) - 0.05) < 0.005 and not sd["interest_extractor.B"].any()
        assert lay.interest_extractor.routing_rounds == 3
    else:
        assert abs(float(sd["interest_extractor.W1"].std()) - np.sqrt(2 / 96)) < 0.03
    lazy = layers.ComiRecLayer(feature_dims=100, mode=mode)                            # built by the first call
    assert sorted(lazy.state_dict()) == ["embed.embeddings"]
    ext = layers.ComiRecDynamicRoutingLayer(4, 48, seq_length=50, embedding_dims=32)
    assert tuple(ext.W.shape) == (4, 50, 32, 48) and tuple(ext.B.shape) == (4, 50)
    ext = layers.ComiRecSelfAttentiveLayer(4, 48, embedding_dims=32)
    assert tuple(ext.W1.shape) == (32, 48) and tuple(ext.W2.shape) == (4, 48)


def test_error_paths_of_the_layer():
    from explicit_tf2_recommendation_amd import layers
    with pytest.raises(ValueError, match=r"mode must be in \('DR','SA'\)"):
        layers.ComiRecLayer(feature_dims=10, mode="XX")
    with pytest.raises(ValueError, match=r"negative_sample_type must be in \('auto','manual'\)"):
        layers.ComiRecLayer(feature_dims=10, negative_sample_type="none")
    with pytest.raises(NotImplementedError, match="sampled_softmax_loss"):
        layers.ComiRecLayer(feature_dims=10, negative_sample_type="auto")
    with pytest.raises(AssertionError):
        layers.ComiRecLayer(item_categorical_features=["a"], feature_dims=10)
    with pytest.raises(NotImplementedError, match="capsule width <= 256"):
        layers.ComiRecLayer(feature_dims=10, embedding_dims=128)
    with pytest.raises(NotImplementedError, match="in LDS"):
        layers.ComiRecLayer(feature_dims=10, seq_length=700)
    assert layers.ComiRecLayer(feature_dims=10).reference_mask is True
    assert not hasattr(layers.ComiRecLayer, "greedy_search_inference")                 # serving code: out of scope


@pytest.mark.parametrize("case", CR.SELECT_CASES, ids=ids)
def test_near_tie_examples_are_at_most_a_tenth_of_a_body_case(case):
    c = CR.select_case(*case)
    ref = CR.select_numpy(c["table"], c["items"], c["m"])
    near = ref["gap"] < CR.GAP_EPS_BODY
    print("near-tie examples: %d of %d" % (near.sum(), len(near)))
    assert np.array_equal(near, c["near"]) and near.mean() <= 0.10
    for k in ("ginner", "gloss", "gsel"):
        assert not np.any(c[k][near])


@pytest.mark.parametrize("reference_mask", [True, False], ids=["literal", "paper"])
@pytest.mark.parametrize("mode", ["DR", "SA"])
@pytest.mark.parametrize("T", CR.LAYER_TS)
def test_layer_seed_has_no_near_tie_example(T, mode, reference_mask):
    seed = CR.layer_seed(T, mode, reference_mask)
    res = CR.layer_torch(CR.layer_state(seed, T, mode), CR.layer_inputs(seed, CR.LAYER_B, T, mode), torch.float64, mode,
                         reference_mask)
    print("seed %d, smallest top-two gap %.2e" % (seed, res["gap"].min()))
    assert seed == next(s for s in (1, 2, 3, 4, 5, 6, 7, 8) if not (CR.layer_torch(
        CR.layer_state(s, T, mode), CR.layer_inputs(s, CR.LAYER_B, T, mode), torch.float64, mode, reference_mask)["gap"]
        < CR.GAP_EPS_LAYER).any())
    assert not (res["gap"] < CR.GAP_EPS_LAYER).any()
    assert all(np.all(np.isfinite(res[k])) for k in ("output", "loss", "capsules"))
    assert tuple(res["output"].shape) == (CR.LAYER_B, CR.LAYER_NS, CR.LAYER_D)
