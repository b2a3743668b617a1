"""DIEN without a GPU: the hand-derived backward through time of tests/dien_ref.py against autograd in fp64, the
unmasked GRU against torch.nn.GRU with permuted gates, the carry semantics of the mask, the consequence of the
reference's mask convention (an evolved interest that is exactly zero), rows that select nothing, the auxiliary loss at
T = 1, stage 'inference', the layer's constructor and state dict in the three modes, the composed sub-layers on the CPU
against the transcription, and the ABI: names, signatures, the LDS formula and the error codes in the documented order."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import dien_ref as DR

ids = lambda c: "x".join(map(str, c))
HOST_CASES = [c for c in DR.CASES if c != DR.LARGEST]


@pytest.mark.parametrize("case", HOST_CASES, ids=ids)
def test_hand_derived_backward_equals_autograd_in_fp64(case):
    c = DR.inputs(case)
    pairs = [("extractor", DR.extractor_numpy(c, c["dgru_output"], c["gaux"]),
              DR.extractor_torch(c, torch.float64, c["dgru_output"], c["gaux"]), DR.GRU_OUT + DR.GRU_GRADS)]
    pairs.append(("aux alone", DR.extractor_numpy(c, None, c["gaux"]), DR.extractor_torch(c, torch.float64, None, c["gaux"]),
                  DR.GRU_OUT + DR.GRU_GRADS))
    for kind in DR.KINDS:
        for mv in (0, 1):
            pairs.append(("%s mask_valid=%d" % (kind, mv), DR.evolution_numpy(c, kind, mv, c["dh_final"]),
                          DR.evolution_torch(c, torch.float64, kind, mv, c["dh_final"]), DR.EVO_OUT + DR.EVO_GRADS))
    for what, ref, t64, names in pairs:
        for name in names:
            assert ref[name].shape == t64[name].shape, (what, name)
            assert DR.rel_err(ref[name], t64[name]) <= 1e-10, (what, name, DR.rel_err(ref[name], t64[name]))
            if not np.any(t64[name]):
                assert not np.any(ref[name]), (what, name)
            assert np.isfinite(ref[name]).all(), (what, name)


def test_the_generator_mixes_every_mask_pattern_and_keeps_exp_finite():
    for case in DR.CASES:
        c = DR.inputs(case)
        B, T = case[:2]
        valid = c["valid"]
        assert np.abs(np.einsum("bth,bh->bt", c["g"], c["q"])).max() < 10.0
        if T > 1:
            for b in range(min(B, 5)):
                kind, v = DR.pattern_of(b), valid[b]
                n = int(v.sum())
                assert {"holes": 0 < n < T, "left": 0 < n < T and not v[0] and v[-1] and v[T - n:].all(),
                        "all": n == 0, "right": 0 < n < T and v[0] and not v[-1] and v[:n].all(), "none": n == T}[kind]
        assert (c["series"][:, :, 1:] != 0).all()                            # the first feature alone decides
    assert len(np.unique(DR.inputs(DR.MASKED)["series"])) < DR.inputs(DR.MASKED)["series"].size


def test_unmasked_gru_equals_torch_nn_gru_with_permuted_gates():
    """Keras orders the gates z, r, h and torch r, z, n; both bias rows are used (reset_after=True)."""
    B, T, H = 4, 7, 12
    rng = np.random.default_rng(5)
    x, K, U, b = (rng.standard_normal(s) * 0.5 for s in ((B, T, H), (H, 3 * H), (H, 3 * H), (2, 3 * H)))
    hs, _ = DR.cell_forward(x, np.ones((B, T), bool), K, U, b[0], b[1], "GRU")
    perm = np.concatenate([np.arange(H, 2 * H), np.arange(0, H), np.arange(2 * H, 3 * H)])
    gru = torch.nn.GRU(H, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(torch.tensor(K[:, perm].T))
        gru.weight_hh_l0.copy_(torch.tensor(U[:, perm].T))
        gru.bias_ih_l0.copy_(torch.tensor(b[0][perm]))
        gru.bias_hh_l0.copy_(torch.tensor(b[1][perm]))
        want = gru(torch.tensor(x))[0].numpy()
    assert DR.rel_err(hs, want) <= 1e-14
    t64 = DR.keras_gru_torch(torch.tensor(x), torch.ones(B, T, dtype=torch.bool), *(torch.tensor(v) for v in (K, U, b)))
    assert DR.rel_err(t64.numpy(), want) <= 1e-14


def test_a_masked_step_carries_the_state():
    c = DR.inputs(DR.MASKED)
    hs = DR.extractor_numpy(c)["gru_output"]
    valid = c["valid"]
    T = valid.shape[1]
    seen = set()
    for b in range(5):
        kind, v = DR.pattern_of(b), valid[b]
        seen.add(kind)
        for t in range(T):
            if not v[t]:
                prev = hs[b, t - 1] if t > 0 else np.zeros_like(hs[b, 0])
                assert np.array_equal(hs[b, t], prev), (kind, t)             # the carried state IS the output
            else:
                assert np.any(hs[b, t] != (hs[b, t - 1] if t > 0 else 0)), (kind, t)
        if kind == "all":
            assert not hs[b].any()
        if kind == "left":
            assert not hs[b, :int((~v).sum())].any() and hs[b, -1].any()     # zero before the first valid step
    assert seen == set(DR.PATTERNS)
    # the carried rows equal the GRU run on the valid steps alone
    b = 0
    v = valid[b]
    only = {k: (c[k][b:b + 1][:, v] if k in ("x", "xn", "valid") else c[k]) for k in
            ("x", "xn", "valid", "kernel", "recurrent_kernel", "bias")}
    assert DR.rel_err(DR.extractor_numpy(only, negatives=False)["gru_output"][0, -1], hs[b, np.nonzero(v)[0][-1]]) <= 1e-14


@pytest.mark.parametrize("kind", ("AGRU", "AUGRU"))
def test_reference_mask_mode_gives_an_exactly_zero_evolved_interest(kind):
    """As written only PADDED positions score, so a valid step has a = 0 and a padded one is skipped."""
    c = DR.inputs(DR.MASKED)
    for r in (DR.evolution_numpy(c, kind, 0, c["dh_final"]), DR.evolution_torch(c, torch.float32, kind, 0, c["dh_final"])):
        assert not np.any(r["h_final"])
        for name in ("dq", "dWx", "dUh", "dbx"):                               # dq carries dW and dX_item
            assert not np.any(r[name]), name
        assert not np.any(r["dgru_output"])
        assert np.any(r["scores"])
    r = DR.evolution_numpy(c, kind, 1, c["dh_final"])
    for name in ("h_final", "dgru_output", "dq", "dWx", "dUh", "dbx"):
        assert np.any(r[name]), name
    assert np.any(DR.evolution_numpy(c, "AIGRU", 0, c["dh_final"])["h_final"])  # the biases still move a Keras GRU


def test_a_row_that_selects_nothing_scores_zeros_and_no_gradient_is_nan():
    c = DR.inputs(DR.MASKED)
    valid = c["valid"]
    rows = {0: np.nonzero(valid.all(1))[0], 1: np.nonzero(~valid.any(1))[0]}   # nothing padded / nothing valid
    for kind in DR.KINDS:
        for mv in (0, 1):
            assert len(rows[mv]) > 0
            for r in (DR.evolution_numpy(c, kind, mv, c["dh_final"]),
                      DR.evolution_torch(c, torch.float32, kind, mv, c["dh_final"])):
                assert not r["scores"][rows[mv]].any()
                assert all(np.isfinite(v).all() for v in r.values())
                assert not r["dq"][rows[mv]].any()


def test_auxiliary_loss_is_zero_at_t_1_and_keeps_the_double_sigmoid():
    c = DR.inputs((1, 1, 1, 1))
    assert float(DR.extractor_numpy(c, None, c["gaux"])["aux"][0]) == 0.0
    assert float(DR.extractor_torch(c, torch.float64, None, c["gaux"])["aux"][0]) == 0.0
    c = DR.inputs(DR.MASKED)
    x, xn, valid = c["x"], c["xn"], c["valid"]
    hs = DR.extractor_numpy(c)["gru_output"]
    want = 0.0
    for b in range(x.shape[0]):
        for t in range(1, x.shape[1]):
            if valid[b, t]:
                p, n = DR.sigmoid(x[b, t - 1] @ hs[b, t]), DR.sigmoid(x[b, t - 1] @ xn[b, t])
                want += np.log1p(np.exp(-p)) + n + np.log1p(np.exp(-n))      # p, n in (0, 1) are fed as LOGITS
    got = float(DR.extractor_numpy(c)["aux"][0])
    assert abs(got - want) <= 1e-10 * want and want > 0


# ---- the layer -----------------------------------------------------------------------------------------------------------
REFERENCE_SIGNATURE = [
    ("user_and_context_categorical_features", ["uid", "utag1", "utag2", "utag3", "utag4"]),
    ("item_categorical_features", ["i_goods_id", "i_shop_id", "i_cate_id"]),
    ("behavior_series_features", ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]),
    ("negative_sample_features", ["negative_goods_ids", "negative_shop_ids", "negative_cate_ids"]),
    ("feature_dims", 160000), ("embedding_dims", 16), ("activation", "Dice"), ("padding_index", 0), ("mode", "AUGRU"),
    ("stage", "train")]


def test_constructor_signature_and_assertions_are_the_reference_s():
    from explicit_tf2_recommendation_amd import layers
    params = inspect.signature(layers.DIENLayer.__init__).parameters
    got = [(n, q.default) for n, q in list(params.items())[1:]]
    assert got == REFERENCE_SIGNATURE + [("mask_mode", "reference"), ("fused", True)]
    assert list(inspect.signature(layers.DienActivationLayer.__init__).parameters)[1:3] == ["embedding_dims1",
                                                                                           "embedding_dims2"]
    for cls in (layers.CustomGRUCell, layers.DienGRU):
        assert list(inspect.signature(cls.__init__).parameters)[1:3] == ["units", "mode"]
    with pytest.raises(AssertionError):
        layers.DIENLayer(item_categorical_features=["a", "b"], behavior_series_features=["x", "y"],
                         negative_sample_features=["n"], feature_dims=10)
    with pytest.raises(AssertionError):
        layers.DIENLayer(feature_dims=10, mode="GRU")
    with pytest.raises(ValueError):
        layers.DIENLayer(feature_dims=10, mask_mode="padded")
    with pytest.raises(NotImplementedError):
        layers.DIENLayer(feature_dims=10, embedding_dims=43)                   # 3 x 43 = 129 > 128
    lay = layers.DIENLayer(feature_dims=10)
    assert lay.stage == "train" and lay.mode == "AUGRU" and lay.mask_mode == "reference" and lay.fused
    lay.set_stage("inference")
    assert lay.stage == "inference"
    with pytest.raises(AssertionError):
        lay.set_stage("valid")


@pytest.mark.parametrize("kind", DR.KINDS)
def test_state_dict_names_shapes_and_initialisation(kind):
    from explicit_tf2_recommendation_amd import layers
    lay = layers.DIENLayer(feature_dims=DR.LAYER_V, mode=kind, activation="PReLU")
    sd = lay.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == DR.state_shapes(kind)
    assert not any("gru_cell.gru_cell" in k for k in sd)                       # the never-built inner GRUCell owns nothing
    H = DR.LAYER_H
    for pre in ("gru.",) + (("dien_gru.gru.",) if kind == "AIGRU" else ()):
        lim = np.sqrt(6.0 / (H + 3 * H))
        k = sd[pre + "kernel"].double()
        assert 0.9 * lim < float(k.abs().max()) <= lim                          # Glorot uniform
        rk = sd[pre + "recurrent_kernel"].double()
        assert float((rk @ rk.t() - torch.eye(H, dtype=torch.float64)).abs().max()) < 1e-5   # orthogonal rows
        assert not sd[pre + "bias"].any()
    W = sd["dien_activation_layer.W"].double()
    assert 0.04 < float(W.std()) < 0.06 and abs(float(W.mean())) < 0.01        # normal(0, 0.05)
    if kind != "AIGRU":
        lim = np.sqrt(6.0 / (2 * H))
        for n in DR.CELL[kind]:
            v = sd["dien_gru.gru_cell." + n]
            assert (not v.any()) if n.startswith("b") else 0.9 * lim < float(v.abs().max()) <= lim
    assert set(layers.DIENLayer(feature_dims=10, mode=kind).state_dict()) >= set(k for k in sd if "alpha" not in k)


def _cpu_layer(kind, mask_mode, stage="train", seed=3, T=6):
    from explicit_tf2_recommendation_amd import layers
    lay = layers.DIENLayer(feature_dims=DR.LAYER_V, mode=kind, activation="PReLU", mask_mode=mask_mode, stage=stage)
    sd = DR.layer_state(seed, kind)
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in sd.items()})
    rng = np.random.default_rng(seed)
    B, H = DR.LAYER_B, DR.LAYER_H
    series = DR.mask_series(rng, rng.integers(1, 50, (B, T, 3)))
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    x, xn, xi = (t(rng.standard_normal(s) * 0.3) for s in ((B, T, H), (B, T, H), (B, H)))
    return lay, x.requires_grad_(), xn, xi, torch.tensor(series[:, :, 0] != 0)


@pytest.mark.parametrize("kind", DR.KINDS)
@pytest.mark.parametrize("mask_mode", ("reference", "valid"))
def test_composed_layer_body_on_the_cpu_equals_the_transcription(kind, mask_mode):
    lay, x, xn, xi, valid = _cpu_layer(kind, mask_mode)
    evolved, aux = lay.body(x, xn, xi, valid)
    p = dict(lay.named_parameters())
    want, want_aux = DR.body_torch(p, x, xn, xi, valid, kind, 1 if mask_mode == "valid" else 0, "train")
    assert tuple(evolved.shape) == (DR.LAYER_B, DR.LAYER_H) and aux.dim() == 0
    assert DR.rel_err(evolved.detach().numpy(), want.detach().numpy()) <= 1e-5
    assert DR.rel_err(aux.detach().numpy(), want_aux.detach().numpy()) <= 1e-5
    (evolved.sum() + aux).backward()
    cell = [q for n, q in lay.named_parameters() if n.startswith("dien_gru.") or n == "dien_activation_layer.W"]
    if kind != "AIGRU" and mask_mode == "reference":
        assert not evolved.any()
        assert all(q.grad is None or not q.grad.any() for q in cell)           # exactly zero, or not reached at all
    elif mask_mode == "reference":                                             # AIGRU: scaled inputs reach skipped steps only
        dead = [lay.dien_activation_layer.W, lay.dien_gru.gru.kernel]       # ... whose inputs are zero at the valid ones
        assert evolved.any() and all(q.grad is None or not q.grad.any() for q in dead)
        assert all(q.grad is not None and q.grad.any() for q in cell if all(q is not d for d in dead))
    else:
        assert evolved.any() and all(q.grad is not None and q.grad.any() for q in cell)
    assert all(torch.isfinite(q.grad).all() for q in lay.parameters() if q.grad is not None)
    assert torch.isfinite(x.grad).all()


def test_stage_inference_returns_the_number_zero_and_never_reads_the_negatives():
    lay, x, xn, xi, valid = _cpu_layer("AUGRU", "valid", stage="inference")
    evolved, aux = lay.body(x, None, xi, valid)                                # no negative rows exist
    assert aux == 0 and isinstance(aux, int)
    lay.set_stage("train")
    evolved2, aux2 = lay.body(x, xn, xi, valid)
    assert torch.equal(evolved, evolved2) and float(aux2.detach()) > 0


def test_check_shape_names_the_limit():
    from explicit_tf2_recommendation_amd import ops
    with pytest.raises(ValueError, match="positive"):
        ops.dien_check_shape(0)
    with pytest.raises(ValueError):
        ops.dien_check_shape(8, T=0)
    with pytest.raises(NotImplementedError, match="<= 128"):
        ops.dien_check_shape(129)
    ops.dien_check_shape(128, T=100)
    ops.dien_check_shape(128, T=131, mode=ops.DIEN_AUGRU)
    with pytest.raises(NotImplementedError, match="tile of 32 examples"):
        ops.dien_check_shape(128, T=132, mode=ops.DIEN_AUGRU)
    z = torch.zeros
    with pytest.raises(RuntimeError):                                          # no CPU fallback
        ops.dien_gru_fwd(z(4, 12), z(4, 12), z(2, 12), embed=z(5, 4), series=z(1, 2, 1, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        ops.dien_augru_fwd(z(1, 2, 4), z(1, 4), z(1, 2, dtype=torch.int64), ops.DIEN_AUGRU, z(4, 12), z(4, 12), z(12))


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_abi_names_and_signatures():
    from explicit_tf2_recommendation_amd import _lib
    p, i, l, z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    head = [p, l, l, i, i, p, p, p, p, l, i, i, p, p, p, l]
    evo = [p, p, p, l, l, i, i, i, p, p, p, l, i]
    want = {"rec_dien_gru_lds_bytes": (z, [i, i]), "rec_dien_augru_lds_bytes": (z, [i, i, i]),
            "rec_dien_gru_scratch_bytes": (z, [l, i, i, i]), "rec_dien_augru_scratch_bytes": (z, [l, i, i, i]),
            "rec_dien_gru_fwd_f32": (i, head + [p, p, p, p, p, z, p]),
            "rec_dien_gru_bwd_f32": (i, head + [p] * 9 + [p, z, p]),
            "rec_dien_augru_fwd_f32": (i, evo + [p, p, p, p]),
            "rec_dien_augru_bwd_f32": (i, evo + [p] * 8 + [p, z, p])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert hasattr(_lib.lib, name)


def test_lds_formula_and_the_supported_range():
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import lib
    cap = 150 * 1024
    for H in (1, 15, 48, 96, 128):
        assert lib.rec_dien_gru_lds_bytes(1, H) == lib.rec_dien_gru_lds_bytes(10 ** 4, H) == ops.dien_lds_bytes(1, H) <= cap
        for mode in (ops.DIEN_AUGRU, ops.DIEN_AGRU):
            T = 1
            while ops.dien_lds_bytes(T + 1, H, mode) <= cap:
                T += 1
            assert lib.rec_dien_augru_lds_bytes(T, H, mode) == ops.dien_lds_bytes(T, H, mode) <= cap
            assert lib.rec_dien_augru_lds_bytes(T + 1, H, mode) == 0
    assert ops.dien_lds_bytes(131, 128, ops.DIEN_AUGRU) <= cap < ops.dien_lds_bytes(132, 128, ops.DIEN_AUGRU)
    assert ops.dien_lds_bytes(243, 96, ops.DIEN_AUGRU) <= cap < ops.dien_lds_bytes(244, 96, ops.DIEN_AUGRU)
    assert lib.rec_dien_gru_lds_bytes(6, 129) == 0 and lib.rec_dien_augru_lds_bytes(6, 129, 1) == 0
    assert lib.rec_dien_augru_lds_bytes(6, 48, 0) == 0 and lib.rec_dien_augru_lds_bytes(6, 48, 3) == 0
    for B, T, Cn, E in DR.CASES:
        assert lib.rec_dien_gru_scratch_bytes(B, T, Cn * E, 1) > lib.rec_dien_gru_scratch_bytes(B, T, Cn * E, 0) > 0
        assert lib.rec_dien_augru_scratch_bytes(B, T, Cn * E, 1) > lib.rec_dien_augru_scratch_bytes(B, T, Cn * E, 2) > 0
    assert lib.rec_dien_gru_scratch_bytes(4, 6, 129, 1) == 0 and lib.rec_dien_gru_scratch_bytes(-1, 6, 48, 1) == 0
    assert lib.rec_dien_gru_scratch_bytes(4, 6, 48, 2) == 0 and lib.rec_dien_augru_scratch_bytes(4, 6, 48, 0) == 0


def _gru(lib, bwd, **kw):
    d = C.c_void_p(4096)                                                       # never dereferenced
    a = dict(embed=d, ld=16, V=10, E=16, C=3, series=d, negatives=d, x=None, mask_ids=None, B=4, T=6, H=48, kernel=d,
             recurrent_kernel=d, bias=d, pad=0)
    if bwd:
        a.update(dict(gru_output=d, dgru_output=d, dh_final=None, gaux=d, dx=d, dneg=d, dkernel=d, drecurrent_kernel=d,
                      dbias=d, scratch=d, scratch_bytes=1 << 40))
    else:
        a.update(dict(gru_output=d, h_final=None, aux=d, oob=None, scratch=d, scratch_bytes=1 << 40))
    assert set(kw) <= set(a), kw
    a.update(kw)
    return (lib.rec_dien_gru_bwd_f32 if bwd else lib.rec_dien_gru_fwd_f32)(*a.values(), None)


def _evo(lib, bwd, **kw):
    d = C.c_void_p(4096)
    a = dict(gru_output=d, q=d, mask_ids=d, mask_stride=3, B=4, T=6, H=48, mode=1, Wx=d, Uh=d, bx=d, pad=0, mask_valid=0)
    if bwd:
        a.update(dict(scores=d, states=d, dh_final=d, dgru_output=d, dq=d, dWx=d, dUh=d, dbx=d, scratch=d,
                      scratch_bytes=1 << 40))
    else:
        a.update(dict(scores=d, states=d, h_final=d))
    assert set(kw) <= set(a), kw
    a.update(kw)
    return (lib.rec_dien_augru_bwd_f32 if bwd else lib.rec_dien_augru_fwd_f32)(*a.values(), None)


def test_abi_errors_in_the_documented_order():
    """On a CPU-only load of the library every call returns before any launch."""
    from explicit_tf2_recommendation_amd._lib import lib
    for bwd in (0, 1):
        for f in (_gru, _evo):
            for kw in (dict(T=0), dict(H=0), dict(B=-1), dict(T=0, H=129), dict(H=-5)):
                assert f(lib, bwd, **kw) == -1, (f.__name__, bwd, kw)          # a size below 1 first, whatever else
            for kw in (dict(H=129), dict(B=2 ** 31), dict(H=129, kernel=None) if f is _gru else dict(H=129, Wx=None)):
                assert f(lib, bwd, **kw) == -2, (f.__name__, bwd, kw)          # the limits before the pointers
            assert f(lib, bwd, B=0) == 0
        for kw in (dict(E=0), dict(C=0), dict(ld=15), dict(V=0), dict(series=None), dict(kernel=None),
                   dict(recurrent_kernel=None), dict(bias=None), dict(E=8), dict(x=C.c_void_p(4096)),
                   dict(embed=None), dict(embed=None, negatives=None, x=C.c_void_p(4096))):
            assert _gru(lib, bwd, **kw) == -1, (bwd, kw)
        dense = dict(embed=None, series=None, negatives=None, x=C.c_void_p(4096), mask_ids=C.c_void_p(4096), B=0)
        assert _gru(lib, bwd, **dense) == 0
        for kw in (dict(mode=0), dict(mode=3), dict(mask_valid=2), dict(mask_stride=0), dict(q=None), dict(Wx=None),
                   dict(Uh=None), dict(bx=None), dict(gru_output=None), dict(mask_ids=None), dict(scores=None)):
            assert _evo(lib, bwd, **kw) == -1, (bwd, kw)
    assert _evo(lib, 0, T=244, H=96) == -2 and _evo(lib, 0, T=243, H=96, B=0) == 0     # the evolution's LDS fit
    assert _gru(lib, 0, gru_output=None) == -1 and _gru(lib, 0, aux=None) == -1
    assert _gru(lib, 0, scratch_bytes=0) == -3 and _gru(lib, 0, negatives=None, aux=None, scratch=None, scratch_bytes=0,
                                                        B=0) == 0
    for name in ("gru_output", "dx", "dneg", "dkernel", "drecurrent_kernel", "dbias", "scratch"):
        assert _gru(lib, 1, **{name: None}) == -1, name
    for name in ("states", "dh_final", "dgru_output", "dq", "dWx", "dUh", "dbx", "scratch"):
        assert _evo(lib, 1, **{name: None}) == -1, name
    need = lib.rec_dien_gru_scratch_bytes(4, 6, 48, 1)
    assert _gru(lib, 1, scratch_bytes=need - 17) == -3
    assert _gru(lib, 1, scratch_bytes=need - 17, dx=None) == -1                 # the pointers before the scratch
    need = lib.rec_dien_augru_scratch_bytes(4, 6, 48, 1)
    assert _evo(lib, 1, scratch_bytes=need - 17) == -3
