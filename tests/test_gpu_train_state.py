"""GPU tests of the STATE a compiled train loop leaves behind (engine="auto": engine.GraphedTrainStep for every layer
but DeepFM, engine.DeepFMFusedStep for DeepFM) against the eager autograd path and the float64 oracle: not only losses
and ``named_parameters()`` but every entry of ``state_dict()`` -- module buffers such as BatchNormalization's moving
statistics included -- and the table rows whose Keras-Adam sweeps the fused step evaluates lazily.

Tolerances, all taken from elsewhere in the suite:
  exact   graphed vs eager: the same kernels in the same order (tests/test_gpu_manager.py,
          test_compiled_train_loop_other_layers_replay_one_graph, and the per-family *_graphed_like_eager tests)
  1e-6    moving statistics against the float64 oracle (tests/test_gpu_f4.py, test_nfm_layer)
  2e-5    loss, and 5e-5 per parameter, of the fused DeepFM step against eager Keras Adam after 6 iterations at lr 0.01
          (tests/test_gpu_manager.py, test_compiled_train_loop_fresh_batches_neither_recapture_nor_grow)
"""
import gc
import random

import numpy as np
import pytest
import torch

from oracle import layers_np as L

pytestmark = pytest.mark.gpu

NAMES = ["user_tag1", "user_tag2", "item_tag1", "item_tag2", "item_tag3"]     # 2.FM/ModelManager.py:13
CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
USER = ["uid", "utag1", "utag2", "utag3", "utag4"]
ITEM = ["i_goods_id", "i_shop_id", "i_cate_id"]
SER = ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]
B_GRAPHED = 200                                               # not a multiple of a wave, a workgroup or a GEMM tile


@pytest.fixture(autouse=True)
def collect_dropped_managers():
    """A ModelManager is part of a reference cycle (the closures it hands to its step), so its hipGraphs live until the
    cyclic collector runs; every test here drops several, and they are collected here, not in the middle of whatever
    a later test captures."""
    yield
    gc.collect()


def full_state(module):
    """A copy of every entry of state_dict(): parameters AND buffers."""
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def assert_same_state(a, b, where):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb), where
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (where, k)


def family(name, engine="auto", act=None):
    """(manager, batch generator) of one layer family at a small shape."""
    from explicit_tf2_recommendation_amd import data, layers
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    B = B_GRAPHED
    layers.set_init_seed(51)                                 # the initial parameters must not depend on the test order
    torch.manual_seed(51)
    if name in ("ffm_ranking", "pnn_ranking"):
        V = 3000
        mm = ModelManager(feature_names=NAMES, data_info=data.data_info(V, len(NAMES)), embedding_dims=8, lr=0.01,
                          batch=B, layer=name, engine=engine)
        return mm, data.SyntheticGenerator(NAMES, V, dist="zipf", seed=11)
    if name == "din_layer":
        V = 5000
        params = {"user_and_context_categorical_features": USER, "item_categorical_features": ITEM,
                  "behavior_series_features": SER}
        if act is not None:
            params["activation"] = act
        mm = ModelManager(feature_names=USER + ITEM, behavior_series_features=SER, data_info=data.data_info(V, 11),
                          embedding_dims=8, lr=0.01, batch=B, layer="din_layer", model_params=params,
                          regularization_factor=0.01, engine=engine)      # the L2 term on the used rows is in the graph
        return mm, data.SyntheticGenerator(USER + ITEM, V, series=SER, seq_len=11, dist="zipf", seed=12)
    V = 5000
    params = {"NFM": {}, "CCPM": {"units": [32, 8]}, "FGCNN": {"units": [32, 8]}, "dcn_vec": {"type": "vec"},
              "dcn_matrix": {"type": "matrix"}}[name]
    layer = "dcn_ranking" if name.startswith("dcn") else name
    mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(V, len(CAT)),
                      embedding_dims=16, lr=0.01, batch=B, layer=layer, model_params=params, engine=engine)
    return mm, data.SyntheticGenerator(CAT, V, continuous=CONT, dist="zipf", seed=13)


def train_auto_like_eager(name, act=None, need_buffers=False):
    """Eager and auto managers from one state, 4 train_loop calls on 4 different batches (Adam applied between the
    replays): after every call the losses are the same number and the full state is bit-identical."""
    a, gen = family(name, "eager", act)
    b, _ = family(name, "auto", act)
    b.model.load_state_dict(a.model.state_dict())
    if need_buffers:                                         # the comparison below must reach the moving statistics
        assert any(k.endswith("moving_mean") for k in a.model.state_dict())
        assert a.model.training and b.model.training
    assert_same_state(a.model, b.model, (name, "start"))
    for it in range(4):
        batch = gen.batch(B_GRAPHED)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert b._eng[0] == "graphed"
        assert np.isfinite(la.item()) and la.item() == lb.item(), (name, it, la.item(), lb.item())
        assert_same_state(a.model, b.model, (name, it))      # exact: same kernels in the same order
    return a, b


# ------------------------------------------------------------------------------------------------
# A. building a GraphedTrainStep changes nothing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NFM", "CCPM", "FGCNN", "mlp_bn"])
def test_building_a_graphed_step_leaves_the_full_state_alone(name):
    """The constructor runs warm-up forward+backward passes in training mode before it captures; whatever a module
    updates in place on a forward (BatchNormalization's moving mean / variance) must be as it was afterwards."""
    from explicit_tf2_recommendation_amd import data, engine, layers, functional as Fn
    if name == "mlp_bn":
        class Wrapped(layers.Layer):                         # dict in, dict out, probabilities for KerasBCE
            def __init__(self):
                super().__init__()
                self.mlp = layers.MLPLayer(units=[16, 4], is_batch_norm=True, input_dim=24)

            def forward(self, inputs):
                return {"output": Fn.Sigmoid.apply(self.mlp(inputs["x"]))}

        layers.set_init_seed(3)
        layer = Wrapped().cuda()
        r = np.random.default_rng(3)
        batch = data.to_device({"x": (r.normal(size=(B_GRAPHED, 24)) * 2 + 1).astype(np.float32),
                                "label": (r.random((B_GRAPHED, 1)) < 0.3).astype(np.float32)})
    else:
        mm, gen = family(name, "eager")
        layer, batch = mm.model, data.to_device(gen.batch(B_GRAPHED))
    assert layer.training
    before = full_state(layer)
    assert sum(k.endswith("moving_variance") for k in before) >= 1
    step = engine.GraphedTrainStep(layer, batch)
    after = layer.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    # and the step is live: one replay folds the batch into the moving statistics exactly once
    step(batch)
    torch.cuda.synchronize()
    moved = [k for k in before if k.endswith("moving_mean") and not torch.equal(layer.state_dict()[k], before[k])]
    assert moved


# ------------------------------------------------------------------------------------------------
# B. moving statistics after training equal eager's and the oracle's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["NFM", "CCPM", "FGCNN"])
def test_batchnorm_families_graphed_leave_eagers_full_state(name):
    train_auto_like_eager(name, need_buffers=True)


def test_nfm_first_graphed_step_folds_the_batch_once_like_the_float64_oracle():
    """After the first train_loop of a fresh NFM layer, bn_layer's moving statistics are ONE fold (momentum 0.99) of the
    batch statistics of [bi_interaction | X_cont] into (0, 1): the recipe and the 1e-6 of tests/test_gpu_f4.py's
    test_nfm_layer.  The table keeps its default U(-0.05, 0.05) init ON PURPOSE: the interaction columns then have a
    batch variance of ~1e-6, so one fold leaves their moving variance at ~0.99 and four folds (one per warm-up pass of
    the graphed step plus the replay) at ~0.961 -- 3e-2 apart, against a bound of 1e-6."""
    mm, gen = family("NFM", "auto")
    bn = mm.model.bn_layer
    assert torch.equal(bn.moving_mean, torch.zeros_like(bn.moving_mean))
    assert torch.equal(bn.moving_variance, torch.ones_like(bn.moving_variance))
    table = mm.model.embed.embeddings.detach().cpu().numpy().copy()
    n = bn.moving_mean.numel()
    batch = gen.batch(B_GRAPHED)
    mm.train_loop(dict(batch))
    assert mm._eng[0] == "graphed"
    X = L.index_assemble(batch, CAT)
    XC = np.concatenate([batch[c] for c in CONT], axis=1)
    comb = np.concatenate([L.bi_interaction_forward(table, X, np.float64), XC], axis=1)
    assert comb[:, :table.shape[1]].var(axis=0).max() < 1e-4          # the property the docstring relies on
    _, nm, nv = L.batchnorm_forward(comb, np.ones(n), np.zeros(n), np.zeros(n), np.ones(n), True, dt=np.float64)
    got_m, got_v = bn.moving_mean.cpu().numpy().astype(np.float64), bn.moving_variance.cpu().numpy().astype(np.float64)
    print("NFM first fold: max |moving_mean - oracle| %.3e, max |moving_variance - oracle| %.3e"
          % (np.abs(got_m - nm).max(), np.abs(got_v - nv).max()))
    assert np.abs(got_m - nm).max() <= 1e-6 * max(1.0, np.abs(nm).max())
    assert np.abs(got_v - nv).max() <= 1e-6 * max(1.0, np.abs(nv).max())


# ------------------------------------------------------------------------------------------------
# C. families that had no manager-level auto-vs-eager comparison
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,act", [("ffm_ranking", None), ("pnn_ranking", None), ("dcn_vec", None),
                                      ("dcn_matrix", None), ("din_layer", None), ("din_layer", "PReLU")])
def test_other_families_graphed_leave_eagers_full_state(name, act):
    """DIN: the layer's default activation (Dice) and the other one its constructor offers (PReLU)."""
    from explicit_tf2_recommendation_amd import layers
    a, _ = train_auto_like_eager(name, act)
    if name == "din_layer":
        kinds = {type(m) for m in a.model.modules() if isinstance(m, (layers.Dice, layers.PReLU))}
        assert kinds == {layers.PReLU if act == "PReLU" else layers.Dice}


# ------------------------------------------------------------------------------------------------
# D, E. the fused DeepFM step: what train_step / run(mode="train") leave behind
# ------------------------------------------------------------------------------------------------
def deepfm_manager(engine, **kw):
    from explicit_tf2_recommendation_amd import data, layers
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    V, B = 3000, 256
    layers.set_init_seed(52)
    torch.manual_seed(52)
    mm = ModelManager(feature_names=NAMES, data_info=data.data_info(V, len(NAMES)), embedding_dims=16, lr=0.01, batch=B,
                      layer="deepfm_ranking", engine=engine, steps_per_call=2, **kw)     # default mlp_dims: fused step
    return mm


def deepfm_batches(n, seed):
    from explicit_tf2_recommendation_amd import data
    gen = data.SyntheticGenerator(NAMES, 3000, dist="zipf", seed=seed)
    return [gen.batch(256) for _ in range(n)]


def test_train_step_alone_leaves_current_parameters():
    """train_step with no eval_step and no sync_parameters() after it: the parameters it leaves are Keras Adam's (the
    eager manager's), although the compiled step lets rows outside a batch skip the dense sweeps.  6 batches with
    steps_per_call=2: the first goes through train_loop (builds the engine), the other 5 through _train_chunks as chunks
    of 2, 2 and 1 -- a tail chunk.  Bounds: 2e-5 on the loss, 5e-5 per parameter, the suite's own for 6 fused-vs-eager
    iterations at lr 0.01 (tests/test_gpu_manager.py,
    test_compiled_train_loop_fresh_batches_neither_recapture_nor_grow)."""
    ds = deepfm_batches(6, seed=21)
    eager, auto, lazy = deepfm_manager("eager"), deepfm_manager("auto"), deepfm_manager("auto")
    auto.model.load_state_dict(eager.model.state_dict())
    lazy.model.load_state_dict(eager.model.state_dict())
    order, eager_loop = [], eager.train_loop                 # the batches in the order train_step itself fed them

    def recording_loop(inputs, next_inputs=None):
        order.append(inputs)
        return eager_loop(inputs, next_inputs)

    eager.train_loop = recording_loop
    random.seed(7)
    res_e = eager.train_step(ds)
    eager.train_loop = eager_loop
    assert sorted(id(b["label"]) for b in order) == sorted(id(b["label"]) for b in ds)      # each batch once
    random.seed(7)
    res_a = auto.train_step(ds)
    assert auto._eng[0] == "fused" and auto._eng[1].t == 6
    print("train_step: eager loss %.8f, auto loss %.8f" % (res_e["loss"], res_a["loss"]))
    assert abs(res_e["loss"] - res_a["loss"]) <= 2e-5
    pe, pa = dict(eager.model.named_parameters()), dict(auto.model.named_parameters())
    assert list(pe) == list(pa)
    for k in pe:
        err = (pe[k] - pa[k]).abs().max().item()
        print("train_step: max |eager - auto| of %s = %.3e" % (k, err))
        assert err <= 5e-5, k
    # not vacuous: the same 6 batches in the same order through train_loop alone leave stale rows, until they are synced
    for b in order:
        lazy.train_loop(dict(b))
    assert lazy._eng[0] == "fused" and lazy._eng[1].t == 6
    te, tl = eager.model.embed.embeddings.detach(), lazy.model.embed.embeddings.detach()
    row_err = (te - tl).abs().max(dim=1).values
    assert int((row_err > 5e-5).sum().item()) >= 1           # rows touched in the first iterations and not afterwards
    lazy.sync_parameters()
    for k, p in lazy.model.named_parameters():
        assert (pe[k] - p).abs().max().item() <= 5e-5, k
    auto._eng[1].check_flags()
    lazy._eng[1].check_flags()


def test_state_dict_after_run_train_is_the_trained_model():
    """run(mode="train"), 2 epochs of 4 batches (the second epoch continues from a flushed state, all of it through
    _train_chunks): model.state_dict() taken right afterwards, loaded into a fresh eager manager, evaluates to exactly
    the auto manager's own eval_step loss (current tables, the same weights through the same forward) and within 2e-5
    (tests/test_gpu_manager.py's bound for the fused step against eager Keras Adam) of the eager-trained manager's."""
    ds, held = deepfm_batches(4, seed=22), deepfm_batches(2, seed=23)
    eager, auto, fresh = deepfm_manager("eager", epochs=2), deepfm_manager("auto", epochs=2), deepfm_manager("eager")
    auto.model.load_state_dict(eager.model.state_dict())
    random.seed(9)
    eager.run(ds, mode="train")
    random.seed(9)
    auto.run(ds, mode="train")
    assert auto._eng[0] == "fused" and auto._eng[1].t == 8
    fresh.model.load_state_dict(auto.model.state_dict())     # BEFORE auto's eval_step, which syncs the tables itself
    loss_fresh = fresh.eval_step(held)["loss"]
    loss_auto = auto.eval_step(held)["loss"]
    loss_eager = eager.eval_step(held)["loss"]
    print("eval loss: from auto's state dict %.8f, auto %.8f, eager-trained %.8f" % (loss_fresh, loss_auto, loss_eager))
    assert loss_fresh == loss_auto
    assert abs(loss_fresh - loss_eager) <= 2e-5
    auto._eng[1].check_flags()
