"""MMOE / ESMM without a GPU: the restatements of tests/mmoe_ref.py against each other (numpy backward against torch
autograd in fp64 and against central differences, the double-softmax and ctcvr variants, the two-task loss identity), the
layers' construction and state-dict names, the shape guard at and one past each limit, the ABI's status codes, the
two-label TFRecord round trip, and the near-kink share of every case of tests/test_gpu_mmoe.py on the fp64 reading."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import mmoe_ref as MR

CAT = ["sdk_type", "remote_host", "device_type", "dtu", "click_goods_num", "buy_click_num", "goods_show_num",
       "goods_click_num", "brand_name"]
CONT = ["click_goods_num_origin", "click_goods_num_square", "click_goods_num_cube"]
ENTRY_POINTS = ["rec_mmoe_workspace_bytes", "rec_mmoe_fwd_f32", "rec_mmoe_bwd_f32"]
SMALL = [(5, 7, 3, 2, 4, 3, 5, 2, 1, 0), (5, 7, 3, 2, 4, 3, 5, 2, 2, 0), (5, 7, 3, 2, 4, 3, 5, 2, 1, 1),
         (5, 7, 3, 2, 4, 3, 5, 2, 2, 1), (4, 6, 1, 2, 3, 2, 4, 3, 1, 0), (4, 6, 2, 1, 3, 2, 4, 3, 2, 0),
         (3, 5, 2, 4, 3, 2, 4, 1, 1, 0)]


def _inputs(case, seed=3):
    B, D, n, T, H1, O, H2, O2, passes, ctcvr = case
    r = np.random.default_rng(seed)
    params = MR.make_body(r, D, n, T, H1, O, H2, O2)
    return params, r.normal(0, 1, (B, D)), r.uniform(-1, 1, (B, T)), passes, ctcvr


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_numpy_backward_equals_torch_autograd_in_fp64(case):
    params, x, dout, passes, ctcvr = _inputs(case)
    ref = MR.body_numpy(x, params, passes, ctcvr, dout)
    out, dx, dparams, saved = MR.body_torch_grads(x, params, passes, ctcvr, dout, torch.float64)
    assert MR.rel_err(out, ref["out"]) < 1e-13 and MR.rel_err(dx, ref["dx"]) < 1e-12
    for name in MR.SAVED:
        assert MR.rel_err(saved[name], ref[name]) < 1e-13, name
    for name, got, want in zip(MR.NAMES, dparams, ref["dparams"]):
        assert got.shape == want.shape and MR.rel_err(got, want) < 1e-12, name


@pytest.mark.parametrize("case", [SMALL[0], SMALL[3]], ids=["mmoe", "esmm"])
def test_numpy_backward_equals_central_differences(case):
    def far_from_kinks(seed):
        params, x, _, passes, ctcvr = _inputs(case, seed)
        return MR.body_numpy(x, params, passes, ctcvr)["pre"].min() < 1e-3

    seed = MR.clean_seed(far_from_kinks)
    params, x, dout, passes, ctcvr = _inputs(case, seed)
    ref = MR.body_numpy(x, params, passes, ctcvr, dout)
    loss = lambda xx, pp: float((MR.body_numpy(xx, pp, passes, ctcvr)["out"] * dout).sum())
    eps = 1e-6
    r = np.random.default_rng(0)
    for k, want in [(-1, ref["dx"])] + list(enumerate(ref["dparams"])):
        base = x if k < 0 else params[k]
        for _ in range(4):                                # four random elements of every tensor
            at = tuple(int(r.integers(0, s)) for s in base.shape)
            hi, lo = base.copy(), base.copy()
            hi[at] += eps
            lo[at] -= eps
            fd = (loss(hi, params) - loss(lo, params)) / (2 * eps) if k < 0 else \
                (loss(x, params[:k] + [hi] + params[k + 1:]) - loss(x, params[:k] + [lo] + params[k + 1:])) / (2 * eps)
            assert abs(fd - want[at]) <= 1e-7 + 1e-6 * abs(want[at]), (k, at, fd, want[at])


def test_variants_differ_as_the_reference_defines_them():
    params, x, _, _, _ = _inputs(SMALL[0])
    one, two = MR.body_numpy(x, params, 1, 0), MR.body_numpy(x, params, 2, 0)
    esmm = MR.body_numpy(x, params, 2, 1)
    B = x.shape[0]
    g1 = one["g"].reshape(B, 2, 3)
    ex = np.exp(g1 - g1.max(-1, keepdims=True))
    assert np.allclose(two["g"].reshape(B, 2, 3), ex / ex.sum(-1, keepdims=True), rtol=1e-14, atol=0)
    assert np.allclose(one["g"].reshape(B, 2, 3).sum(-1), 1) and not np.allclose(one["g"], 1 / 3)
    assert np.array_equal(esmm["out"][:, 0], two["out"][:, 0])
    assert np.array_equal(esmm["out"][:, 1], two["p"][:, 0] * two["p"][:, 1]) and np.array_equal(esmm["p"], two["p"])
    # n = 1: the gate is the constant 1 and takes no gradient
    params, x, dout, _, _ = _inputs(SMALL[4])
    ref = MR.body_numpy(x, params, 1, 0, dout)
    assert np.array_equal(ref["g"], np.ones_like(ref["g"]))
    assert np.count_nonzero(ref["dparams"][4]) == 0 and np.count_nonzero(ref["dparams"][5]) == 0


def test_bce_over_both_columns_is_the_mean_of_the_two_task_losses():
    """4.MMOE/ModelManager.py:179-183: 0.5 BCE(ctr) + 0.5 BCE(cvr), each Keras' mean over the batch, is the mean of the
    element-wise cross-entropy over the [B, 2] outputs."""
    r = np.random.default_rng(5)
    p = r.uniform(0, 1, (257, 2))
    p[0], p[1] = (0.0, 1.0), (1.0, 1e-9)                  # Keras clips to [1e-7, 1 - 1e-7]
    y = (r.random((257, 2)) < 0.3).astype(np.float64)

    def bce(yy, pp):
        pp = np.clip(pp, 1e-7, 1 - 1e-7)
        return -(yy * np.log(pp + 1e-7) + (1 - yy) * np.log(1 - pp + 1e-7))

    both = bce(y, p).mean()
    parts = 0.5 * bce(y[:, 0], p[:, 0]).mean() + 0.5 * bce(y[:, 1], p[:, 1]).mean()
    # an identity in exact arithmetic; in fp64 the two orders of 514 additions differ by at most 2 * 514 roundings
    assert abs(both - parts) <= 2 * 514 * 2.0 ** -53 * abs(parts)


# ---- layers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["MMOELayer", "ESMMLayer"])
def test_layer_signature_and_state_dict_names(name):
    from explicit_tf2_recommendation_amd import layers
    cls = getattr(layers, name)
    sig = inspect.signature(cls.__init__)
    assert list(sig.parameters)[1:] == ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                        "expert_num"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["categorical_features"] == CAT and d["continuous_features"] == CONT
    assert (d["feature_dims"], d["embedding_dims"], d["expert_num"]) == (160000, 16, 3)
    lay = cls(feature_dims=50, embedding_dims=4, expert_num=2)
    want = {"embedding_layer.embeddings": (50, 4)}
    for i in range(2):
        want.update({"expert_model.%d.kernel_0" % i: (36, 64), "expert_model.%d.bias_0" % i: (64,),
                     "expert_model.%d.kernel_1" % i: (64, 8), "expert_model.%d.bias_1" % i: (8,)})
    for t in MR.TASKS:
        want.update({t + "_gate.kernel_0": (36, 64), t + "_gate.bias_0": (64,), t + "_gate.kernel_1": (64, 2),
                     t + "_gate.bias_1": (2,), t + "_output.0.kernel_0": (16, 64), t + "_output.0.bias_0": (64,),
                     t + "_output.0.kernel_1": (64, 8), t + "_output.0.bias_1": (8,),
                     t + "_output.1.kernel_0": (8, 1), t + "_output.1.bias_0": (1,)})
    assert {k: tuple(v.shape) for k, v in lay.state_dict().items()} == want
    assert (lay.gate_softmax_passes, bool(lay.ctcvr)) == ((2, True) if name == "ESMMLayer" else (1, False))
    # the packed operands are the sub-layers' parameters in the layout of tests/mmoe_ref.py
    packed = [t.detach().numpy() for t in lay.packed_weights()]
    sd = MR.state_dict_of(lay.embedding_layer.embeddings.detach().numpy(), packed)
    assert sd.keys() == want.keys()
    for k, v in lay.state_dict().items():
        assert np.array_equal(np.asarray(sd[k]).reshape(v.shape), v.numpy()), k
    with pytest.raises(NotImplementedError, match="512"):
        cls(categorical_features=["f%d" % i for i in range(33)], feature_dims=50, embedding_dims=16)


def test_model_manager_builds_both_layers_with_two_labels():
    from explicit_tf2_recommendation_amd import data, layers
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    for name, cls in (("mmoe_layer", layers.MMOELayer), ("esmm_layer", layers.ESMMLayer)):
        mm = ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(5000, 9), layer=name,
                          device="cpu")
        assert type(mm.layer) is cls and mm.task_labels == ("ctr", "cvr") and mm.layer.expert_num == 3
        assert mm._metric_result().keys() == {"ctr_auc", "cvr_auc", "loss"}
    mm = ModelManager(feature_names=CAT, data_info=data.data_info(5000, 9), layer="mmoe_layer", device="cpu",
                      label_name=("click", "buy"), model_params={"expert_num": 2})
    assert mm.task_labels == ("click", "buy") and len(mm.layer.expert_model) == 2
    with pytest.raises(ValueError):
        ModelManager(feature_names=CAT, data_info=data.data_info(5000, 9), layer="esmm_layer", device="cpu",
                     label_name=("a", "b", "c"))
    single = ModelManager(data_info=data.data_info(5000, 5), layer="fm_ranking", device="cpu")
    assert single.task_labels is None and single._metric_result().keys() == {"auc", "loss"}


LIMIT_OK = [(512, 3, 2, 64, 8, 64, 8), (144, 4, 4, 64, 8, 64, 8), (144, 2, 2, 128, 8, 64, 8), (144, 3, 2, 64, 8, 128, 8),
            (144, 16, 2, 8, 8, 64, 8), (144, 3, 2, 64, 8, 64, 128), (144, 3, 4, 64, 8, 64, 8), (1, 1, 1, 1, 1, 1, 1),
            (144, 32, 4, 8, 4, 64, 8)]
LIMIT_PAST = [((513, 3, 2, 64, 8, 64, 8), "512"), ((144, 5, 4, 64, 8, 64, 8), "512"), ((144, 1, 2, 129, 8, 64, 8), "128"),
              ((144, 3, 2, 64, 8, 129, 8), "128"), ((144, 17, 2, 8, 8, 64, 8), "128"), ((144, 3, 2, 64, 8, 64, 129), "128"),
              ((144, 3, 5, 64, 8, 64, 8), "4"), ((144, 33, 4, 8, 4, 64, 8), "128")]


def test_check_shape_at_and_one_past_each_limit():
    from explicit_tf2_recommendation_amd import ops
    for shape in LIMIT_OK:
        ops.mmoe_check_shape(*shape)
    for shape, word in LIMIT_PAST:
        with pytest.raises(NotImplementedError, match=word):
            ops.mmoe_check_shape(*shape)
    for k in range(7):
        bad = [144, 3, 2, 64, 8, 64, 8]
        bad[k] = 0
        with pytest.raises(ValueError):
            ops.mmoe_check_shape(*bad)
    t = torch.zeros(2, 4)
    w = [torch.zeros(s) for s in ((4, 9), (9,), (1, 3, 2), (1, 2), (2, 3, 1), (2, 1), (2, 2, 3), (2, 3), (2, 3, 2), (2, 2),
                                  (2, 2), (2,))]
    with pytest.raises(RuntimeError):                     # there is no CPU path
        ops.mmoe_fwd(t, w)
    with pytest.raises(RuntimeError):
        ops.mmoe_bwd(t, w, (t,) * 7, t)


def test_header_declares_the_entry_points_and_adds_no_constant():
    from explicit_tf2_recommendation_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.SIGNATURES["rec_mmoe_workspace_bytes"] == (C.c_size_t, [C.c_int64] + [C.c_int] * 7)
    assert len(_lib.SIGNATURES["rec_mmoe_fwd_f32"][1]) == 13 + 10 + 8 + 1
    assert len(_lib.SIGNATURES["rec_mmoe_bwd_f32"][1]) == 15 + 10 + 13 + 3
    assert not [k for k in list(_lib.LIMITS) + list(_lib.ENUMS) if "MMOE" in k.upper() or "ESMM" in k.upper()]


def test_abi_status_codes_without_a_gpu():
    from explicit_tf2_recommendation_amd._lib import lib
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    ws = lib.rec_mmoe_workspace_bytes
    base = dict(B=4, D=144, n=3, T=2, H1=64, O=8, H2=64, O2=8, passes=1, ctcvr=0)

    def fwd(x=d, out=d, save=(d,) * 7, **kw):
        a = dict(base, **kw)
        return lib.rec_mmoe_fwd_f32(x, *[d] * 12, a["B"], a["D"], a["n"], a["T"], a["H1"], a["O"], a["H2"], a["O2"],
                                    a["passes"], a["ctcvr"], out, *save, None)

    def bwd(x=d, dx=d, g=d, ws_=d, nbytes=1 << 30, **kw):
        a = dict(base, **kw)
        return lib.rec_mmoe_bwd_f32(x, *[d] * 6, *[d] * 3, g, *[d] * 3, d, a["B"], a["D"], a["n"], a["T"], a["H1"], a["O"],
                                    a["H2"], a["O2"], a["passes"], a["ctcvr"], dx, *[d] * 12, ws_, nbytes, None)

    keys = ("D", "n", "T", "H1", "O", "H2", "O2")
    for shape in LIMIT_OK:
        kw = dict(zip(keys, shape))
        assert ws(17, *shape) > 0
        assert fwd(B=0, **kw) == 0 and bwd(B=0, ws_=None, **kw) == 0
    for shape, _ in LIMIT_PAST:
        kw = dict(zip(keys, shape))
        assert ws(17, *shape) == 0
        assert fwd(B=0, **kw) == -2 and fwd(**kw) == -2 and bwd(**kw) == -2
    assert ws(-1, 144, 3, 2, 64, 8, 64, 8) == 0 and ws(4, 0, 3, 2, 64, 8, 64, 8) == 0 and ws(0, 144, 3, 2, 64, 8, 64, 8) > 0
    assert fwd(x=None) == -1 and fwd(out=None) == -1 and bwd(x=None) == -1 and bwd(dx=None) == -1 and bwd(g=None) == -1
    assert fwd(save=(d, None) + (d,) * 5) == -1 and fwd(save=(d,) * 6 + (None,)) == -1     # save buffers given in part
    for k in ("B", "D", "n", "T", "H1", "O", "H2", "O2"):
        assert fwd(**{k: -1}) == -1 and bwd(**{k: -1}) == -1, k
        if k != "B":
            assert fwd(**{k: 0}) == -1 and fwd(B=0, **{k: 0}) == -1, k
    assert fwd(passes=0) == -1 and fwd(passes=3) == -1 and fwd(B=0, passes=3) == -1 and bwd(passes=3) == -1
    assert fwd(ctcvr=2) == -1 and fwd(ctcvr=-1) == -1 and fwd(ctcvr=1, T=1) == -1 and fwd(ctcvr=1, T=3) == -1
    assert fwd(B=0, ctcvr=1, T=2, passes=2) == 0 and bwd(ctcvr=1, T=4) == -1
    assert bwd(ws_=None) == -1 and bwd(nbytes=16) == -3
    # per example 4 (N1 + n O + T n + T H2 + T O2 + T) bytes; the rest does not grow with the batch beyond the slots
    per = 4 * (320 + 24 + 6 + 128 + 16 + 2)
    w1, w2 = ws(8192, 144, 3, 2, 64, 8, 64, 8), ws(16384, 144, 3, 2, 64, 8, 64, 8)
    assert 8192 * per < w1 and 8192 * per <= w2 - w1 < 8192 * (per + per // 32 + 64)


def test_tfrecord_dataset_reads_two_labels(tmp_path):
    from explicit_tf2_recommendation_amd import data, tfrecord
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    r = np.random.default_rng(2)
    rows = [{"ctr": float(r.random() < 0.4), "cvr": float(r.random() < 0.2), "a": int(r.integers(0, 50)),
             "b": int(r.integers(50, 90))} for _ in range(7)]
    w = tfrecord.TFRecordWriter(str(tmp_path / "mmoe-train-1"))
    for row in rows:
        w.write(tfrecord.encode_example(row))
    w.close()
    ds = tfrecord.TFRecordDataset(str(tmp_path), "train", ["a", "b"], ("ctr", "cvr"), batch=3)
    batches = list(ds)
    assert [len(b["a"]) for b in batches] == [3, 3, 1] and batches[0].keys() == {"a", "b", "ctr", "cvr"}
    for k, dt in (("ctr", np.float32), ("cvr", np.float32), ("a", np.int64), ("b", np.int64)):
        got = np.concatenate([b[k] for b in batches])
        assert got.dtype == dt and got.shape == (7, 1) and np.array_equal(got.reshape(-1), [row[k] for row in rows])
    one = list(tfrecord.TFRecordDataset(str(tmp_path), "train", ["a", "b"], "cvr", batch=7))       # a string: as before
    assert one[0].keys() == {"a", "b", "cvr"} and np.array_equal(one[0]["cvr"].reshape(-1), [row["cvr"] for row in rows])
    with pytest.raises(ValueError, match="buy"):
        list(tfrecord.TFRecordDataset(str(tmp_path), "train", ["a", "b"], ("ctr", "buy"), batch=3))
    mm = ModelManager(feature_names=["a", "b"], data_info=data.data_info(90, 2), layer="mmoe_layer", device="cpu", batch=4)
    got = list(mm.init_dataset("train", data_dir=str(tmp_path)))
    assert [len(b["ctr"]) for b in got] == [4, 3] and got[0].keys() == {"a", "b", "ctr", "cvr"}


@pytest.mark.parametrize("case", MR.BODY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_near_kink_share_of_every_gpu_case(case):
    """What tests/test_gpu_mmoe.py relies on, checked on the fp64 reading: at most 10 % of a case's examples have a relu
    pre-activation below PRE_EPS, none in a case under 100 examples, and their dout rows are zero."""
    c = MR.body_case(*case)
    near = c["near"]
    assert np.array_equal(near, c["ref"]["pre"] < MR.PRE_EPS)
    print("near-kink examples: %d of %d (seed %d)" % (near.sum(), len(near), c["seed"]))
    assert near.mean() <= 0.10 and (case[0] >= 100 or not near.any())
    assert np.count_nonzero(c["dout"][near]) == 0 and np.count_nonzero(c["dout"][~near]) > 0
    if case[2] == 1:                                      # one expert: the gate takes no gradient
        assert np.count_nonzero(c["ref"]["dparams"][4]) == 0 and np.count_nonzero(c["ref"]["dparams"][5]) == 0
