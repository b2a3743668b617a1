"""PLE without a GPU: the restatements of tests/ple_ref.py against each other (numpy backward against torch autograd in
fp64 and against central differences), what the reference's PLELayer defines (the softmax twice on task gates and once on
the shared gate, the gated SUM, the last level, one level, which input an expert reads), the layer's signature,
state-dict names and parameter count, the guard at and one past each limit, the ABI's status codes, and the near-kink
share of every case of tests/test_gpu_ple.py on the fp64 reading."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests import ple_ref as PR

CAT = ["sdk_type", "remote_host", "device_type", "dtu", "click_goods_num", "buy_click_num", "goods_show_num",
       "goods_click_num", "brand_name"]
CONT = ["click_goods_num_origin", "click_goods_num_square", "click_goods_num_cube"]
ENTRY_POINTS = ["rec_ple_cgc_workspace_bytes", "rec_ple_cgc_fwd_f32", "rec_ple_cgc_bwd_f32"]
# (B, Din, Gin, T, S, Sh, H1, O, Og, last): small odd shapes, all four (Gin, last) combinations
SMALL = [(5, 7, 1, 2, 2, 1, 4, 3, 2, 0), (5, 7, 1, 2, 2, 1, 4, 3, 2, 1), (4, 3, 3, 2, 1, 2, 5, 3, 2, 0),
         (4, 3, 3, 2, 1, 2, 5, 3, 2, 1), (3, 5, 4, 3, 2, 2, 3, 2, 3, 0), (3, 2, 1, 1, 1, 1, 2, 1, 1, 1)]


def _inputs(case, seed=3):
    B, Din, Gin, T, S, Sh, H1, O, Og, last = case
    r = np.random.default_rng(seed)
    params = PR.make_level(r, Din, T, S, Sh, H1, O, Og, last)
    Gout = T if last else T + 1
    return (params, r.normal(0, 1, (B, Gin, Din)), r.uniform(-1, 1, (B, Gout, O)),
            r.uniform(-1, 1, (B, T)) if last else None, (T, S, Sh, last))


@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join(map(str, c)))
def test_numpy_backward_equals_torch_autograd_in_fp64(case):
    params, xin, dy, dout, cfg = _inputs(case)
    ref = PR.level_numpy(xin, params, *cfg, dy, dout)
    y, out, dxin, dparams, saved = PR.level_torch_grads(xin, params, *cfg, dy, dout, torch.float64)
    assert PR.rel_err(y, ref["y"]) < 1e-13 and PR.rel_err(dxin, ref["dxin"]) < 1e-12
    assert (out is None and ref["out"] is None) if not cfg[3] else PR.rel_err(out, ref["out"]) < 1e-13
    for name in PR.SAVED:
        assert saved[name].shape == ref[name].shape and PR.rel_err(saved[name], ref[name]) < 1e-13, name
    for name, got, want in zip(PR.NAMES, dparams, ref["dparams"]):
        assert (got is None) == (want is None), name
        if got is not None:
            assert got.shape == want.shape and PR.rel_err(got, want) < 1e-12, name


@pytest.mark.parametrize("L", [1, 2, 3])
def test_numpy_body_equals_torch_autograd_in_fp64(L):
    r = np.random.default_rng(L)
    levels = PR.make_body(r, 5, 2, 2, 1, L, H1=4, O=3, Og=2)
    x, dout = r.normal(0, 1, (6, 5)), r.uniform(-1, 1, (6, 2))
    ref = PR.body_numpy(x, levels, 2, 2, 1, dout)
    out, dx, dparams = PR.body_torch_grads(x, levels, 2, 2, 1, dout, torch.float64)
    assert PR.rel_err(out, ref["out"]) < 1e-13 and PR.rel_err(dx, ref["dx"]) < 1e-12
    for got_l, want_l in zip(dparams, ref["dparams"]):
        for name, got, want in zip(PR.NAMES, got_l, want_l):
            assert (got is None) == (want is None) and (got is None or PR.rel_err(got, want) < 1e-12), name


def test_numpy_backward_equals_central_differences():
    """two levels: a first level with a shared gate, a grouped last level with towers"""
    T, S, Sh, L = 2, 2, 1, 2

    def gen(seed):
        r = np.random.default_rng(seed)
        return PR.make_body(r, 5, T, S, Sh, L, H1=4, O=3, Og=2), r.normal(0, 1, (3, 5)), r.uniform(-1, 1, (3, T))

    def close_to_a_kink(seed):
        levels, x, _ = gen(seed)
        return PR.body_numpy(x, levels, T, S, Sh)["pre"].min() < 1e-3

    levels, x, dout = gen(PR.clean_seed(close_to_a_kink))
    ref = PR.body_numpy(x, levels, T, S, Sh, dout)
    loss = lambda xx, lv: float((PR.body_numpy(xx, lv, T, S, Sh)["out"] * dout).sum())
    eps, r = 1e-6, np.random.default_rng(0)

    def fd_of(base, rebuild):
        at = tuple(int(r.integers(0, s)) for s in base.shape)
        hi, lo = base.copy(), base.copy()
        hi[at] += eps
        lo[at] -= eps
        return at, (rebuild(hi) - rebuild(lo)) / (2 * eps)

    for _ in range(4):
        at, fd = fd_of(x, lambda xx: loss(xx, levels))
        assert abs(fd - ref["dx"][at]) <= 1e-7 + 1e-6 * abs(ref["dx"][at]), ("x", at)
    for lv in range(L):
        for k, base in enumerate(levels[lv]):
            if base is None:
                assert ref["dparams"][lv][k] is None
                continue
            for _ in range(4):                            # four random elements of every tensor
                swap = lambda a: loss(x, levels[:lv] + [levels[lv][:k] + [a] + levels[lv][k + 1:]] + levels[lv + 1:])
                at, fd = fd_of(base, swap)
                want = ref["dparams"][lv][k][at]
                assert abs(fd - want) <= 1e-7 + 1e-6 * abs(want), (lv, PR.NAMES[k], at, fd, want)


def _softmax(z):
    ex = np.exp(z - z.max(-1, keepdims=True))
    return ex / ex.sum(-1, keepdims=True)


def test_structure_is_the_references():
    case = SMALL[4]                                       # grouped, three tasks, a shared gate
    B, Din, Gin, T, S, Sh, H1, O, Og, last = case
    params, xin, _, _, cfg = _inputs(case)
    ne, ns = T * S + Sh, S + Sh
    res = PR.level_numpy(xin, params, *cfg)
    q, e = res["q"].reshape(B, T + 1, Og), res["e"].reshape(B, ne, O)
    # task gates: softmax(softmax(.)); the shared gate: one softmax over all ne experts
    once = _softmax(np.einsum("btk,tkj->btj", q[:, :T], params[6]))
    assert res["g"].shape == (B, T * ns + ne)
    assert np.allclose(res["g"][:, :T * ns].reshape(B, T, ns), _softmax(once), rtol=1e-14, atol=0)
    assert not np.allclose(res["g"][:, :T * ns].reshape(B, T, ns), once, rtol=1e-3, atol=0)
    gh = res["g"][:, T * ns:]
    assert np.allclose(gh, _softmax(q[:, T] @ params[7]), rtol=1e-14, atol=0) and np.allclose(gh.sum(1), 1)
    # y is the weighted SUM over the experts: [B, T + 1, O], not the [B, ., ns O] of a flatten
    assert res["y"].shape == (B, T + 1, O) and res["out"] is None
    idx = PR.task_experts(T, S, Sh)
    for t in range(T):
        want = sum(res["g"][:, t * ns + j, None] * e[:, idx[t, j]] for j in range(ns))
        assert np.allclose(res["y"][:, t], want, rtol=1e-14, atol=1e-300)
    assert np.allclose(res["y"][:, T], sum(gh[:, i, None] * e[:, i] for i in range(ne)), rtol=1e-14, atol=1e-300)
    # expert i reads group i / S, a shared expert and the shared gate group T, task gate t group t
    assert PR.groups(T, S, Sh, False) == [0, 0, 1, 1, 2, 2, 3, 3, 0, 1, 2, 3]
    for g in range(T + 1):
        moved = xin.copy()
        moved[:, g] += 1.0
        other = PR.level_numpy(moved, params, *cfg)
        he_ = np.abs(other["h"] - res["h"]).reshape(B, -1, H1).max((0, 2)) > 0
        assert [m for m in range(len(he_)) if he_[m]] == [m for m, gm in enumerate(PR.groups(T, S, Sh, False)) if gm == g]
    # the last level: T outputs, towers, no shared-gate parameters
    params, xin, _, _, cfg = _inputs(SMALL[3])
    res = PR.level_numpy(xin, params, *cfg)
    assert res["y"].shape == (4, 2, 3) and res["out"].shape == (4, 2) and res["g"].shape == (4, 2 * 3)
    assert params[7] is None and params[8].shape == (2, 3) and PR.groups(2, 1, 2, True) == [0, 1, 2, 2, 0, 1]
    want = 1 / (1 + np.exp(-((res["y"] * params[8][None]).sum(2) + params[9])))
    assert np.allclose(res["out"], want, rtol=1e-14, atol=0)
    # one level is legal: a last level reading x for every branch
    r = np.random.default_rng(1)
    levels = PR.make_body(r, 5, 2, 2, 1, 1, H1=4, O=3, Og=2)
    x = r.normal(0, 1, (3, 5))
    one = PR.body_numpy(x, levels, 2, 2, 1)
    assert np.array_equal(one["out"], PR.level_numpy(x[:, None], levels[0], 2, 2, 1, True)["out"])


# ---- the layer ------------------------------------------------------------------------------------------------------
def _want_names(F, E, S, Sh, L, T=3):
    want = {"embedding_layer.embeddings": None}
    for lv in range(L):
        din = F * E if lv == 0 else 8
        mlp = lambda pre: {pre + "kernel_0": (din, 64), pre + "bias_0": (64,), pre + "kernel_1": (64, 8),
                           pre + "bias_1": (8,)}
        for i in range(T * S):
            want.update(mlp("specific_expert_networks.%d.%d." % (lv, i)))
        for k in range(Sh):
            want.update(mlp("shared_expert_networks.%d.%d." % (lv, k)))
        for t in range(T):
            want.update(mlp("specific_gates.%d.%d.0." % (lv, t)))
            want["specific_gates.%d.%d.1.kernel_0" % (lv, t)] = (8, S + Sh)
        if lv < L - 1:
            want.update(mlp("shared_gates.%d.0." % lv))
            want["shared_gates.%d.1.kernel_0" % lv] = (8, T * S + Sh)
    for t in range(T):
        want.update({"tower_outputs.%d.kernel_0" % t: (8, 1), "tower_outputs.%d.bias_0" % t: (1,)})
    return want


def test_layer_signature_state_dict_names_and_parameter_count():
    from explicit_tf2_recommendation_amd import layers
    sig = inspect.signature(layers.PLELayer.__init__)
    assert list(sig.parameters)[1:] == ["categorical_features", "continuous_features", "feature_dims", "embedding_dims",
                                        "specific_expert_num", "shared_expert_num", "level_num"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["categorical_features"] == CAT and d["continuous_features"] == CONT
    assert (d["feature_dims"], d["embedding_dims"], d["specific_expert_num"], d["shared_expert_num"], d["level_num"]) == \
        (160000, 8, 3, 3, 2)
    assert "PLELayer" in layers.__doc__ and layers.PLELayer.num_tasks == 3
    lay = layers.PLELayer(feature_dims=50)
    want = _want_names(9, 8, 3, 3, 2)
    want["embedding_layer.embeddings"] = (50, 8)
    assert {k: tuple(v.shape) for k, v in lay.state_dict().items()} == want
    assert not [k for k in want if k.startswith("shared_gates.1")] and len(lay.shared_gates) == 1
    # 12 experts and 3 + 1 gate MLPs over 72 inputs, 12 and 3 over 8, the gates' dense layers, three towers
    mlp = lambda din: din * 64 + 64 + 64 * 8 + 8
    count = 50 * 8 + 16 * mlp(72) + 3 * 8 * 6 + 8 * 12 + 15 * mlp(8) + 3 * 8 * 6 + 3 * 9
    assert sum(p.numel() for p in lay.parameters()) == count == 400 + 83312 + 16584 + 27
    # the packed operands are the sub-layers' parameters in the layout of tests/ple_ref.py
    packed = [[None if t is None else t.detach().numpy() for t in lay.packed_weights(lv)] for lv in range(2)]
    assert [t is None for t in packed[0]] == [False] * 7 + [False, True, True]
    assert [t is None for t in packed[1]] == [False] * 7 + [True, False, False]
    sd = PR.state_dict_of(lay.embedding_layer.embeddings.detach().numpy(), packed, 3, 3, 3)
    assert sd.keys() == want.keys()
    for k, v in lay.state_dict().items():
        assert np.array_equal(np.asarray(sd[k]).reshape(v.shape), v.numpy()), k
    other = layers.PLELayer(categorical_features=["a", "b"], feature_dims=20, embedding_dims=4, specific_expert_num=2,
                            shared_expert_num=1, level_num=3)
    w = _want_names(2, 4, 2, 1, 3)
    w["embedding_layer.embeddings"] = (20, 4)
    assert {k: tuple(v.shape) for k, v in other.state_dict().items()} == w
    one = layers.PLELayer(feature_dims=20, level_num=1)   # one level: a last level, no shared gate anywhere
    assert len(one.shared_gates) == 0 and one.packed_weights(0)[7] is None and one.packed_weights(0)[8] is not None
    with pytest.raises(ValueError):
        layers.PLELayer(feature_dims=20, level_num=0)
    with pytest.raises(NotImplementedError, match="512"):
        layers.PLELayer(categorical_features=["f%d" % i for i in range(65)], feature_dims=50)
    with pytest.raises(NotImplementedError, match="128"):
        layers.PLELayer(feature_dims=50, specific_expert_num=5, shared_expert_num=2)       # 17 experts of 8 outputs


# (Din, Gin, T, S, Sh, H1, O, Og, last)
LIMIT_OK = [(512, 1, 3, 3, 3, 64, 8, 8, 0), (72, 1, 4, 2, 2, 64, 8, 8, 0), (72, 1, 3, 3, 3, 128, 8, 8, 0),
            (72, 1, 3, 4, 4, 64, 8, 8, 0), (72, 1, 3, 3, 3, 64, 8, 32, 0), (72, 1, 1, 32, 32, 64, 2, 8, 0),
            (72, 1, 1, 32, 64, 64, 1, 8, 1), (32, 4, 3, 3, 3, 64, 8, 8, 1), (1, 1, 1, 1, 1, 1, 1, 1, 1),
            (8, 4, 3, 4, 4, 64, 8, 8, 0), (512, 1, 4, 2, 2, 128, 12, 8, 0)]
LIMIT_PAST = [((513, 1, 3, 3, 3, 64, 8, 8, 0), "512"), ((72, 1, 5, 2, 2, 64, 8, 8, 0), "4"),
              ((72, 1, 3, 3, 3, 129, 8, 8, 0), "128"), ((72, 1, 3, 4, 4, 64, 9, 8, 0), "128"),
              ((72, 1, 3, 3, 3, 64, 8, 33, 0), "128"), ((72, 1, 1, 33, 32, 64, 1, 8, 0), "128"),
              ((72, 1, 1, 32, 97, 64, 1, 8, 1), "128"), ((33, 4, 3, 3, 3, 64, 8, 8, 1), "128")]


def test_check_shape_at_and_one_past_each_limit():
    from explicit_tf2_recommendation_amd import ops
    for shape in LIMIT_OK:
        ops.ple_check_shape(*shape)
    for shape, word in LIMIT_PAST:
        with pytest.raises(NotImplementedError, match=word):
            ops.ple_check_shape(*shape)
    for k in range(8):
        bad = [72, 1, 3, 3, 3, 64, 8, 8]
        bad[k] = 0
        with pytest.raises(ValueError):
            ops.ple_check_shape(*bad)
    with pytest.raises(ValueError):                       # neither one input group nor tasks + 1
        ops.ple_check_shape(8, 3, 3, 3, 3)
    t = torch.zeros(2, 1, 4)
    w = [torch.zeros(s) for s in ((4, 10), (10,), (3, 2, 2), (3, 2), (2, 2, 1), (2, 1), (2, 1, 2))] + [None,
        torch.zeros(2, 2), torch.zeros(2)]
    with pytest.raises(RuntimeError):                     # there is no CPU path
        ops.ple_cgc_fwd(t, w, 2, 1, 1, last=True)
    with pytest.raises(ValueError):                       # a last level with a shared gate
        ops.ple_cgc_fwd(t, w[:7] + [torch.zeros(1, 3)] + w[8:], 2, 1, 1, last=True)


def test_header_declares_the_entry_points_and_adds_no_constant():
    from explicit_tf2_recommendation_amd import _lib
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    assert _lib.SIGNATURES["rec_ple_cgc_workspace_bytes"] == (C.c_size_t, [C.c_int64] + [C.c_int] * 9)
    assert len(_lib.SIGNATURES["rec_ple_cgc_fwd_f32"][1]) == 11 + 10 + 6 + 1
    assert len(_lib.SIGNATURES["rec_ple_cgc_bwd_f32"][1]) == 15 + 10 + 11 + 3
    assert not [k for k in list(_lib.LIMITS) + list(_lib.ENUMS) if "PLE" in k.upper().split("_")]


def test_abi_status_codes_without_a_gpu():
    from explicit_tf2_recommendation_amd._lib import lib
    d = C.c_void_p(16)                                    # never dereferenced: every call below fails its checks
    ws = lib.rec_ple_cgc_workspace_bytes
    base = dict(B=4, Din=72, Gin=1, T=3, S=3, Sh=3, H1=64, O=8, Og=8, last=0)
    keys = ("Din", "Gin", "T", "S", "Sh", "H1", "O", "Og", "last")

    def fwd(x=d, y=d, save=(d,) * 4, ptr=None, **kw):
        a = dict(base, **kw)
        p = dict(Wg3h=None if a["last"] else d, Wtw=d if a["last"] else None, btw=d if a["last"] else None,
                 out=d if a["last"] else None)
        p.update(ptr or {})
        return lib.rec_ple_cgc_fwd_f32(x, *[d] * 7, p["Wg3h"], p["Wtw"], p["btw"], a["B"], *[a[k] for k in keys], y,
                                       p["out"], *save, None)

    def bwd(x=d, dx=d, g=d, ws_=d, nbytes=1 << 30, ptr=None, **kw):
        a = dict(base, **kw)
        la = a["last"]
        p = dict(Wg3h=None if la else d, Wtw=d if la else None, out=d if la else None, dy=d, dout=d if la else None,
                 dWg3h=None if la else d, dWtw=d if la else None, dbtw=d if la else None)
        p.update(ptr or {})
        return lib.rec_ple_cgc_bwd_f32(x, *[d] * 4, p["Wg3h"], p["Wtw"], *[d] * 3, g, d, p["out"], p["dy"], p["dout"],
                                       a["B"], *[a[k] for k in keys], dx, *[d] * 7, p["dWg3h"], p["dWtw"], p["dbtw"],
                                       ws_, nbytes, None)

    for shape in LIMIT_OK:
        kw = dict(zip(keys, shape))
        assert ws(17, *shape) > 0, shape
        assert fwd(B=0, **kw) == 0 and bwd(B=0, ws_=None, **kw) == 0
    for shape, _ in LIMIT_PAST:
        kw = dict(zip(keys, shape))
        assert ws(17, *shape) == 0, shape
        assert fwd(B=0, **kw) == -2 and fwd(**kw) == -2 and bwd(**kw) == -2
    ok = [base[k] for k in keys]
    assert ws(-1, *ok) == 0 and ws(4, 0, *ok[1:]) == 0 and ws(0, *ok) > 0
    assert fwd(x=None) == -1 and fwd(y=None) == -1 and bwd(x=None) == -1 and bwd(dx=None) == -1 and bwd(g=None) == -1
    assert fwd(save=(d, None, d, d)) == -1 and fwd(save=(d, d, d, None)) == -1               # save buffers given in part
    for k in ("B",) + keys:
        assert fwd(**{k: -1}) == -1 and bwd(**{k: -1}) == -1, k
        if k not in ("B", "last"):
            assert fwd(**{k: 0}) == -1 and fwd(B=0, **{k: 0}) == -1, k
    assert fwd(last=2) == -1 and fwd(Gin=2) == -1 and fwd(Gin=3) == -1 and fwd(B=0, Gin=4, Din=8) == 0
    # what belongs to the last level alone, and what to the others alone
    assert fwd(ptr=dict(Wg3h=None)) == -1 and fwd(ptr=dict(Wtw=d)) == -1 and fwd(ptr=dict(out=d)) == -1
    assert fwd(last=1, ptr=dict(Wg3h=d)) == -1 and fwd(last=1, ptr=dict(Wtw=None)) == -1
    assert fwd(last=1, ptr=dict(out=None)) == -1 and fwd(last=1, ptr=dict(btw=None)) == -1
    assert bwd(ptr=dict(dy=None)) == -1 and bwd(ptr=dict(dout=d)) == -1 and bwd(ptr=dict(dWg3h=None)) == -1
    assert bwd(last=1, ptr=dict(dout=None)) == -1 and bwd(last=1, ptr=dict(dWtw=None)) == -1
    assert bwd(last=1, ptr=dict(dWg3h=d)) == -1
    assert bwd(ws_=None) == -1 and bwd(nbytes=16) == -3 and bwd(last=1, nbytes=16) == -3
    assert bwd(last=1, ptr=dict(dy=None), nbytes=16) == -3                                   # dy is optional there
    # per example 4 (N1 + ne O + Gout Og + GW + T) bytes; the rest does not grow with the batch beyond the slots
    per = 4 * (1024 + 96 + 32 + 27 + 3)
    w1, w2 = ws(8192, *ok), ws(16384, *ok)
    assert 8192 * per < w1 and 8192 * per <= w2 - w1 < 8192 * (per + per // 32 + 64)


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PR.LEVEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_near_kink_share_of_every_gpu_level_case(case):
    """What tests/test_gpu_ple.py relies on, checked on the fp64 reading: at most 10 % of a case's examples have a relu
    pre-activation below PRE_EPS, none in a case under 100 examples, and their gradient rows are zero."""
    c = PR.level_case(*case)
    near = c["near"]
    assert np.array_equal(near, c["ref"]["pre"] < PR.PRE_EPS)
    print("near-kink examples: %d of %d (seed %d)" % (near.sum(), len(near), c["seed"]))
    assert near.mean() <= 0.10 and (case[0] >= 100 or not near.any())
    assert np.count_nonzero(c["dy"][near]) == 0 and np.count_nonzero(c["dy"][~near]) > 0
    if case[9]:
        assert np.count_nonzero(c["dout"][near]) == 0 and np.count_nonzero(c["dout"][~near]) > 0


@pytest.mark.parametrize("case", PR.BODY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_near_kink_share_of_every_gpu_body_case(case):
    c = PR.body_case(*case)
    print("near-kink examples: %d of %d (seed %d)" % (c["near"].sum(), len(c["near"]), c["seed"]))
    assert np.array_equal(c["near"], c["ref"]["pre"] < PR.PRE_EPS) and not c["near"].any()
    assert len(c["levels"]) == case[5] and np.count_nonzero(c["dout"]) > 0


def test_near_kink_share_of_the_layer_case_and_at_2049_with_three_levels():
    seed, table, X, levels = PR.layer_case()
    assert not (PR.body_numpy(table[X].reshape(PR.LAYER_B, -1), levels, 3, 3, 3)["pre"] < PR.PRE_EPS).any()
    # the scales of the generator keep the share small where the levels are chained, too
    r = np.random.default_rng(1)
    levels = PR.make_body(r, 72, 3, 3, 3, 3)
    share = (PR.body_numpy(r.normal(0, 1, (2049, 72)), levels, 3, 3, 3)["pre"] < PR.PRE_EPS).mean()
    print("three levels, 2049 examples: %.2f %% near a kink" % (100 * share))
    assert share <= 0.10
