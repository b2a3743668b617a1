"""DMT on the GPU: dmt.EncoderLayer on the attention, LayerNorm and GEMM kernels against the fp64 numpy reading of
tests/dmt_ref.py under four masks -- all valid, all padded, a valid prefix, holes -- with every gradient, LayerNorm with a
given epsilon, bit identity run to run, the error paths, the layers (Encoder, DeepInterestTransformer, DMTLayer in both
``head`` modes, fused and composed) against the torch-CPU transcription, and one graphed train step.

Tolerance, per tensor (the project's rule, as tests/test_gpu_sim.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  Every check prints `name error / bound`.
dbk -- zero in exact arithmetic, rounding residue in every implementation -- is normalised by max|dbq| instead of its own
maximum, against 4 x the transcription's same ratio with the 3e-5 floor.

Measured on the MI355X, the printout as a DIGEST (2372 `error / bound` lines in all).  40 passed in 5.6 s.  2328 of the
bounds sit on their floor.  Largest error / bound ratios: encoder layer 0.26 (dW1 of 1x1x2x1x2x2, where a LayerNorm over
two features makes the fp32 transcription itself 0.46 off: 4.78e-01 / 1.83 -- for the gradients behind a LayerNorm of that
case the rule's bound is above 1, so the case checks their shapes, finiteness and exact zeros, and z), LayerNorm with
epsilon 0.01, the layers fused
0.08 (a decoder value bias 2.31e-06 / 3.00e-05), composed 0.29 (ctr_gate's softmax bias 8.61e-06 / 3.00e-05).
"""
import copy

import numpy as np
import pytest
import torch

from tests import dmt_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = R.rel_err(got, want), max(floor, 4 * R.rel_err(t32, want))
    print("%-22s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


def check_dbk(name, got, want, t32, dbq):
    """dbk by the scale of dbq: its own maximum is rounding residue"""
    scale = np.abs(dbq).max() or 1.0
    err, bound = np.abs(got - want).max() / scale, max(3e-5, 4 * np.abs(t32 - want).max() / scale)
    print("%-22s error/bound %.2e / %.2e = %.2f (by max|dbq|)" % (name, err, bound, err / bound))
    assert got.shape == want.shape and err <= bound, (name, err, bound)


_DEV = {}


def dev(case):
    if case not in _DEV:
        c = R.inputs(case)
        _DEV[case] = {"x": cu(c["x"]), "gz": cu(c["gz"]), "w": tuple(cu(c["w"][n]) for n in R.WEIGHTS),
                      "masks": {m: cu(v, np.int32) for m, v in c["masks"].items()}}
    return _DEV[case]


def encoder_layer(case, fused=True):
    """dmt.EncoderLayer with the case's weights: its 16 parameters in the order of R.WEIGHTS"""
    from explicit_tf2_recommendation_amd import dmt, layers
    B, T, D, H, dk, dff = case
    lay = dmt.EncoderLayer(D, H, dff, fused=fused)
    if dk != D:                                              # the reference builds MultiHeadAttention(num_heads, d_model);
        lay.mha = layers.MultiHeadAttention(H, key_dim=dk, input_dim=D)     # the cases also take key_dim apart from it
    lay = lay.cuda()
    f0, f1 = lay.ffn.layers
    params = lay.mha.weights() + (lay.layernorm1.gamma, lay.layernorm1.beta, f0.kernel, f0.bias, f1.kernel, f1.bias,
                                  lay.layernorm2.gamma, lay.layernorm2.beta)
    with torch.no_grad():
        for q, t in zip(params, dev(case)["w"]):
            q.copy_(t)
    return lay, params


def run(case, mask, fused=True):
    """-> z, then gx and the 16 weight gradients (R.GRADS)"""
    d = dev(case)
    lay, params = encoder_layer(case, fused)
    x = d["x"].clone().requires_grad_()
    z = lay(x, False, d["masks"][mask])
    (z * d["gz"]).sum().backward()
    return (z.detach(), x.grad) + tuple(q.grad for q in params)


@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("case", R.CASES, ids=ids)
def test_encoder_layer_matches_fp64(case, mask):
    got = run(case, mask)
    ref, t32 = R.cached(R.encoder_numpy, case, mask), R.cached(R.encoder_torch, case, mask, torch.float32)
    assert len(got) == 1 + 17
    for name, t in zip(("z",) + R.GRADS, got):
        if name == "dbk":
            check_dbk(name, host(t), ref[name], t32[name], ref["dbq"])
        else:
            check(name, host(t), ref[name], t32[name], 1e-5 if name == "z" else 3e-5)
    assert all(bool(torch.isfinite(t).all()) for t in got)


def test_every_output_is_bit_identical_run_to_run():
    for case in (R.DEFAULTS, R.RAGGED):
        for a, b in zip(run(case, "holes"), run(case, "holes")):
            assert torch.equal(a, b)


@pytest.mark.parametrize("N", (1, 6, 48, 130))
def test_layernorm_with_a_given_epsilon(N):
    """functional.LayerNorm(epsilon): against fp64 at 1e-6, and the default path bit for bit at 1e-3"""
    from explicit_tf2_recommendation_amd import functional as Fn
    rng = np.random.default_rng(N)
    x, gy = rng.standard_normal((37, N)).astype(F32), rng.standard_normal((37, N)).astype(F32)
    gamma, beta = (1 + 0.2 * rng.standard_normal(N)).astype(F32), (0.2 * rng.standard_normal(N)).astype(F32)

    def torch_ref(dtype, eps):
        ts = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in (x, gamma, beta)]
        y = R.t_ln(ts[0], ts[1], ts[2], eps)
        (y * torch.tensor(gy, dtype=dtype)).sum().backward()
        return [y.detach().numpy()] + [t.grad.numpy() for t in ts]

    def gpu(*eps):
        ts = [cu(a).requires_grad_() for a in (x, gamma, beta)]
        y = Fn.LayerNorm.apply(*ts, *eps)
        (y * cu(gy)).sum().backward()
        return [y.detach()] + [t.grad for t in ts]
    got, r64, r32 = gpu(1e-6), torch_ref(torch.float64, 1e-6), torch_ref(torch.float32, 1e-6)
    for name, g, a, b in zip(("y", "gx", "dgamma", "dbeta"), got, r64, r32):
        check("N=%d %s" % (N, name), host(g), a, b, 1e-5 if name == "y" else 3e-5)
    if N == 1:
        assert torch.equal(got[0], cu(beta).expand(37, 1)) and not got[1].any()          # beta, and nothing upstream
    for a, b in zip(gpu(), gpu(1e-3)):
        assert torch.equal(a, b)                             # the old entry point is the new one at Keras' default
    with pytest.raises(ValueError):
        gpu(0.0)


def test_bad_shapes_and_limits():
    from explicit_tf2_recommendation_amd import dmt
    lay, _ = encoder_layer(R.ODD)
    d = dev(R.ODD)
    B, T, D = R.ODD[:3]
    with pytest.raises(ValueError):
        lay(d["x"][0], False, d["masks"]["valid"][0])
    with pytest.raises(ValueError):
        lay(d["x"], False, d["masks"]["valid"][:, :-1])
    long_x = torch.zeros(2, dmt.MAX_T + 1, D, device="cuda")
    with pytest.raises(NotImplementedError, match="T <= %d" % dmt.MAX_T):
        lay(long_x)
    with pytest.raises(NotImplementedError, match="<= 64"):
        dmt.EncoderLayer(66, 2, 8, fused=True).cuda()(torch.zeros(2, 3, 66, device="cuda"))
    with pytest.raises(NotImplementedError, match="num_heads <= 8"):
        dmt.EncoderLayer(8, 9, 8, fused=True).cuda()(torch.zeros(2, 3, 8, device="cuda"))
    assert tuple(encoder_layer(R.ODD, fused=False)[0](long_x).shape) == (2, dmt.MAX_T + 1, D)   # composed runs there
    for width, heads, key_dim in ((7, 1, 7), (8, 1, 3)):                     # odd d_model, odd key_dim
        odd = dmt.EncoderLayer(width, heads, 4, fused=True)
        if key_dim != width:
            from explicit_tf2_recommendation_amd import layers
            odd.mha = layers.MultiHeadAttention(heads, key_dim=key_dim, input_dim=width)
        with pytest.raises(NotImplementedError, match="even widths"):
            odd.cuda()(torch.zeros(2, 3, width, device="cuda"))
    with pytest.raises(NotImplementedError, match="even widths"):
        dmt.DeepInterestTransformer(1, 7, 1, 4, input_vocab_size=10, fused=True)


def test_empty_batches():
    """B == 0 through the fused classes: shapes kept, every parameter gradient zero, nothing launched"""
    from explicit_tf2_recommendation_amd import dmt
    lay, params = encoder_layer(R.ODD)
    B, T, D = R.ODD[:3]
    x = torch.zeros(0, T, D, device="cuda", requires_grad=True)
    z = lay(x, False, torch.zeros(0, T, dtype=torch.int32, device="cuda"))
    assert tuple(z.shape) == (0, T, D)
    z.sum().backward()
    assert tuple(x.grad.shape) == (0, T, D) and all(q.grad is None or not q.grad.any() for q in params)
    tf = dmt.DeepInterestTransformer(2, D_MODEL, HEADS, DFF, input_vocab_size=50, fused=True).cuda()
    ids0 = torch.zeros(0, 6, dtype=torch.int64, device="cuda")
    out = tf(ids0, ids0[:, :1], False, torch.zeros(0, 6, D_MODEL, device="cuda"), torch.zeros(0, 1, D_MODEL, device="cuda"))
    assert tuple(out.shape) == (0, 1, D_MODEL)


# ---- the layers ----------------------------------------------------------------------------------------------------------
D_MODEL, HEADS, DFF = 3 * R.LAYER_E, 2, 8


def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()}


def _grads(lay):
    out = {}
    for k, q in lay.named_parameters():
        out[k] = np.zeros(tuple(q.shape), F32) if q.grad is None else host(q.grad.to_dense() if q.grad.is_sparse else q.grad)
    return out


def check_grads(tag, grads, g64, g32):
    for k in grads:
        if k.endswith("_key_dense.bias"):
            check_dbk(tag + k, grads[k], g64[k], g32[k], g64[k.replace("_key_dense", "_query_dense")])
        else:
            check(tag + k, grads[k], g64[k], g32[k], 3e-5)


def _tf_inputs(seed, T):
    """series ids [B,T] with a valid prefix (example 1 padded throughout), candidate ids [B,1] (example 2: id 0), the
    embedded inputs and an upstream gradient"""
    rng = np.random.default_rng(seed)
    B = R.LAYER_B
    n = rng.integers(1, T + 1, B)
    n[0], n[1] = T, 0
    enc_ids = rng.integers(1, 50, (B, T)) * (np.arange(T)[None, :] < n[:, None])
    dec_ids = rng.integers(1, 50, (B, 1))
    dec_ids[2] = 0
    f = lambda *s: (0.7 * rng.standard_normal(s)).astype(F32)
    return enc_ids, dec_ids, f(B, T, D_MODEL), f(B, 1, D_MODEL), f(B, 1, D_MODEL), f(B, T, D_MODEL)


def _torch_ref(fn, sd, tensors, gout, dtype):
    """fn(state, *tensors) in dtype -> (output, {name: gradient}, gradients of the tensors)"""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    ts = [torch.tensor(t, dtype=dtype, requires_grad=True) for t in tensors]
    out = fn(p, *ts)
    (out * torch.tensor(gout, dtype=dtype)).sum().backward()
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in p.items()}, [t.grad.numpy() for t in ts]


@pytest.mark.parametrize("T", (6, 16))
@pytest.mark.parametrize("layers_num", (1, 3))
def test_encoder_stack_fused_and_composed_against_the_transcription(layers_num, T):
    from explicit_tf2_recommendation_amd import dmt
    enc_ids, _, x_enc, _, _, gout = _tf_inputs(7, T)
    valid = torch.from_numpy(enc_ids != 0)
    results = {}
    for fused in (True, False):
        lay = dmt.Encoder(layers_num, D_MODEL, HEADS, DFF, fused=fused)
        sd = R.layer_state(8, {k: tuple(v.shape) for k, v in lay.state_dict().items()})
        lay.load_state_dict(_tensors(sd))
        lay = lay.cuda()
        fn = lambda p, x: R.encoder_stack_torch(p, "", x, valid.to(x.dtype), layers_num)
        sdp = {"." + k: v for k, v in sd.items()}
        (o64, g64, x64), (o32, g32, x32) = (_torch_ref(fn, sdp, [x_enc], gout, dt) for dt in (torch.float64, torch.float32))
        x = cu(x_enc).requires_grad_()
        out = lay(x, False, valid.cuda())
        (out * cu(gout)).sum().backward()
        tag = "fused " if fused else "composed "
        check(tag + "out", host(out), o64, o32, 1e-5)
        check(tag + "gx", host(x.grad), x64[0], x32[0], 3e-5)
        check_grads(tag, _grads(lay), {k[1:]: v for k, v in g64.items()}, {k[1:]: v for k, v in g32.items()})
        results[fused] = host(out)
    assert R.rel_err(results[True], results[False]) <= 1e-5


@pytest.mark.parametrize("T", (6, 16))
def test_deep_interest_transformer_fused_and_composed_against_the_transcription(T):
    """with a candidate id of 0 and a series padded throughout in the batch: the decoder then attends uniformly over the
    encoder's rows, which are real data"""
    from explicit_tf2_recommendation_amd import dmt
    enc_ids, dec_ids, x_enc, x_dec, gout, _ = _tf_inputs(9, T)
    e_ids, d_ids = torch.from_numpy(enc_ids), torch.from_numpy(dec_ids)
    results = {}
    for fused in (True, False):
        lay = dmt.DeepInterestTransformer(2, D_MODEL, HEADS, DFF, input_vocab_size=50, fused=fused)
        sd = R.layer_state(10, {k: tuple(v.shape) for k, v in lay.state_dict().items()})
        lay.load_state_dict(_tensors(sd))
        lay = lay.cuda()
        fn = lambda p, xe, xd: R.transformer_torch(p, "tf", e_ids, d_ids, xe, xd, 2)
        sdp = {"tf." + k: v for k, v in sd.items() if k != "embedding.embeddings"}
        (o64, g64, x64), (o32, g32, x32) = (_torch_ref(fn, sdp, [x_enc, x_dec], gout, dt)
                                            for dt in (torch.float64, torch.float32))
        xe, xd = cu(x_enc).requires_grad_(), cu(x_dec).requires_grad_()
        out = lay(e_ids.cuda(), d_ids.cuda(), False, xe, xd)
        assert tuple(out.shape) == (R.LAYER_B, 1, D_MODEL)
        (out * cu(gout)).sum().backward()
        tag = "fused " if fused else "composed "
        check(tag + "out", host(out), o64, o32, 1e-5)
        check(tag + "gx_enc", host(xe.grad), x64[0], x32[0], 3e-5)
        check(tag + "gx_dec", host(xd.grad), x64[1], x32[1], 3e-5)
        grads = _grads(lay)
        assert not grads.pop("embedding.embeddings").any()                    # the embedded inputs were given
        check_grads(tag, grads, {k[3:]: v for k, v in g64.items()}, {k[3:]: v for k, v in g32.items()})
        results[fused] = host(out)
    assert R.rel_err(results[True], results[False]) <= 1e-5
    long_ids = torch.ones(2, 17, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="T <= 16"):
        lay_f = dmt.DeepInterestTransformer(1, D_MODEL, HEADS, DFF, input_vocab_size=50, fused=True).cuda()
        lay_f(long_ids, long_ids[:, :1], False)
    assert tuple(lay(long_ids, long_ids[:, :1], False).shape) == (2, 1, D_MODEL)     # composed runs there


def _dmt_layer(head, fused):
    from explicit_tf2_recommendation_amd.dmt import DMTLayer
    lay = DMTLayer(user_and_context_categorical_features=R.USER_F, item_categorical_features=R.ITEM_F,
                   continuous_features=R.CONT_F, feature_dims=R.LAYER_V, embedding_dims=R.LAYER_E, tf_dim=D_MODEL,
                   tf_layers_num=2, tf_heads_num=HEADS, tf_dff=DFF, expert_units=[10, 6], expert_num=2, gate_units=[5],
                   max_position=R.MAX_POSITION, max_page=R.MAX_PAGE, head=head, fused=fused)
    sd = R.layer_state(3, {k: tuple(v.shape) for k, v in lay.state_dict().items()})
    lay.load_state_dict(_tensors(sd))
    return lay.cuda(), sd


@pytest.mark.parametrize("head", ("reference", "linear"))
def test_dmt_layer_fused_and_composed_against_the_transcription(head):
    from explicit_tf2_recommendation_amd import data
    ins = R.layer_inputs(4, R.LAYER_B, 6)
    weight = ins.pop("weight")
    results = {}
    for fused in (True, False):
        lay, sd = _dmt_layer(head, fused)
        t64, t32 = (R.dmt_layer_torch(sd, ins, dt, head, 2, weight=weight) for dt in (torch.float64, torch.float32))
        batch = data.to_device(ins)
        keys = set(batch)
        res = lay(batch)
        assert res.keys() == {"ctr_logits", "cvr_logits"} and set(batch) == keys
        tag = "fused " if fused else "composed "
        for k in ("ctr_logits", "cvr_logits"):
            assert tuple(res[k].shape) == (R.LAYER_B, 1)
            check(tag + k, host(res[k]), t64[k], t32[k], 1e-5)
            assert (np.ptp(host(res[k])) == 0) == (head == "reference")
        (torch.cat([res["ctr_logits"], res["cvr_logits"]], 1) * cu(weight)).sum().backward()
        grads = _grads(lay)
        assert grads.keys() == t64["grads"].keys()
        check_grads(tag, grads, t64["grads"], t32["grads"])                   # exact zeros upstream in 'reference'
        if head == "reference":
            assert not grads["id_embed.embeddings"].any()
            assert sum(bool(g.any()) for g in grads.values()) <= 8
        results[fused] = res
    for k in ("ctr_logits", "cvr_logits"):
        assert R.rel_err(host(results[True][k]), host(results[False][k])) <= 1e-5


def test_graphed_train_step_with_keras_bce_equals_eager():
    from explicit_tf2_recommendation_amd import data, engine, functional as Fn
    lay, _ = _dmt_layer("linear", True)
    eager = copy.deepcopy(lay)
    output_fn = lambda l, x: torch.cat(list(l(x).values()), 1)
    loss_fn = lambda out, y: Fn.KerasBCE.apply(out[:, :1], y[:, :1].contiguous()) \
        + Fn.KerasBCE.apply(out[:, 1:], y[:, 1:].contiguous())

    def batch_of(seed):
        ins = R.layer_inputs(seed, R.LAYER_B, 6)
        ins.pop("weight")
        rng = np.random.default_rng(seed)
        ins["ctr_label"], ins["cvr_label"] = rng.integers(0, 2, R.LAYER_B), rng.integers(0, 2, R.LAYER_B)
        return data.to_device(ins)

    batches = [batch_of(s) for s in (11, 12, 13)]
    labels = ("ctr_label", "cvr_label")
    step = engine.GraphedTrainStep(lay, batches[0], label_name=labels, output_fn=output_fn, loss_fn=loss_fn)
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        out = output_fn(eager, {k: v for k, v in b.items() if k not in labels})
        want = loss_fn(out, torch.stack([b[n].to(torch.float32) for n in labels], 1))
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach().reshape(()))
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            assert a.grad is not None and q.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
