"""DIN attention (csrc/din.hip) on every kernel class its dispatcher can pick, against the fp64 literal ActivationUnit.

tests/din_classes_ref.py holds the shapes (CASES), the restatement of the dispatch (kernel_class) and the references;
tests/test_din_classes_host.py proves on the CPU that CASES reaches all 15 (NT, ND) template pairs, both row paths, both
Eff load paths and both kinds of two-pass backward, that the fp64 references agree, and that no relu / prelu case sits on
the kink.  Here every case runs Fn.DinAttention forward and backward and compares scores, pooled and the gradients of q,
the table, W1, b1, W2, b2 and alpha.  Further: strided tables and a misaligned Mext bit for bit, ids outside the table
at the ops level, the single-key path DinActivationLayer.forward with its gradients, and the envelope.

Tolerances: outputs 1e-5, gradients 3e-5, relative to max(1, |ref|max) -- the figures of tests/test_gpu_din.py, set at
D <= 96.  For the wide classes (ND = 8, 16: a contraction up to 2.7 times longer) the bound is the larger of that figure
and 4 x the error of a correct fp32 evaluation of the factorised formula (din_classes_ref.fp32_error, CPU, against the
fp64 literal unit; the 4 covers the summation order of the MFMA tiles).  Measured, rel. to max(1, |ref|max):
  case                D   H    T  fp32 out  fp32 grad  bound o bound g
  nd8_d128          128  36   20  3.92e-07  4.05e-07   1e-05   3e-05
  nd8_d100          100  36    7  2.19e-07  9.69e-07   1e-05   3e-05
  nd16_t5           192  36    5  3.18e-07  6.91e-07   1e-05   3e-05
  nd16_t20          192  36   20  2.33e-07  5.03e-07   1e-05   3e-05
  nd16_t70          192  36   70  4.03e-07  4.08e-07   1e-05   3e-05
  nd16_d136         136  36   18  3.59e-07  8.37e-07   1e-05   3e-05
  nd16_d132_h20     132  20    9  1.83e-07  5.53e-07   1e-05   3e-05
  nd16_d256_h48     256  48   18  3.89e-07  6.16e-07   1e-05   3e-05
  nd8_h17           128  17    6  1.33e-07  4.92e-07   1e-05   3e-05
  nd16_h5           144   5    6  1.02e-07  5.05e-07   1e-05   3e-05
  nt_nd8_h16        128  16    6  1.77e-07  3.77e-07   1e-05   3e-05
  nt_nd8_h64        128  64    6  1.81e-07  2.96e-07   1e-05   3e-05
  c25_e4            100  36   18  1.96e-07  4.82e-07   1e-05   3e-05
  edge_e64_t1       192  36    1  1.96e-07  3.94e-07   1e-05   3e-05
  edge_e64_t15      192  36   15  8.30e-07  6.78e-07   1e-05   3e-05
  edge_e64_t16      192  36   16  2.87e-07  4.13e-07   1e-05   3e-05
  edge_e64_t17      192  36   17  3.79e-07  5.54e-07   1e-05   3e-05
  edge_e64_t63      192  36   63  1.17e-06  2.05e-06   1e-05   3e-05
  edge_e64_t65      192  36   65  1.02e-06  9.51e-07   1e-05   3e-05
  edge_e64_t129     192  36  129  5.21e-07  3.48e-06   1e-05   3e-05
  act_none_e64      192  36   18  6.18e-07  3.86e-07   1e-05   3e-05
  act_relu_e64      192  36   18  9.76e-07  4.48e-07   1e-05   3e-05
  act_tanh_e64      192  36   18  1.07e-06  4.11e-07   1e-05   3e-05
  act_sigmoid_e64   192  36   18  3.85e-07  3.64e-07   1e-05   3e-05
  act_dice_e64      192  36   18  1.23e-06  7.97e-07   1e-05   3e-05
  act_prelu_e64     192  36   18  5.91e-07  6.04e-07   1e-05   3e-05
4 x the fp32 error is below the project's figure in every row, so the figures hold everywhere (the host test asserts it).
"""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests import din_classes_ref as DR
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    assert torch.cuda.is_available()
    import explicit_tf2_recommendation_amd as pkg
    return pkg


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(got, want, tol, what):
    err = DR.rel_err(host(got) if isinstance(got, torch.Tensor) else got, want)
    print("%-8s rel err %.2e (bound %.0e)" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _act(ops, att):
    a = att["act"]
    kind = ops.DACT_CODE[a["kind"]]
    return kind, *(dev(a[k]) if k in a else None for k in ("alpha", "mean", "var"))


@pytest.mark.parametrize("name", [c.name for c in DR.CASES])
def test_every_kernel_class_vs_literal_activation_unit(R, name):
    ops, Fn = R.ops, R.functional
    case, data, ref = DR.BY_NAME[name], DR.make(DR.BY_NAME[name]), DR.reference(name)
    print(name, "class (NT, ND, NPASS, fast, vec_eff) =", DR.kernel_class(case.E, case.C, case.H, case.E))
    out_tol, grad_tol = DR.tolerances(name)
    att = data["att"]
    kind, alpha, mean, var = _act(ops, att)
    if alpha is not None:
        alpha.requires_grad_()
    emb, q = dev(data["embed"]).requires_grad_(), dev(data["q"]).requires_grad_()
    W1, b1, W2, b2 = [dev(att[k]).requires_grad_() for k in ("W1", "b1", "W2", "b2")]
    flag = ops.new_flag(emb.device)
    pooled, scores = Fn.DinAttention.apply(emb, q, dev(data["series"]), W1, b1, kind, alpha, mean, var, W2, b2,
                                           case.padding_index, case.mask_valid, flag)
    (pooled * dev(data["g"])).sum().backward()
    assert flag.item() == 0
    check(scores, ref["scores"], out_tol, "scores")
    check(pooled, ref["pooled"], out_tol, "pooled")
    check(q.grad, ref["q"], grad_tol, "q")
    check(emb.grad.to_dense(), ref["embed"], grad_tol, "embed")
    for k, t in (("W1", W1), ("b1", b1), ("W2", W2), ("b2", b2)):
        check(t.grad, ref[k], grad_tol, k)
    if alpha is not None:
        check(alpha.grad, ref["alpha"], grad_tol, "alpha")
    else:
        assert ref["alpha"] is None
    p = host(pooled)
    if case.mask_valid:                     # an all-padding series pools to exactly zero, a full one does under the quirk
        assert np.all(p[1] == 0.0) and np.any(p[0] != 0.0)
    else:
        assert np.all(p[0] == 0.0) and np.any(p[1] != 0.0)


# ---- the ops level: one call of rec_din_attn_fwd_f32 and one of rec_din_attn_bwd_f32

OPS_OUT = ("scores", "pooled", "gkeys", "gMext", "gw2p", "galphap", "gb2p")


def ops_call(R, case, data, embed=None, series=None, misalign=False, oob=None):
    """-> {name: numpy} of OPS_OUT.  ``embed``: the table as a device tensor (default: contiguous); ``misalign``: Mext as
    a contiguous view that starts one float into its storage."""
    ops = R.ops
    att, D = data["att"], case.E * case.C
    Wcat, Wkd, bext = ops.din_prepare(dev(att["W1"]), dev(att["b1"]), D, case.H)
    Mext = ops.gemm(dev(data["q"]), Wcat, epi=ops.EPI_BIAS, bias=bext)
    if misalign:
        buf = torch.empty(Mext.numel() + 1, dtype=torch.float32, device=Mext.device)
        shifted = buf[1:].view(Mext.shape)
        shifted.copy_(Mext)
        assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and Mext.data_ptr() % 16 == 0
        Mext = shifted
    kind, alpha, mean, var = _act(ops, att)
    embed = dev(data["embed"]) if embed is None else embed
    series = dev(data["series"] if series is None else series)
    args = (embed, series, Mext, Wkd, kind, alpha, mean, var, dev(att["W2"]).reshape(-1), dev(att["b2"]),
            case.padding_index, case.mask_valid)
    scores, pooled = ops.din_attn_fwd(*args, oob=oob)
    back = ops.din_attn_bwd(*args, scores, dev(data["g"]))
    torch.cuda.synchronize()
    return dict(zip(OPS_OUT, (host(t) for t in (scores, pooled) + tuple(back))))


def check_ops(got, ref, live=None):
    """One ops-level result against the fp64 factorised reference (the host test proves it equal to the literal unit):
    the per-example partials by their sums; ``live`` [B,T,C] selects the key slots whose gradient is compared."""
    check(got["scores"], ref["scores"], DR.OUT_TOL, "scores")
    check(got["pooled"], ref["pooled"], DR.OUT_TOL, "pooled")
    check(got["gMext"], ref["Mext"], DR.GRAD_TOL, "gMext")
    check(got["gw2p"].astype(np.float64).sum(0), ref["W2"].reshape(-1), DR.GRAD_TOL, "gw2p")
    check(got["gb2p"].astype(np.float64).sum(), ref["b2"].reshape(()), DR.GRAD_TOL, "gb2p")
    if ref["alpha"] is not None:
        check(got["galphap"].astype(np.float64).sum(0), ref["alpha"], DR.GRAD_TOL, "galphap")
    gk, want = got["gkeys"], ref["keys"]
    if live is not None:
        B, T_, C = live.shape
        gk, want = gk.reshape(B, T_, C, -1)[live], want.reshape(B, T_, C, -1)[live]
    check(gk, want, DR.GRAD_TOL, "gkeys")


@pytest.mark.parametrize("name", ["act_dice_e8", "nt_e32_h48", "nd16_t20"])
def test_ops_level_matches_the_reference(R, name):
    case = DR.BY_NAME[name]
    flag = R.ops.new_flag("cuda")
    got = ops_call(R, case, DR.make(case), oob=flag)
    assert flag.item() == 0                                  # a clean batch leaves the flag alone
    check_ops(got, DR.reference(name, "factorised"))


@pytest.mark.parametrize("name", ["act_dice_e8", "nt_e32_h48", "nd16_t20"])
def test_misaligned_mext_takes_the_scalar_eff_path_bit_for_bit(R, name):
    case = DR.BY_NAME[name]
    assert DR.kernel_class(case.E, case.C, case.H, case.E)[4]
    assert not DR.kernel_class(case.E, case.C, case.H, case.E, aligned=False)[4]
    data = DR.make(case)
    a, b = ops_call(R, case, data), ops_call(R, case, data, misalign=True)
    for k in OPS_OUT:
        assert np.array_equal(a[k], b[k]), k
    check(a["scores"], DR.reference(name)["scores"], DR.OUT_TOL, "scores")


@pytest.mark.parametrize("extra,fast", [(4, True), (1, False)])
def test_strided_table_bit_for_bit(R, extra, fast):
    """embed = big[:, :E] of a [V, E + extra] buffer: ops._table takes a strided row view, the kernels read it with
    ld = E + extra -- 16-byte pieces at ld = 12, element by element at ld = 9 -- and give what the contiguous table
    gives."""
    case = DR.BY_NAME["act_dice_e8"]
    assert DR.kernel_class(case.E, case.C, case.H, case.E + extra)[3] == fast
    data = DR.make(case)
    big = torch.full((case.V, case.E + extra), float("nan"), dtype=torch.float32, device="cuda")
    big[:, :case.E] = dev(data["embed"])
    view = big[:, :case.E]
    assert view.stride(0) == case.E + extra and not view.is_contiguous()
    a, b = ops_call(R, case, data), ops_call(R, case, data, embed=view)
    for k in OPS_OUT:
        assert np.array_equal(a[k], b[k]), k
    check_ops(b, DR.reference(case.name, "factorised"))


@pytest.mark.parametrize("name", ["act_dice_e8", "nd16_t20"])
def test_ids_outside_the_table_are_zero_rows_and_set_the_flag(R, name):
    """One id equal to V and one equal to -1 at live positions, at the ops level: the flag goes up, those key rows read as
    zeros, and every other result is the reference's with zeros there."""
    case = DR.BY_NAME[name]
    fast = DR.kernel_class(case.E, case.C, case.H, case.E)[3]
    assert fast == (name == "act_dice_e8")
    data = DR.make(case)
    series = data["series"].copy()
    assert data["lens"][0] == case.T and data["lens"][2] > 1
    series[0, 1, 1] = case.V
    series[2, 0, 0] = -1
    zero = (series < 0) | (series >= case.V)
    assert zero.sum() == 2
    flag = R.ops.new_flag("cuda")
    got = ops_call(R, case, data, series=series, oob=flag)
    assert flag.item() == 1
    bad = dict(data, series=series)
    ref = DR.evaluate(bad, case.padding_index, case.mask_valid, torch.float64, "factorised", zero_rows=zero)
    lit = DR.evaluate(bad, case.padding_index, case.mask_valid, torch.float64, "literal", zero_rows=zero)
    assert DR.rel_err(ref["scores"], lit["scores"]) <= 1e-12 and DR.rel_err(ref["pooled"], lit["pooled"]) <= 1e-12
    clean = DR.reference(name)["scores"]
    assert abs(ref["scores"][0, 1] - clean[0, 1]) > 1e-4 and abs(ref["scores"][2, 0] - clean[2, 0]) > 1e-4
    check_ops(got, ref, live=~zero)


GUARD = 128 * 64 + 64            # floats on either side: more than 16 * NMT rows of H units, the most a pass stages


def _guarded(shape):
    """A zero tensor of `shape` inside a larger buffer whose two ends hold a sentinel -> (tensor, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), -77.0, dtype=torch.float32, device="cuda")
    t = buf[GUARD:GUARD + n].view(shape)
    t.zero_()
    return t, buf


@pytest.mark.parametrize("name", ["nt_e4_h17", "slow_e12_t33", "nd8_d100", "nd16_d136", "nd16_d132_h20"])
def test_every_output_stays_inside_its_buffer(R, name):
    """D below the padded D of its class (12 of 32, 36 of 96, 100 of 128, 136 and 132 of 256): the kernels stage whole
    16-row tiles and must store only the real rows.  The C ABI is called with every output inside a buffer with
    sentinels at both ends: none may change, and the outputs are the reference's."""
    ops, L = R.ops, R._lib
    case = DR.BY_NAME[name]
    data, D, Hh, B, T_ = DR.make(case), case.E * case.C, case.H, case.B, case.T
    assert D % 16 and D < 16 * DR.kernel_class(case.E, case.C, Hh, case.E)[1]
    att = data["att"]
    Wcat, Wkd, bext = ops.din_prepare(dev(att["W1"]), dev(att["b1"]), D, Hh)
    Mext = ops.gemm(dev(data["q"]), Wcat, epi=ops.EPI_BIAS, bias=bext)
    kind, alpha, mean, var = _act(ops, att)
    embed, series, g = dev(data["embed"]), dev(data["series"]), dev(data["g"])
    w2, b2 = dev(att["W2"]).reshape(-1), dev(att["b2"])
    p = lambda t: None if t is None else t.data_ptr()
    head = (p(embed), case.E, case.V, case.E, case.C, p(series), B, T_, p(Mext), p(Wkd), Hh, kind, p(alpha), p(mean),
            p(var), p(w2), p(b2), case.padding_index, case.mask_valid)
    shapes = {"scores": (B, T_), "pooled": (B, D), "gkeys": (B, T_, D), "gMext": (B, D * Hh + Hh), "gw2p": (B, Hh),
              "galphap": (B, Hh), "gb2p": (B, 1)}
    out = {k: _guarded(v) for k, v in shapes.items()}
    o = lambda k: p(out[k][0])
    L.check(L.lib.rec_din_attn_fwd_f32(*head, o("scores"), o("pooled"), None, ops._stream()), "rec_din_attn_fwd_f32")
    L.check(L.lib.rec_din_attn_bwd_f32(*head, o("scores"), p(g), None, o("gkeys"), o("gMext"), o("gw2p"), o("galphap"),
                                       o("gb2p"), ops._stream()), "rec_din_attn_bwd_f32")
    torch.cuda.synchronize()
    for k, (t, buf) in out.items():
        ends = torch.cat([buf[:GUARD], buf[GUARD + t.numel():]])
        assert bool((ends == -77.0).all()), k
    check_ops({k: host(t) for k, (t, _) in out.items()}, DR.reference(name, "factorised"))


# ---- DinActivationLayer.forward: one key per example through attend_rows (T = 1, C = 1, E = D, V = B)

@pytest.mark.parametrize("D,activation", [(24, "Dice"), (32, "tanh")])
def test_din_activation_layer_single_key(R, D, activation):
    B = 5
    assert DR.kernel_class(D, 1, 36, D)[3] == (D == 32)      # D = 32: 16-byte pieces with C = 1
    r = H.rng(D)
    layer = R.layers.DinActivationLayer(activation=activation, input_dim=D).cuda()
    dense, outl = layer.mlp_layer.layers[0], layer.output_layer
    kind, alpha, mean, var = layer.act_params()
    att = {"W1": H.glorot(r, 3 * D + D * D, 36), "b1": r.uniform(-0.1, 0.1, size=36).astype(np.float32),
           "W2": H.glorot(r, 36, 1), "b2": r.uniform(-0.1, 0.1, size=1).astype(np.float32),
           "act": {"kind": activation.lower()}}
    if activation == "Dice":
        att["act"].update(alpha=r.uniform(-0.2, 0.3, size=36).astype(np.float32),
                          mean=r.uniform(-0.1, 0.1, size=36).astype(np.float32),
                          var=r.uniform(0.5, 1.5, size=36).astype(np.float32))
    with torch.no_grad():
        for dst, src in ((dense.kernel, att["W1"]), (dense.bias, att["b1"]), (outl.kernel, att["W2"]),
                         (outl.bias, att["b2"])):
            dst.copy_(dev(src).reshape(dst.shape))
        if activation == "Dice":
            alpha.copy_(dev(att["act"]["alpha"])); mean.copy_(dev(att["act"]["mean"])); var.copy_(dev(att["act"]["var"]))
    v1, v2 = r.normal(size=(B, D)).astype(np.float32), r.uniform(-0.5, 0.5, size=(B, D)).astype(np.float32)
    g = r.normal(size=(B, 1)).astype(np.float32)
    ta = H.to_torch(att, torch.float64, True)
    q64, k64 = torch.from_numpy(v1).double().requires_grad_(), torch.from_numpy(v2).double().requires_grad_()
    want = T.din_activation_unit(q64, k64, ta)
    (want * torch.from_numpy(g).double()).sum().backward()
    qd, kd = dev(v1).requires_grad_(), dev(v2).requires_grad_()
    out = layer((qd, kd))
    assert tuple(out.shape) == (B, 1)
    (out * dev(g)).sum().backward()
    check(out, want.detach().numpy(), DR.OUT_TOL, "output")
    check(qd.grad, q64.grad.numpy(), DR.GRAD_TOL, "vec1")
    gk = kd.grad.to_dense() if kd.grad.is_sparse else kd.grad
    check(gk, k64.grad.numpy(), DR.GRAD_TOL, "vec2")
    check(dense.kernel.grad, ta["W1"].grad.numpy(), DR.GRAD_TOL, "W1")
    check(dense.bias.grad, ta["b1"].grad.numpy(), DR.GRAD_TOL, "b1")
    check(outl.kernel.grad, ta["W2"].grad.numpy(), DR.GRAD_TOL, "W2")
    check(outl.bias.grad.reshape(-1), ta["b2"].grad.numpy(), DR.GRAD_TOL, "b2")
    if activation == "Dice":
        check(alpha.grad, ta["act"]["alpha"].grad.numpy(), DR.GRAD_TOL, "alpha")
    # a non-leaf key tensor: the sparse gradient of the identity table flows on to what made the keys
    base = dev(v2).requires_grad_()
    layer((dev(v1), base * 2.0)).sum().backward()
    assert base.grad is not None and tuple(base.grad.shape) == (B, D)


# ---- the envelope: the corner the backward's LDS cannot hold is refused by both directions, before any work

@pytest.mark.parametrize("E,C", [(43, 3), (64, 3), (64, 4)])
@pytest.mark.parametrize("Hh", [49, 64])
def test_refused_corner_is_refused_in_both_directions_before_any_work(R, E, C, Hh):
    ops = R.ops
    D, B, T_, V = E * C, 2, 3, 11
    assert D in (129, 192, 256)
    with pytest.raises(ValueError):
        DR.kernel_class(E, C, Hh, E)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    args = (z(V, E), torch.ones((B, T_, C), dtype=torch.int64, device="cuda"), z(B, D * Hh + Hh), z(D, Hh),
            ops.DACT_SIGMOID, None, None, None, z(Hh), z(1), 0, 1)
    scores, gpooled = z(B, T_), z(B, D)
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]
    n0 = count()
    with pytest.raises(NotImplementedError) as fwd:
        ops.din_attn_fwd(*args)
    with pytest.raises(NotImplementedError) as bwd:
        ops.din_attn_bwd(*args, scores, gpooled)
    assert count() == n0                                     # nothing was allocated for either answer
    assert type(fwd.value) is type(bwd.value) and str(fwd.value) == str(bwd.value)
    # and the library itself, asked with the same live pointers, says the same in both directions and launches nothing
    L = R._lib
    p = lambda t: None if t is None else t.data_ptr()
    raw = (p(args[0]), E, V, E, C, p(args[1]), B, T_, p(args[2]), p(args[3]), Hh, args[4], None, None, None, p(args[8]),
           p(args[9]), 0, 1)
    out = [z(B, T_), z(B, D), z(B, T_, D), z(B, D * Hh + Hh), z(B, Hh), z(B, Hh), z(B, 1)]
    st = ops._stream()
    rc_f = L.lib.rec_din_attn_fwd_f32(*raw, p(out[0]), p(out[1]), None, st)
    rc_b = L.lib.rec_din_attn_bwd_f32(*raw, p(scores), p(gpooled), None, *(p(t) for t in out[2:]), st)
    assert rc_f == rc_b == L.LIMITS["REC_E_UNSUPPORTED"]
    with pytest.raises(NotImplementedError):
        L.check(rc_f, "rec_din_attn_fwd_f32")
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in out)     # no kernel wrote anything


def test_supported_corners_next_to_the_refused_one_are_cases():
    """(D = 256, H = 48) and (D = 128, H = 64) run in both directions and match the reference: they are rows of CASES."""
    shapes = {(c.E * c.C, c.H) for c in DR.CASES}
    assert (256, 48) in shapes and (128, 64) in shapes
