"""GPU tests of engine.DSSMFusedStep (csrc/dssm_fused.hip): the fused DSSM two-tower train step against the reference-pinned
ckpt-7 vectors, the fp64 oracle (T.dssm_tower / T.two_tower_score / T.keras_bce) at config D's widths, the autograd
path replayed by GraphedTrainStep, itself (graph replay vs eager, fresh steps: bit for bit), batch tails, out-of-range
ids, tables above 4 GiB, and the touched-rows Adam."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests import helpers as H

pytestmark = pytest.mark.gpu

UN, IN = ["user_tag1", "user_tag2"], ["item_tag1", "item_tag2", "item_tag3"]
DENSE = ["mlp.kernel_0", "mlp.bias_0", "mlp.kernel_1", "mlp.bias_1", "final.kernel_0", "final.bias_0"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_layer(Vu, Vi, E, seed=5):
    from explicit_tf2_recommendation_amd import layers
    layer = layers.DSSMTwoTowerRetrievalLayer(u_feature_names=UN, i_feature_names=IN, u_feature_dims=Vu,
                                              i_feature_dims=Vi, u_embedding_dims=E, i_embedding_dims=E).cuda()
    pu, pi = H.tower_params(seed, Vu, 2, E), H.tower_params(seed + 1, Vi, 3, E)
    sd = dict(layer.named_parameters())
    with torch.no_grad():
        for t, p in (("u_tower", pu), ("i_tower", pi)):
            vals = [p["embed"], p["mlp_k"][0], p["mlp_b"][0], p["mlp_k"][1], p["mlp_b"][1], p["final_k"][0],
                    p["final_b"][0]]
            for n, v in zip(["embed.embeddings"] + DENSE, vals):
                sd[t + "." + n].copy_(torch.from_numpy(v))
    return layer


def make_batch(seed, B, Vu, Vi, dist="uniform"):
    r = H.rng(seed)

    def ids(V):
        if dist == "zipf":
            return (r.zipf(1.2, size=B) - 1) % V
        return r.integers(0, V, size=B)
    b = {n: ids(Vu).astype(np.int64) for n in UN}
    b.update({n: ids(Vi).astype(np.int64) for n in IN})
    b["label"] = (r.uniform(size=(B, 1)) < 0.3).astype(np.float32)
    return b


def avoid_kinks(layer, batch, seed, margin=2e-5):
    """Redraw the ids of the examples whose fp64 hidden pre-activations lie within `margin` of the ReLU kink: there the
    sign an fp32 evaluation sees is a matter of rounding, and so is the gradient (any fp32 implementation, autograd's
    included)."""
    r = H.rng(seed)
    sd = {k: v.detach().cpu().double() for k, v in layer.named_parameters()}
    B = batch["label"].shape[0]
    for _ in range(20):
        amb = np.zeros(B, bool)
        for t, names in (("u_tower", UN), ("i_tower", IN)):
            X = torch.from_numpy(np.stack([batch[n].reshape(-1) for n in names], axis=1))
            z1 = sd[t + ".embed.embeddings"][X].flatten(1) @ sd[t + ".mlp.kernel_0"] + sd[t + ".mlp.bias_0"]
            z2 = torch.relu(z1) @ sd[t + ".mlp.kernel_1"] + sd[t + ".mlp.bias_1"]
            amb |= ((z1.abs() < margin).any(1) | (z2.abs() < margin).any(1)).numpy()
        if not amb.any():
            return batch
        for t, names in (("u_tower", UN), ("i_tower", IN)):
            V = sd[t + ".embed.embeddings"].shape[0]
            for n in names:
                batch[n][amb] = r.integers(0, V, size=int(amb.sum()))
    raise AssertionError("could not move the batch off the ReLU kinks")


def to_dev(b):
    return {k: dev(v) for k, v in b.items()}


def oracle(layer, batch):
    """fp64 oracle on the rows the batch touches: loss, per-parameter gradients (tables: (uniq ids, rows)), outputs."""
    sd = {k: v.detach().cpu().double() for k, v in layer.named_parameters()}
    res, towers = {}, {}
    for t, names in (("u_tower", UN), ("i_tower", IN)):
        X = np.stack([batch[n].reshape(-1) for n in names], axis=1)
        uniq, inv = np.unique(X, return_inverse=True)
        p = {"embed": sd[t + ".embed.embeddings"][torch.from_numpy(uniq)].clone().requires_grad_(),
             "mlp_k": [sd[t + ".mlp.kernel_0"].clone().requires_grad_(), sd[t + ".mlp.kernel_1"].clone().requires_grad_()],
             "mlp_b": [sd[t + ".mlp.bias_0"].clone().requires_grad_(), sd[t + ".mlp.bias_1"].clone().requires_grad_()],
             "final_k": [sd[t + ".final.kernel_0"].clone().requires_grad_()],
             "final_b": [sd[t + ".final.bias_0"].clone().requires_grad_()]}
        towers[t] = (p, uniq, T.dssm_tower(p, torch.from_numpy(inv.reshape(X.shape))))
    s = T.two_tower_score(towers["u_tower"][2], towers["i_tower"][2])
    loss = T.keras_bce(torch.from_numpy(batch["label"]).double(), s)
    loss.backward()
    for t, (p, uniq, out) in towers.items():
        res[t + ".embed.embeddings"] = (uniq, p["embed"].grad.numpy())
        for n, q in zip(DENSE, [p["mlp_k"][0], p["mlp_b"][0], p["mlp_k"][1], p["mlp_b"][1], p["final_k"][0],
                                p["final_b"][0]]):
            res[t + "." + n] = q.grad.numpy()
    return loss.item(), res, towers["u_tower"][2].detach().numpy(), towers["i_tower"][2].detach().numpy(), \
        s.detach().numpy()


def check_against_oracle(step, layer, batch, tol=2e-5):
    loss, ref, u, i, s = oracle(layer, batch)
    assert abs(step.loss.item() - loss) <= 1e-5, (step.loss.item(), loss)
    g = step.gradients()
    for name, want in ref.items():
        if name.endswith("embed.embeddings"):
            uniq, rows = want
            ids, got, nu = g[name]
            nu = int(nu.item())
            assert nu == uniq.size
            assert np.array_equal(ids.cpu().numpy()[:nu], uniq)
            assert rel(got.cpu().numpy()[:nu], rows) <= tol, name
            assert not got[nu:].any()
        else:
            assert rel(g[name].cpu().numpy(), want) <= tol, name
    if step.outputs is not None:
        assert np.abs(step.outputs["user_embedding"].cpu().numpy() - u).max() <= 1e-5
        assert np.abs(step.outputs["item_embedding"].cpu().numpy() - i).max() <= 1e-5
        assert np.abs(step.outputs["score"].cpu().numpy() - s).max() <= 1e-5


def test_reference_pinned_ckpt7_vectors(golden_dir):
    """ckpt-7 weights (E = 8): the 54 user rows paired cyclically with the 256 item rows -> the embeddings of
    ebd_result/{user,item}_embedding.json."""
    from explicit_tf2_recommendation_amd import engine, layers
    k = np.load(os.path.join(golden_dir, "dssm_ckpt7_kat.npz"))
    V = int(k["vocab"][0])
    layer = layers.DSSMTwoTowerRetrievalLayer(u_feature_names=UN, i_feature_names=IN, u_feature_dims=V,
                                              i_feature_dims=V).cuda()
    sd = dict(layer.named_parameters())
    with torch.no_grad():
        for t, x in (("u_tower", "u"), ("i_tower", "i")):
            emb = np.zeros((V, 8), np.float32)
            emb[k[x + "_embed_row_ids"]] = k[x + "_embed_rows"]
            sd[t + ".embed.embeddings"].copy_(torch.from_numpy(emb))
            for n, key in zip(DENSE, ["_k0", "_b0", "_k1", "_b1", "_kf", "_bf"]):
                sd[t + "." + n].copy_(torch.from_numpy(k[x + key]))
    B = 256
    uidx = np.arange(B) % 54
    batch = {n: k["u_ids"][uidx, j].copy() for j, n in enumerate(UN)}
    batch.update({n: k["i_ids"][:, j].copy() for j, n in enumerate(IN)})
    batch["label"] = (H.rng(3).uniform(size=(B, 1)) < 0.5).astype(np.float32)
    step = engine.DSSMFusedStep(layer, B, use_graph=False, want_outputs=True)
    step(to_dev(batch))
    step.check_flags()
    assert np.abs(step.outputs["user_embedding"].cpu().numpy() - k["u_expected"][uidx]).max() <= 1e-5
    assert np.abs(step.outputs["item_embedding"].cpu().numpy() - k["i_expected"]).max() <= 1e-5
    check_against_oracle(step, layer, batch)


@pytest.mark.parametrize("B", [4096, 8192])
@pytest.mark.parametrize("dist", ["zipf", "uniform"])
def test_config_d_widths_against_oracle(B, dist):
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi = 20_011, 300_007
    layer = make_layer(Vu, Vi, 64)
    batch = avoid_kinks(layer, make_batch(11, B, Vu, Vi, dist), 12)
    step = engine.DSSMFusedStep(layer, B, want_outputs=True)
    step(to_dev(batch))
    step.check_flags()
    check_against_oracle(step, layer, batch)


def test_agrees_with_graphed_train_step():
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi, B = 3000, 7000, 1024
    layer = make_layer(Vu, Vi, 16)
    batch = to_dev(avoid_kinks(layer, make_batch(12, B, Vu, Vi, "zipf"), 13))
    step = engine.DSSMFusedStep(layer, B)
    loss = step(batch).item()
    gstep = engine.GraphedTrainStep(layer, batch)
    ref_loss = gstep(batch).item()
    assert abs(loss - ref_loss) <= 1e-5
    g = step.gradients()
    for name, p in layer.named_parameters():
        want = p.grad.to_dense() if p.grad.is_sparse else p.grad
        want = want.cpu().numpy()
        if name.endswith("embed.embeddings"):
            ids, rows, nu = g[name]
            nu = int(nu.item())
            ids = ids.cpu().numpy()[:nu]
            assert not np.delete(want, ids, axis=0).any()
            assert rel(rows.cpu().numpy()[:nu], want[ids]) <= 2e-5, name
        else:
            assert rel(g[name].cpu().numpy(), want) <= 2e-5, name


def _snapshot(step):
    g = step.gradients()
    out = [step.loss_steps.clone()]
    for name in sorted(g):
        v = g[name]
        out += [x.clone() for x in v] if isinstance(v, tuple) else [v.clone()]
    return out


def test_graph_replay_equals_eager_bit_for_bit():
    """Alternating cycles A -> B -> A ... with then= announcements: the graphed step enqueues eagerly, captures on the
    second sighting and replays from the third; after every call its losses and gradients equal, bit for bit, those of
    an eager step on the same inputs."""
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi, B = 2000, 5000, 512
    layer = make_layer(Vu, Vi, 32)
    A = [to_dev(make_batch(20 + j, B, Vu, Vi, "zipf")) for j in range(3)]
    Bb = [to_dev(make_batch(30 + j, B, Vu, Vi)) for j in range(3)]
    graphed = engine.DSSMFusedStep(layer, B, use_graph=True)
    eager = engine.DSSMFusedStep(layer, B, use_graph=False)
    for c in range(8):
        cur, nxt = (A, Bb) if c % 2 == 0 else (Bb, A)
        graphed.many(cur, then=nxt)
        eager.many(cur, then=nxt)
        for x, y in zip(_snapshot(graphed), _snapshot(eager)):
            assert torch.equal(x, y), c
    assert len(graphed._graphs) >= 1
    # two fresh steps on the same inputs
    s1 = engine.DSSMFusedStep(layer, B, use_graph=False)
    s2 = engine.DSSMFusedStep(layer, B, use_graph=False)
    s1(A[0])
    s2(A[0])
    for x, y in zip(_snapshot(s1), _snapshot(s2)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("B", [1, 1000])
def test_batch_tails(B):
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi = 500, 900
    layer = make_layer(Vu, Vi, 16)
    batch = avoid_kinks(layer, make_batch(40, B, Vu, Vi), 41)
    batch["label"][0] = 1.0
    step = engine.DSSMFusedStep(layer, B, use_graph=False, want_outputs=True)
    step(to_dev(batch))
    check_against_oracle(step, layer, batch)


def test_out_of_range_ids_flag_and_do_not_fault():
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi, B = 400, 800, 256
    layer = make_layer(Vu, Vi, 8)
    batch = make_batch(50, B, Vu, Vi)
    bad = np.zeros(B, bool)
    bad[[3, 77, 200]] = True
    batch["user_tag2"][3] = Vu + 5
    batch["item_tag1"][77] = -1
    batch["item_tag3"][200] = 1 << 40
    step = engine.DSSMFusedStep(layer, B, use_graph=False, want_outputs=True)
    step(to_dev(batch))
    with pytest.raises(IndexError):
        step.check_flags()
    torch.cuda.synchronize()
    clean = {k: v.copy() for k, v in batch.items()}
    for n, V in (("user_tag2", Vu), ("item_tag1", Vi), ("item_tag3", Vi)):
        clean[n] = np.clip(clean[n], 0, V - 1)
    _, _, u, i, s = oracle(layer, clean)
    ok = ~bad
    assert np.abs(step.outputs["user_embedding"].cpu().numpy()[ok] - u[ok]).max() <= 1e-5
    assert np.abs(step.outputs["item_embedding"].cpu().numpy()[ok] - i[ok]).max() <= 1e-5
    assert np.abs(step.outputs["score"].cpu().numpy()[ok] - s[ok]).max() <= 1e-5


def _hash_rows(ids, E):
    r = ids.reshape(-1, 1).to(torch.int64)
    c = torch.arange(E, device=ids.device, dtype=torch.int64).reshape(1, -1)
    return (((r * 2654435761 + c * 40503 + 12345) % 1000003).to(torch.float32) / 1000003.0) - 0.5


def test_item_table_above_4gib():
    """A 20M x 64 item table (5.1 GB) with ids near the top: the step against the oracle on the gathered rows."""
    from explicit_tf2_recommendation_amd import engine
    Vu, Vi, E, B = 1000, 20_000_000, 64, 512
    layer = make_layer(Vu, 1000, E)
    big = torch.empty((Vi, E), device="cuda")
    for lo in range(0, Vi, 5_000_000):
        big[lo:lo + 5_000_000] = _hash_rows(torch.arange(lo, min(Vi, lo + 5_000_000), device="cuda"), E)
    layer.i_tower.embed.embeddings = torch.nn.Parameter(big)
    batch = make_batch(60, B, Vu, 1000)
    r = H.rng(61)
    for n in IN:
        batch[n] = Vi - 1 - r.integers(0, 3_000_000, size=B)
    batch["item_tag1"][0] = Vi - 1
    assert (batch["item_tag2"].max() * 4 * E) > (4 << 30)
    step = engine.DSSMFusedStep(layer, B, use_graph=False, want_outputs=True)
    step(to_dev(batch))
    step.check_flags()
    # the oracle sees a compact copy of the touched item rows (ids remapped)
    X = np.stack([batch[n] for n in IN], axis=1)
    uniq, inv = np.unique(X, return_inverse=True)
    from explicit_tf2_recommendation_amd import layers
    small = make_layer(Vu, uniq.size, E)
    with torch.no_grad():
        for (n, p), (_, q) in zip(small.named_parameters(), layer.named_parameters()):
            if n != "i_tower.embed.embeddings":
                p.copy_(q)
        small.i_tower.embed.embeddings.copy_(_hash_rows(torch.from_numpy(uniq).cuda(), E))
    sb = dict(batch)
    for j, n in enumerate(IN):
        sb[n] = inv.reshape(X.shape)[:, j].astype(np.int64)
    loss, ref, u, i, s = oracle(small, sb)
    assert abs(step.loss.item() - loss) <= 1e-5
    ids, rows, nu = step.gradients()["i_tower.embed.embeddings"]
    nu = int(nu.item())
    assert np.array_equal(ids.cpu().numpy()[:nu], uniq)
    assert rel(rows.cpu().numpy()[:nu], ref["i_tower.embed.embeddings"][1]) <= 2e-5
    assert np.abs(step.outputs["item_embedding"].cpu().numpy() - i).max() <= 1e-5
    assert rel(step.gradients()["i_tower.mlp.kernel_0"].cpu().numpy(), ref["i_tower.mlp.kernel_0"]) <= 2e-5
    del step, layer, big
    torch.cuda.empty_cache()


def test_lazy_adam_matches_touched_rows_restatement():
    """5 steps of optimizer='lazy_adam' against a restatement of touched-rows Adam (tables) / Adam (dense) in fp64 with
    Keras' eps, applied to the gradients each step reports; rows no batch touched stay unchanged."""
    from explicit_tf2_recommendation_amd import engine
    from explicit_tf2_recommendation_amd._lib import lib
    Vu, Vi, B, lr = 600, 1500, 256, 1e-2
    layer = make_layer(Vu, Vi, 16)
    init = {n: p.detach().cpu().numpy().copy() for n, p in layer.named_parameters()}
    batches = [to_dev(make_batch(70 + j, B, Vu, Vi, "zipf")) for j in range(5)]
    step = engine.DSSMFusedStep(layer, B, optimizer="lazy_adam", lr=lr)
    P = {n: v.astype(np.float64) for n, v in init.items()}
    M = {n: np.zeros_like(v) for n, v in P.items()}
    Vv = {n: np.zeros_like(v) for n, v in P.items()}
    touched = {"u_tower.embed.embeddings": set(), "i_tower.embed.embeddings": set()}
    # the constants as the kernels hold them (fp32: 1 - 0.999f is 1.3e-5 away from 0.001)
    f = np.float32
    b1, b2, c1, c2, eps = float(f(0.9)), float(f(0.999)), float(f(1) - f(0.9)), float(f(1) - f(0.999)), float(f(1e-7))
    for t, b in enumerate(batches, start=1):
        step(b, next_inputs=batches[t] if t < len(batches) else None)
        g = step.gradients()
        lr_t = lib.rec_adam_lr_t_f32(lr, 0.9, 0.999, t)
        for n in P:
            if n.endswith("embed.embeddings"):
                ids, rows, nu = g[n]
                nu = int(nu.item())
                idx = ids.cpu().numpy()[:nu]
                gr = rows.cpu().numpy()[:nu].astype(np.float64)
                touched[n].update(idx.tolist())
                M[n][idx] = b1 * M[n][idx] + c1 * gr
                Vv[n][idx] = b2 * Vv[n][idx] + c2 * gr * gr
                P[n][idx] -= lr_t * M[n][idx] / (np.sqrt(Vv[n][idx]) + eps)
            else:
                gd = g[n].cpu().numpy().astype(np.float64)
                M[n] = M[n] + (gd - M[n]) * c1
                Vv[n] = Vv[n] + (gd * gd - Vv[n]) * c2
                P[n] -= lr_t * M[n] / (np.sqrt(Vv[n]) + eps)
    assert int(step._step_dev.item()) == 5
    for n, p in layer.named_parameters():
        got = p.detach().cpu().numpy()
        if n.endswith("embed.embeddings"):
            tidx = np.array(sorted(touched[n]))
            assert rel(got[tidx], P[n][tidx]) <= 1e-6, n
            rest = np.setdiff1d(np.arange(got.shape[0]), tidx)
            assert rest.size > 0 and np.array_equal(got[rest], init[n][rest])
        else:
            assert rel(got, P[n]) <= 1e-6, n
