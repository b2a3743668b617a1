"""Restatements of GateNULayer / PosoForMLPLayer / PEPNetLayer (10.POSO/CustomLayers.py:76-119, 371-462) for the tests: an
fp64 numpy reading of both kernels (the EPNet lookup, the stacked POSO-MLPs) and of the whole layer with hand-written
gradients; a torch transcription in the reference's op order (one Sequential per gate, the loop over the layers as
written or chained, stop_gradient as .detach(), stack / flatten / concat) that autograd differentiates, runnable in fp32
and fp64 on the CPU; and the cases the host and GPU tests share.

Parameters are kept per sub-layer, as the reference holds them: a GateNU is a dict(A, a, Bm, bm); a tower is a list of
layers dict(W, b, C, A, a, Bm, bm); ``pack_epnet`` / ``pack_towers`` give the packed lists of include/mi355rec.h.  Scale
as in tests/mmoe_ref.py: glorot-uniform kernels, every bias N(0, 0.1^2), C = 1 + N(0, 0.1^2) (so that dC is not the
gradient at a special point), inputs N(0, 1), tables N(0, 0.5^2).  ``pre`` is, per example, the smallest |relu
pre-activation|: the EPNet hidden layers, every gate's hidden layer, and C d gate of every relu layer."""
import functools

import numpy as np
import torch

from tests.masknet_ref import PRE_EPS, _t, clean_seed, glorot, rel_err  # noqa: F401

EP_NAMES = ["A", "a", "Bm", "bm"]
PO_NAMES = ["Wg1", "bg1", "Wg2", "bg2", "W", "b", "C"]
PO_SAVED = ["h", "gate", "d", "a"]
DEFAULT_ACTS = ("relu", "relu", "sigmoid")

# (B, Dm, Dg, T, units, acts, m)
POSO_CASES = [(1, 1, 1, 1, (1,), ("sigmoid",), 1),
              (2, 15, 19, 3, (5, 3, 1), DEFAULT_ACTS, 2),
              (33, 72, 88, 3, (64, 16, 1), DEFAULT_ACTS, 2),
              (33, 72, 88, 3, (1,), ("sigmoid",), 2),
              (17, 72, 88, 1, (64, 16), ("relu", "relu"), 2),
              (17, 512, 512, 4, (128,), ("linear",), 4),
              (2049, 72, 88, 3, (64, 16, 1), DEFAULT_ACTS, 2)]
# (B, V, F, P, E, Hg, ids): ids 'uniform', 'zipf' (rows repeat) or 'equal' (every id the same)
EPNET_CASES = [(1, 3, 1, 1, 1, 1, "uniform"), (2, 50, 3, 2, 4, 5, "uniform"), (33, 1000, 9, 2, 8, 16, "uniform"),
               (2049, 1000, 9, 2, 8, 16, "zipf"), (17, 100, 26, 4, 16, 16, "uniform"), (33, 1000, 9, 2, 8, 16, "equal")]


def f32_exact(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_gate(r, din, hidden, out):
    return dict(A=glorot(r, din, hidden), a=r.normal(0, 0.1, hidden), Bm=glorot(r, hidden, out), bm=r.normal(0, 0.1, out))


def make_tower(r, dims_in, units, Dg, m):
    """layers of input widths dims_in[i]: the chained widths, or the main width for every layer (as written)"""
    out = []
    for k, u in zip(dims_in, units):
        lay = dict(W=glorot(r, k, u), b=r.normal(0, 0.1, u), C=np.float64(1 + r.normal(0, 0.1)))
        lay.update(make_gate(r, Dg, m * u, u))
        out.append(lay)
    return out


def exact(tree):
    if isinstance(tree, dict):
        return {k: exact(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [exact(v) for v in tree]
    return f32_exact(tree)


def pack_epnet(gates):
    return [np.stack([g[k] for g in gates]) for k in EP_NAMES]


def pack_towers(towers):
    """towers: T lists of the LIVE layers -> Wg1, bg1, Wg2, bg2, W, b, C of include/mi355rec.h"""
    lays = [lay for tw in towers for lay in tw]
    flat = lambda k: np.concatenate([np.asarray(lay[k], np.float64).reshape(-1) for lay in lays])
    return [np.concatenate([lay["A"] for lay in lays], axis=1), flat("a"), flat("Bm"), flat("bm"), flat("W"), flat("b"),
            np.array([[lay["C"] for lay in tw] for tw in towers], np.float64)]


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _act(z, act):
    return np.maximum(z, 0) if act == "relu" else (_sig(z) if act == "sigmoid" else z)


def _dact(z, act):
    if act == "relu":
        return (z > 0).astype(np.float64)
    if act == "sigmoid":
        s = _sig(z)
        return s * (1 - s)
    return np.ones_like(z)


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def gatenu_numpy(v, p):
    ph = v @ p["A"] + p["a"]
    h = np.maximum(ph, 0)
    return ph, h, 2 * _sig(h @ p["Bm"] + p["bm"])


def gatenu_bwd(v, p, ph, h, gate, dgate):
    """-> dv, dict of parameter gradients"""
    dpg = dgate * gate * (1 - gate / 2)
    dh = (dpg @ p["Bm"].T) * (ph > 0)
    return dh @ p["A"].T, dict(A=v.T @ dh, a=dh.sum(0), Bm=h.T @ dpg, bm=dpg.sum(0))


def poso_numpy(x, g, towers, acts, dout=None):
    """T chained POSO-MLPs over x [B, Dm] and g [B, Dg] -> out [B, T, U_last], the save buffers in the kernel's layout
    and pre; with dout [B, T, U_last] also dx, dg and dparams (packed, the order of PO_NAMES)."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    towers = [[{k: np.asarray(v, np.float64) for k, v in lay.items()} for lay in tw] for tw in towers]
    B = x.shape[0]
    pre = np.full(B, np.inf)
    keep, outs = [], []
    for tw in towers:
        inp, row = x, []
        for lay, act in zip(tw, acts):
            ph, h, gate = gatenu_numpy(g, lay)
            d = inp @ lay["W"] + lay["b"]
            z = lay["C"] * (d * gate)
            a = _act(z, act)
            pre = np.minimum(pre, np.abs(ph).min(1))
            if act == "relu":
                pre = np.minimum(pre, np.abs(z).min(1))
            row.append(dict(inp=inp, ph=ph, h=h, gate=gate, d=d, z=z, a=a))
            inp = a
        keep.append(row)
        outs.append(inp)
    cat = lambda k: np.concatenate([s[k] for row in keep for s in row], axis=1)
    res = dict(out=np.stack(outs, axis=1), pre=pre, h=cat("h"), gate=cat("gate"), d=cat("d"), a=cat("a"))
    if dout is None:
        return res
    dout = np.asarray(dout, np.float64)
    dx, dg, grads = np.zeros_like(x), np.zeros_like(g), []
    for t, (tw, row) in enumerate(zip(towers, keep)):
        da, gt = dout[:, t], []
        for i in reversed(range(len(tw))):
            lay, s = tw[i], row[i]
            dz = da * _dact(s["z"], acts[i])
            dd, dgate = dz * lay["C"] * s["gate"], dz * lay["C"] * s["d"]
            dgi, gp = gatenu_bwd(g, lay, s["ph"], s["h"], s["gate"], dgate)
            gp.update(W=s["inp"].T @ dd, b=dd.sum(0), C=(dz * s["d"] * s["gate"]).sum())
            dg += dgi
            da = dd @ lay["W"].T
            gt.insert(0, gp)
        dx += da
        grads.append(gt)
    res.update(dx=dx, dg=dg, dparams=pack_towers(grads), dtowers=grads)
    return res


def epnet_numpy(table, ids, F, gates, du=None):
    """ids [B, F + P] into table [V, E] -> u [B, (F + P) E] and pre; with du also drows [B, F + P, E], dparams (packed,
    the order of EP_NAMES), dgates and the dense dtable."""
    table = np.asarray(table, np.float64)
    gates = [{k: np.asarray(v, np.float64) for k, v in p.items()} for p in gates]
    B, E = ids.shape[0], table.shape[1]
    rows = table[ids]
    main, pp = rows[:, :F], rows[:, F:].reshape(B, -1)
    keep = [gatenu_numpy(pp, p) for p in gates]
    gate = np.stack([k[2] for k in keep], axis=1)
    u = np.concatenate([(gate * main).reshape(B, -1), pp], axis=1)
    pre = np.min([np.abs(k[0]).min(1) for k in keep], axis=0)
    res = dict(u=u, pre=pre, gate=gate)
    if du is None:
        return res
    du = np.asarray(du, np.float64)
    duc = du[:, :F * E].reshape(B, F, E)
    drows = np.zeros_like(rows)
    drows[:, :F] = duc * gate
    dpp, dgates = du[:, F * E:].copy(), []
    for f, (p, (ph, h, gt)) in enumerate(zip(gates, keep)):
        dv, gp = gatenu_bwd(pp, p, ph, h, gt, duc[:, f] * main[:, f])
        dpp += dv
        dgates.append(gp)
    drows[:, F:] = dpp.reshape(B, -1, E)
    dtable = np.zeros_like(table)
    np.add.at(dtable, ids.reshape(-1), drows.reshape(-1, E))
    res.update(drows=drows, dgates=dgates, dparams=pack_epnet(dgates), dtable=dtable)
    return res


def live(towers, chain):
    return [list(tw) if chain else tw[-1:] for tw in towers]


def layer_numpy(table, ids, F, gates, towers, chain, gout=None, acts=DEFAULT_ACTS):
    """The whole layer -> out [B, T, U_last], pre; with gout also dtable, dgates, dtowers (None for a layer without a
    gradient).  ``towers`` holds every layer of every tower, dead ones included."""
    E = np.shape(table)[1]
    ep = epnet_numpy(table, ids, F, gates)
    u = ep["u"]
    lv, la = live(towers, chain), list(acts) if chain else list(acts)[-1:]
    po = poso_numpy(u[:, :F * E], u, lv, la, gout)
    res = dict(out=po["out"], pre=np.minimum(ep["pre"], po["pre"]), u=u)
    if gout is None:
        return res
    du = po["dg"].copy()
    du[:, :F * E] = po["dx"]                     # stop_gradient: the gate path's share of c is dropped
    eb = epnet_numpy(table, ids, F, gates, du)
    dt = [gt if chain else [None] * (len(tw) - 1) + gt for tw, gt in zip(towers, po["dtowers"])]
    res.update(dtable=eb["dtable"], dgates=eb["dgates"], dtowers=dt, du=du, dx=po["dx"], dg=po["dg"])
    return res


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def gatenu_torch(v, p, saved=None):
    h = torch.relu(v @ p["A"] + p["a"])
    if saved is not None:
        saved.append(h)
    return 2 * torch.sigmoid(h @ p["Bm"] + p["bm"])


def _act_t(z, act):
    return torch.relu(z) if act == "relu" else (torch.sigmoid(z) if act == "sigmoid" else z)


def poso_torch(main, gate_in, tower, acts, chain, saved=None):
    """PosoForMLPLayer.call.  As written (chain False) every layer reads ``main`` and only the last ``inputs`` is
    returned; chained, layer i reads layer i-1's activation."""
    inputs = None
    for i, (lay, act) in enumerate(zip(tower, acts)):
        hs = [] if saved is not None else None
        dense_output = (inputs if chain and i > 0 else main) @ lay["W"] + lay["b"]
        gate_output = gatenu_torch(gate_in, lay, hs)
        layer_output = dense_output * gate_output
        layer_output = lay["C"] * layer_output
        inputs = _act_t(layer_output, act)
        if saved is not None:
            saved.append(dict(h=hs[0], gate=gate_output, d=dense_output, a=inputs))
    return inputs


def pepnet_torch(table, Xc, Xpp, gates, towers, chain, acts=DEFAULT_ACTS):
    """PEPNetLayer.call: one table; the EPNet input is gathered from the ppnet ids a second time."""
    main_input = table[Xc]
    ppnet_input = table[Xpp].flatten(1)
    epnet_input = table[Xpp].flatten(1)
    epnet_output = torch.stack([gatenu_torch(epnet_input, p) for p in gates], dim=1)
    posoed_embedding = epnet_output * main_input
    concated_embedding = posoed_embedding.flatten(1)
    main_for_ppnet = concated_embedding.detach()
    ppnet_input = torch.cat([main_for_ppnet, ppnet_input], dim=1)
    outs = [poso_torch(concated_embedding, ppnet_input, tw, acts, chain) for tw in towers]
    return torch.stack(outs, dim=1)


def _tree_t(tree, dtype):
    if isinstance(tree, dict):
        return {k: _tree_t(v, dtype) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_tree_t(v, dtype) for v in tree]
    return _t(tree, dtype, True)


def _tree_grad(tree):
    if isinstance(tree, dict):
        return {k: _tree_grad(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_tree_grad(v) for v in tree]
    return None if tree.grad is None else tree.grad.detach().double().numpy()


_n64 = lambda t: t.detach().double().numpy()


def poso_torch_grads(x, g, towers, acts, dout, dtype):
    """the standalone kernel's case, chained -> (out, dx, dg, dparams packed, saved) as fp64 numpy"""
    xt, gt, tt = _t(x, dtype, True), _t(g, dtype, True), _tree_t(towers, dtype)
    saved = []
    out = torch.stack([poso_torch(xt, gt, tw, acts, True, saved) for tw in tt], dim=1)
    out.backward(_t(dout, dtype))
    sv = {k: np.concatenate([_n64(s[k]) for s in saved], axis=1) for k in PO_SAVED}
    return _n64(out), _n64(xt.grad), _n64(gt.grad), pack_towers(_tree_grad(tt)), sv


def epnet_torch_grads(table, ids, F, gates, du, dtype):
    """the lookup kernel's case -> (u, dtable, dparams packed) as fp64 numpy"""
    tt, gt = _t(table, dtype, True), _tree_t(gates, dtype)
    X = torch.from_numpy(np.asarray(ids, np.int64))
    pp = tt[X[:, F:]].flatten(1)
    gate = torch.stack([gatenu_torch(pp, p) for p in gt], dim=1)
    u = torch.cat([(gate * tt[X[:, :F]]).flatten(1), pp], dim=1)
    u.backward(_t(du, dtype))
    return _n64(u), _n64(tt.grad), pack_epnet(_tree_grad(gt))


def layer_torch_grads(table, ids, F, gates, towers, chain, gout, dtype, acts=DEFAULT_ACTS):
    """-> (out [B, T, U_last], dtable, dgates, dtowers) as fp64 numpy; a parameter without a gradient gives None"""
    tt, gt, tw = _t(table, dtype, True), _tree_t(gates, dtype), _tree_t(towers, dtype)
    X = torch.from_numpy(np.asarray(ids, np.int64))
    out = pepnet_torch(tt, X[:, :F], X[:, F:], gt, tw, chain, acts)
    out.backward(_t(gout, dtype))
    return _n64(out), _n64(tt.grad), _tree_grad(gt), _tree_grad(tw)


def state_dict_of(table, gates, towers):
    """-> {state-dict name of PEPNetLayer: array or None}"""
    out = {"embedding_layer.embeddings": table}

    def gate_names(pre, p):
        out.update({pre + "gate.layers.0.kernel": p["A"], pre + "gate.layers.0.bias": p["a"],
                    pre + "gate.layers.1.kernel": p["Bm"], pre + "gate.layers.1.bias": p["bm"]})

    for f, p in enumerate(gates):
        gate_names("poso_gate_for_embedding.%d." % f, p)
    for t, tw in enumerate(towers):
        for i, lay in enumerate(tw):
            pre = "poso_mlp_layers.%d." % t
            lay = lay if lay is not None else dict.fromkeys(("W", "b", "C", "A", "a", "Bm", "bm"))
            out.update({pre + "dense_layers.%d.kernel" % i: lay["W"], pre + "dense_layers.%d.bias" % i: lay["b"],
                        pre + "C_list.%d" % i: lay["C"]})
            gate_names(pre + "gates.%d." % i, lay)
    return out


# ---- the cases of the host and GPU tests ----------------------------------------------------------------------------
def _gen_poso(case, seed):
    B, Dm, Dg, T, units, acts, m = case
    r = np.random.default_rng(seed)
    towers = exact([make_tower(r, [Dm] + list(units[:-1]), units, Dg, m) for _ in range(T)])
    return r, towers, f32_exact(r.normal(0, 1, (B, Dm))), f32_exact(r.normal(0, 1, (B, Dg)))


@functools.lru_cache(maxsize=None)
def poso_case(*case):
    """-> dict(towers, params (packed), x, g, dout, ref, near, seed): fp32-exact inputs, the fp64 reading, the near-kink
    examples (their dout rows are zero).  Under 100 examples the first seed 1, 2, 3, ... without one."""
    B, T, units, acts = case[0], case[3], case[4], case[5]

    def near_of(s):
        _, towers, x, g = _gen_poso(case, s)
        return poso_numpy(x, g, towers, acts)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, towers, x, g = _gen_poso(case, seed)
    near = near_of(seed)
    dout = f32_exact(r.uniform(-1, 1, (B, T, units[-1])))
    dout[near] = 0.0
    return dict(towers=towers, params=pack_towers(towers), x=x, g=g, dout=dout, near=near, seed=seed,
                ref=poso_numpy(x, g, towers, acts, dout))


@functools.lru_cache(maxsize=None)
def poso_case_t32(*case):
    c = poso_case(*case)
    return poso_torch_grads(c["x"], c["g"], c["towers"], case[5], c["dout"], torch.float32)


def make_ids(r, B, V, n, kind):
    if kind == "zipf":
        return ((r.zipf(1.3, (B, n)) - 1) % V).astype(np.int64)
    if kind == "equal":
        return np.full((B, n), int(r.integers(0, V)), np.int64)
    return r.integers(0, V, (B, n)).astype(np.int64)


def _gen_epnet(case, seed):
    B, V, F, P, E, Hg, kind = case
    r = np.random.default_rng(seed)
    gates = exact([make_gate(r, P * E, Hg, E) for _ in range(F)])
    return r, gates, f32_exact(r.normal(0, 0.5, (V, E))), make_ids(r, B, V, F + P, kind)


@functools.lru_cache(maxsize=None)
def epnet_case(*case):
    B, V, F, P, E, Hg, kind = case

    def near_of(s):
        _, gates, table, ids = _gen_epnet(case, s)
        return epnet_numpy(table, ids, F, gates)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, gates, table, ids = _gen_epnet(case, seed)
    near = near_of(seed)
    du = f32_exact(r.uniform(-1, 1, (B, (F + P) * E)))
    du[near] = 0.0
    return dict(gates=gates, params=pack_epnet(gates), table=table, ids=ids, du=du, near=near, seed=seed,
                ref=epnet_numpy(table, ids, F, gates, du))


@functools.lru_cache(maxsize=None)
def epnet_case_t32(*case):
    c = epnet_case(*case)
    return epnet_torch_grads(c["table"], c["ids"], case[2], c["gates"], c["du"], torch.float32)


LAYER_B, LAYER_V, LAYER_F, LAYER_P, LAYER_E, LAYER_HG, LAYER_T, LAYER_UNITS = 32, 1000, 9, 2, 8, 16, 3, (64, 16, 1)


def _gen_layer(chain, seed, B=LAYER_B, kind="uniform"):
    r = np.random.default_rng(seed)
    F, P, E = LAYER_F, LAYER_P, LAYER_E
    table = f32_exact(r.normal(0, 0.5, (LAYER_V, E)))
    gates = exact([make_gate(r, P * E, LAYER_HG, E) for _ in range(F)])
    dims = [F * E] + (list(LAYER_UNITS[:-1]) if chain else [F * E] * (len(LAYER_UNITS) - 1))
    towers = exact([make_tower(r, dims, LAYER_UNITS, (F + P) * E, 2) for _ in range(LAYER_T)])
    return r, table, make_ids(r, B, LAYER_V, F + P, kind), gates, towers


@functools.lru_cache(maxsize=None)
def layer_case(chain, B=LAYER_B):
    """the default layer at B examples: a seed without a near-kink example under 100 examples, seed 1 above"""
    def near_of(s):
        _, table, ids, gates, towers = _gen_layer(chain, s, B)
        return layer_numpy(table, ids, LAYER_F, gates, towers, chain)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, table, ids, gates, towers = _gen_layer(chain, seed, B)
    near = near_of(seed)
    gout = f32_exact(r.uniform(-1, 1, (B, LAYER_T, LAYER_UNITS[-1])))
    gout[near] = 0.0
    return dict(table=table, ids=ids, gates=gates, towers=towers, gout=gout, near=near, seed=seed)
