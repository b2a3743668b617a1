"""Shared test helpers: deterministic parameter builders used by oracle and GPU parity tests."""
import numpy as np


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def glorot(r, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return r.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


def det_table(V, E):
    """Hand-checkable table of SURVEY.md 8c: table[i,d] = ((i*31 + d*17) mod 97 - 48)/480."""
    i = np.arange(V, dtype=np.int64)[:, None]
    d = np.arange(E, dtype=np.int64)[None, :]
    return (((i * 31 + d * 17) % 97 - 48) / 480.0).astype(np.float32)


def deepfm_params(seed, V, F, E, mlp_dims=(32, 8), scale=0.05):
    r = rng(seed)
    dims = [F * E] + list(mlp_dims)
    return {
        "embed": r.uniform(-scale, scale, size=(V, E)).astype(np.float32),
        "w": r.uniform(-scale, scale, size=(V, 1)).astype(np.float32),
        "bias": r.uniform(-1, 1, size=(1,)).astype(np.float32),
        "k1": [glorot(r, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],
        "b1": [r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)],
        "k2": [glorot(r, dims[-1], 1)],
        "b2": [r.uniform(-0.1, 0.1, size=(1,)).astype(np.float32)],
    }


def tower_params(seed, V, F, E, mlp_dims=(64, 32), final_dim=8, scale=0.05):
    r = rng(seed)
    dims = [F * E] + list(mlp_dims)
    return {
        "embed": r.uniform(-scale, scale, size=(V, E)).astype(np.float32),
        "mlp_k": [glorot(r, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],
        "mlp_b": [r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)],
        "final_k": [glorot(r, dims[-1], final_dim)],
        "final_b": [r.uniform(-0.1, 0.1, size=(final_dim,)).astype(np.float32)],
    }


def dcn_params(seed, V, F, E, n_cont=3, units=(64, 8), layer_num=3, kind="vec"):
    r = rng(seed)
    D = n_cont + F * E
    dims = [D] + list(units)
    if kind == "vec":
        cw = [r.normal(0, 0.05, size=(D, 1)).astype(np.float32) for _ in range(layer_num)]
    else:
        cw = [r.normal(0, 0.05, size=(D, D)).astype(np.float32) for _ in range(layer_num)]
    return {
        "embed": r.uniform(-0.05, 0.05, size=(V, E)).astype(np.float32),
        "cross_w": cw,
        "cross_b": [r.normal(0, 0.02, size=(D, 1)).astype(np.float32) for _ in range(layer_num)],
        "dnn_k": [glorot(r, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],
        "dnn_b": [r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)],
        "out_k": glorot(r, D + units[-1], 1),
        "out_b": r.uniform(-0.1, 0.1, size=(1,)).astype(np.float32),
    }


def din_params(seed, V, E, n_user=5, n_item=3, act="dice", H=36, mlp_units=(200, 80)):
    r = rng(seed)
    D = n_item * E

    def mk_act(width):
        if act == "dice":
            return {"kind": "dice", "alpha": r.uniform(-0.2, 0.2, size=(width,)).astype(np.float32),
                    "mean": r.uniform(-0.1, 0.1, size=(width,)).astype(np.float32),
                    "var": r.uniform(0.5, 1.5, size=(width,)).astype(np.float32)}
        if act == "prelu":
            return {"kind": "prelu", "alpha": r.uniform(-0.2, 0.3, size=(width,)).astype(np.float32)}
        return {"kind": act}

    in_dim = (n_user + n_item) * E + D
    dims = [in_dim] + list(mlp_units)
    mlp = []
    for i in range(len(mlp_units)):
        mlp.append({"K": glorot(r, dims[i], dims[i + 1]),
                    "b": r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32),
                    "gamma": r.uniform(0.8, 1.2, size=(dims[i + 1],)).astype(np.float32),
                    "beta": r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32),
                    "act": mk_act(dims[i + 1])})
    return {
        "embed": r.uniform(-0.5, 0.5, size=(V, E)).astype(np.float32),
        "att": {"W1": glorot(r, 3 * D + D * D, H), "b1": r.uniform(-0.1, 0.1, size=(H,)).astype(np.float32),
                "act": mk_act(H), "W2": glorot(r, H, 1), "b2": r.uniform(-0.1, 0.1, size=(1,)).astype(np.float32)},
        "mlp": mlp,
        "out_k": glorot(r, dims[-1], 2),
        "out_b": r.uniform(-0.1, 0.1, size=(2,)).astype(np.float32),
    }


def nfm_params(seed, V, E, n_cont=3, units=(64, 8), scale=0.3):
    """NeuralFactorizationMachineLayer (3.DCN/CustomLayers.py:451-474): embed, BatchNormalization(E+n_cont), MLP."""
    r = rng(seed)
    n = E + n_cont
    dims = [n] + list(units)
    return {
        "embed": r.uniform(-scale, scale, size=(V, E)).astype(np.float32),
        "bn_gamma": r.uniform(0.5, 1.5, size=(n,)).astype(np.float32),
        "bn_beta": r.uniform(-0.2, 0.2, size=(n,)).astype(np.float32),
        "bn_mean": r.uniform(-0.1, 0.1, size=(n,)).astype(np.float32),
        "bn_var": r.uniform(0.5, 1.5, size=(n,)).astype(np.float32),
        "k1": [glorot(r, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],
        "b1": [r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)],
        "k2": [glorot(r, dims[-1], 1)],
        "b2": [r.uniform(-0.1, 0.1, size=(1,)).astype(np.float32)],
    }


def pnn_params(seed, V, F, E, mlp_dims=(32, 8), scale=0.3):
    """PNNLayer, method='inner' (2.FM/CustomLayers.py:705-727)."""
    r = rng(seed)
    dims = [F * E + F * (F - 1) // 2] + list(mlp_dims)
    return {
        "embed": r.uniform(-scale, scale, size=(V, E)).astype(np.float32),
        "k1": [glorot(r, dims[i], dims[i + 1]) for i in range(len(dims) - 1)],
        "b1": [r.uniform(-0.1, 0.1, size=(dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)],
        "k2": [glorot(r, dims[-1], 1)],
        "b2": [r.uniform(-0.1, 0.1, size=(1,)).astype(np.float32)],
    }


def to_torch(obj, dtype=None, requires_grad=False, device=None):
    import torch
    if isinstance(obj, dict):
        return {k: to_torch(v, dtype, requires_grad, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [to_torch(v, dtype, requires_grad, device) for v in obj]
    if isinstance(obj, np.ndarray):
        t = torch.from_numpy(obj.copy())
        if t.is_floating_point():
            if dtype is not None:
                t = t.to(dtype)
            if device is not None:
                t = t.to(device)
            t.requires_grad_(requires_grad)
        elif device is not None:
            t = t.to(device)
        return t
    return obj


# ------------------------------------------------------------------------------------------------
# batches with a prescribed de-duplication plan (tests/test_gpu_plan_edges.py)
# ------------------------------------------------------------------------------------------------
PLAN_LAYOUTS = ("scattered", "clustered", "hot", "ranked")


def field_offsets(dims):
    """DataGenerator id-space contract: field f owns [offsets[f], offsets[f] + dims[f]), offsets ascending."""
    return [int(x) for x in np.concatenate([[0], np.cumsum(dims[:-1])])] if len(dims) else []


def plan_batch(B, dims, offsets, spectra, layout="scattered", seed=0, ends=True):
    """A DeepFM batch whose columns have exactly the runs of equal ids the caller asks for.

    spectra[f] is either a sequence of run lengths summing to B (the multiset of the column's runs: one distinct key
    per run) or "uniform" (ids drawn uniformly from the field).  Keys are distinct and lie inside the field
    [offsets[f], offsets[f] + dims[f]); with ``ends`` (a bool, or one per column) key 0 and key dims[f]-1 are among
    them.  Layouts:
      scattered  runs get random keys, their members random examples;
      clustered  runs get random keys, the members of a run are adjacent examples;
      hot        the longest runs get the smallest keys (hot neighbours at the head of the sorted column), members
                 at random examples;
      ranked     spectra[f][u] is the length of the run of the u-th smallest key (places a run at a chosen plan
                 slot), members at random examples.
    Labels are Bernoulli(0.25) from the same seeded generator.  Returns {"f<i>": int64 [B,1], ..., "label": float32
    [B,1]}."""
    if layout not in PLAN_LAYOUTS:
        raise ValueError("layout must be one of %s" % (PLAN_LAYOUTS,))
    r = rng(seed)
    F = len(dims)
    if len(offsets) != F or len(spectra) != F:
        raise ValueError("one dim, offset and spectrum per column")
    ends_f = list(ends) if isinstance(ends, (list, tuple)) else [bool(ends)] * F
    out = {}
    for f in range(F):
        dim, off, spec = int(dims[f]), int(offsets[f]), spectra[f]
        if isinstance(spec, str):
            if spec != "uniform":
                raise ValueError("a spectrum is a list of run lengths or 'uniform'")
            keys = r.integers(0, dim, size=B, dtype=np.int64)
            if ends_f[f] and B >= 2:
                keys[r.choice(B, 2, replace=False)] = (0, dim - 1)
            out["f%d" % f] = (keys + off).reshape(B, 1)
            continue
        lens = np.asarray(spec, dtype=np.int64)
        n = lens.size
        if n == 0 or lens.min() < 1 or lens.sum() != B:
            raise ValueError("column %d: run lengths must be >= 1 and sum to B=%d" % (f, B))
        if n > dim:
            raise ValueError("column %d: %d runs need as many distinct keys, the field has %d" % (f, n, dim))
        # n distinct keys, ascending
        if ends_f[f] and n >= 2:
            inner = r.choice(dim - 2, n - 2, replace=False) + 1 if n > 2 else np.zeros(0, np.int64)
            keys = np.sort(np.concatenate([[0, dim - 1], inner]).astype(np.int64))
        elif ends_f[f]:
            keys = np.zeros(1, np.int64)
        else:
            keys = np.sort(r.choice(dim, n, replace=False).astype(np.int64))
        if layout == "hot":
            lens = np.sort(lens)[::-1]                       # longest run on the smallest key
        elif layout in ("scattered", "clustered"):
            lens = lens[r.permutation(n)]
        members = np.repeat(keys, lens)                      # run of keys[u] has lens[u] members
        if layout == "clustered":
            order = r.permutation(n)                         # runs in random example order, members adjacent
            col = np.concatenate([np.full(lens[u], keys[u], np.int64) for u in order])
        else:
            col = members[r.permutation(B)]
        out["f%d" % f] = (col + off).reshape(B, 1)
    out["label"] = (r.random((B, 1)) < 0.25).astype(np.float32)
    return out


def fill_spectrum(B, runs=(), pairs=0):
    """run lengths: the given runs, `pairs` runs of two, singles for the rest of the B examples"""
    runs = [int(x) for x in runs]
    rest = B - sum(runs) - 2 * pairs
    if rest < 0:
        raise ValueError("runs do not fit in B=%d" % B)
    return runs + [2] * pairs + [1] * rest


def host_plan(col, lo):
    """The de-duplication plan of one column as the sort defines it: perm = stable order of the keys (ids - lo),
    col_uid = the distinct ids ascending, col_seg = first sorted position of every run (then B up to index B),
    dloc[e] = run index of example e, sign bit set unless e is the first member of its run."""
    col = np.asarray(col, np.int64).reshape(-1)
    B = col.size
    perm = np.argsort(col - lo, kind="stable").astype(np.int32)
    uid, first, inv = np.unique(col, return_index=True, return_inverse=True)
    nu = uid.size
    seg = np.full(B + 1, B, np.int32)
    seg[:nu] = np.searchsorted(col[perm], uid, side="left")
    dloc = inv.astype(np.int64)
    head = np.zeros(B, bool)
    head[first] = True
    dloc = np.where(head, dloc, dloc | (1 << 31)).astype(np.uint32).view(np.int32)
    return dict(perm=perm, col_uid=uid, col_seg=seg, col_nu=nu, dloc=dloc)
