"""What the ETA tests share (not a test file): the numpy reading of the SimHash search (7.SIM/CustomLayers.py:556-571) as
include/mi355rec.h defines it -- TensorFlow cannot be imported here -- the torch-CPU transcription of the whole ETALayer
(:518-626) parametrised by dtype, the inputs of a case from a fixed seed and the case lists.

The search: tri-state codes sign(x H) from fp64 projections (NaN equals nothing), the integer count of equal code bits,
a padded step (first id column == padding_index) ranked as -inf, and a stable descending order -- the lower index first
among equals, tf.argsort(direction='DESCENDING').  An id outside [0, V) reads a zero row.

The sign of an fp32 sum is only comparable with the sign of the fp64 sum when it is decided, so there are two kinds of
input:
  exact   table values in {-8..8}/8 and H in {-4..4}/4: every product is a multiple of 1/32 below 1 and every partial sum
          of at most 256 of them a multiple of 1/32 below 256, exact in fp32 in any order.  The kernel must equal this
          file bit for bit.  A few projections in a hundred are exactly zero, and the rows draw their steps from a small
          pool, so zero codes and ties are the normal case.
  random  table U(-0.05, 0.05), H N(0, 0.05).  A projection is DECIDED when |p64| > 2 D 2^-24 sum_d |x_d H_dj|, the
          worst-case error of an fp32 dot product of D terms in any order (each of the D products and D sums rounds once,
          relative 2^-24, of a partial sum bounded by sum |x_d H_dj|).  An example with an undecided projection in its
          item or in any valid step is left out of the comparison; `undecided` returns the mask and the tests assert
          that it covers at most MAX_LEFT_OUT of the examples.
"""
import numpy as np
import torch

from tests import sim_ref as SR

F32, F64 = np.float32, np.float64
V_CASE = 200
POOL = 5                        # distinct steps a row draws its series from: repeats (exact ties) are the normal case
ZERO_ROW, NAN_ROW = 5, 9        # table rows the generators zero / the NaN test fills with NaN
MAX_LEFT_OUT = 0.10
rel_err = SR.rel_err

# (B, T, C, E, m, k): D = C E, K = min(k, T).  The reference's __main__ shape first; T on both sides of the 64-lane wave
# and of the 256-thread workgroup; m at 1, 16 | 17.., 31, 32 (the 16- and 32-column kernels); K at 1, 3, 16 and T; E at 1
# and 2 (scalar row loads), 4 and 12 (one 16-byte load), 16, 48, 64 (four), 22 and 85 (odd strides); D at 2 .. 256
REFERENCE = (3, 10, 3, 16, 16, 3)
CASES = (REFERENCE, (5, 1, 1, 2, 1, 1), (6, 10, 3, 2, 17, 10), (6, 63, 3, 16, 16, 16), (6, 64, 1, 48, 31, 3),
         (6, 65, 3, 22, 32, 1), (5, 257, 1, 64, 16, 16), (5, 257, 3, 85, 32, 3), (5, 65, 1, 256, 32, 16),
         (6, 20, 3, 4, 8, 3), (6, 9, 1, 12, 16, 4), (7, 300, 3, 1, 5, 3))
# random inputs: large batches, so that the share left out is a share; seeds for which this file alone stays under the cap
RANDOM_CASES = ((256, 64, 3, 16, 16, 3), (256, 65, 1, 48, 32, 16), (128, 257, 3, 4, 31, 1))


def dims(case):
    B, T, C, E, m, k = case
    return B, T, C, E, m, min(k, T), C * E


def lookup(table, ids):
    """table[ids] with a zero row for an id outside [0, V)"""
    ids = np.asarray(ids)
    ok = (ids >= 0) & (ids < table.shape[0])
    return np.where(ok[..., None], table[np.where(ok, ids, 0)], table.dtype.type(0))


def keys_of(table, series):
    B, T, C = series.shape
    return lookup(table, series).reshape(B, T, C * table.shape[1])


def projections(x, H):
    with np.errstate(invalid="ignore"):
        return np.einsum("...d,dm->...m", np.asarray(x, F64), np.asarray(H, F64))


def search_numpy(table, series, q, H, padding_index, K):
    """-> scores int32 [B,T], chosen int32 [B,K], sel [B,K,D] (the table's dtype), sel_valid int32 [B,K], sel_ids int64
    [B,K,C], valid bool [B,T]"""
    series = np.asarray(series, np.int64)
    x = keys_of(table, series)
    with np.errstate(invalid="ignore"):
        ck, cq = np.sign(projections(x, H)), np.sign(projections(q, H))
        scores = (ck == cq[:, None, :]).sum(-1).astype(np.int32)           # NaN == NaN is False
    valid = series[:, :, 0] != padding_index
    rank = np.where(valid, scores.astype(F64), -np.inf)
    chosen = np.argsort(-rank, axis=-1, kind="stable")[:, :K]
    rows = np.arange(len(series))[:, None]
    return {"scores": scores, "chosen": chosen.astype(np.int32), "sel": x[rows, chosen],
            "sel_valid": valid[rows, chosen].astype(np.int32), "sel_ids": series[rows, chosen], "valid": valid}


def undecided(table, series, q, H, padding_index):
    """bool [B]: the examples with a projection, of the item or of a valid step, whose fp32 sign is not decided"""
    x = np.asarray(keys_of(table, np.asarray(series, np.int64)), F64)
    D = x.shape[-1]
    H64 = np.asarray(H, F64)

    def open_(v):
        bound = 2.0 * D * 2.0 ** -24 * np.einsum("...d,dm->...m", np.abs(v), np.abs(H64))
        return (np.abs(projections(v, H64)) <= bound) & (bound > 0)          # every term zero: exactly 0 in any order
    valid = np.asarray(series)[:, :, 0] != padding_index
    return open_(np.asarray(q, F64)).any(-1) | (open_(x).any(-1) & valid).any(-1)


# ---- inputs -----------------------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(case, kind="exact", seed=0, padding_index=0):
    """One case's table [V,E], H [D,m], series [B,T,C], items [B,C], q [B,D] (the items' rows) and an exact-valued gsel
    [B,K,D].  Every row draws its steps from POOL items of its own.  About 30 % of the steps have the padding index in
    the first column and ordinary ids in the others, some are padded in every column, some read the zero row.  With B >=
    4: row 0 is one step repeated T times (all valid), row 1 has no valid step, row 2 has one valid step (fewer than K
    wherever K > 1), row 3's item is the zero row."""
    key = (case, kind, seed, padding_index)
    if key in _INPUTS:
        return _INPUTS[key]
    B, T, C, E, m, K, D = dims(case)
    rng = np.random.default_rng([seed, B, T, C, E, m])
    if kind == "exact":
        table = (rng.integers(-8, 9, (V_CASE, E)) / 8.0).astype(F32)
        H = (rng.integers(-4, 5, (D, m)) / 4.0).astype(F32)
    else:
        table = rng.uniform(-0.05, 0.05, (V_CASE, E)).astype(F32)
        H = (rng.standard_normal((D, m)) * 0.05).astype(F32)
    table[ZERO_ROW] = 0

    def ids(shape):                                       # ordinary ids: never the padding index
        v = rng.integers(1, V_CASE, shape)
        return np.where(v == padding_index, (padding_index + 1) % V_CASE or 1, v)
    n_pool = POOL if kind == "exact" else max(POOL, T)      # random: distinct steps, so that undecided signs do occur
    pool = ids((B, n_pool, C))
    series = np.ascontiguousarray(pool[np.arange(B)[:, None], rng.integers(0, n_pool, (B, T))]).astype(np.int64)
    series[rng.random((B, T)) < 0.08] = ZERO_ROW
    series[rng.random((B, T)) < 0.3, 0] = padding_index                     # the first column alone decides
    series[rng.random((B, T)) < 0.1] = padding_index
    items = ids((B, C)).astype(np.int64)
    if B >= 4:
        series[0] = pool[0, 0]
        series[1, :, 0] = padding_index
        series[2, :, 0] = padding_index
        series[2, T // 2] = pool[2, 1]
        items[3] = ZERO_ROW
    c = {"table": table, "H": H, "series": series, "items": items, "q": lookup(table, items).reshape(B, D),
         "gsel": (rng.integers(-8, 9, (B, K, D)) / 8.0).astype(F32), "padding_index": padding_index}
    _INPUTS[key] = c
    return c


_CACHE = {}


def reference(case, kind="exact", seed=0, padding_index=0):
    """search_numpy of a case's inputs, computed once and shared; nobody writes to it"""
    key = (case, kind, seed, padding_index)
    if key not in _CACHE:
        c = inputs(*key)
        _CACHE[key] = search_numpy(c["table"], c["series"], c["q"], c["H"], padding_index, dims(case)[5])
    return _CACHE[key]


def dense_table_grad(c, chosen, V=V_CASE):
    """the table's dense gradient under sum(sel * gsel): gsel's rows added at the chosen steps' ids (exact in fp32 for
    the exact-valued gsel: multiples of 1/8, sums far below 2^21)"""
    E = c["table"].shape[1]
    rows = np.arange(len(chosen))[:, None]
    ids = c["series"][rows, chosen].reshape(-1)
    g = np.zeros((V, E), F64)
    ok = (ids >= 0) & (ids < V)
    np.add.at(g, ids[ok], np.asarray(c["gsel"], F64).reshape(-1, E)[ok])
    return g.astype(F32)


# ---- the layer ----------------------------------------------------------------------------------------------------------
USER = ("uid", "utag1", "utag2", "utag3", "utag4")
ITEM = ("label_goods_ids", "label_shop_ids", "label_cate_ids")
LONG = ("longterm_goods_ids", "longterm_shop_ids", "longterm_cate_ids")
SHORT = ("shortterm_goods_ids", "shortterm_shop_ids", "shortterm_cate_ids")
LAYER_V, LAYER_B, LAYER_E, LAYER_M, LAYER_HEADS, LAYER_DK = 300, 48, 16, 16, 8, 4
LAYER_D = len(ITEM) * LAYER_E
MHA_PARTS = ("_query_dense", "_key_dense", "_value_dense", "_output_dense")


def state_shapes():
    """ETALayer(feature_dims=LAYER_V).state_dict(): name -> shape"""
    D, H, dk = LAYER_D, LAYER_HEADS, LAYER_DK
    s = {"projection_matrix": (D, LAYER_M), "embed.embeddings": (LAYER_V, LAYER_E)}
    for mha in ("shortterm_mha", "longterm_mha"):
        for n in MHA_PARTS[:3]:
            s.update({"%s.%s.kernel" % (mha, n): (D, H, dk), "%s.%s.bias" % (mha, n): (H, dk)})
        s.update({mha + "._output_dense.kernel": (H, dk, D), mha + "._output_dense.bias": (D,)})
    d = (len(ITEM) + len(USER)) * LAYER_E + 2 * D
    for i, unit in zip((0, 3), (200, 80)):              # Dense, LayerNormalization, Activation('relu')
        s.update({"final_mlp.layers.%d.kernel" % i: (d, unit), "final_mlp.layers.%d.bias" % i: (unit,),
                  "final_mlp.layers.%d.gamma" % (i + 1): (unit,), "final_mlp.layers.%d.beta" % (i + 1): (unit,)})
        d = unit
    s.update({"final_mlp.layers.6.kernel": (d, 1), "final_mlp.layers.6.bias": (1,)})
    return s


def layer_state(seed):
    rng = np.random.default_rng(700 + seed)
    sd = {}
    for k, shape in state_shapes().items():
        if k == "projection_matrix":
            v = rng.standard_normal(shape) * 0.05
        elif k.endswith("embeddings"):
            v = rng.standard_normal(shape) * 0.3
        elif k.endswith("gamma"):
            v = 1 + 0.1 * rng.standard_normal(shape)
        elif len(shape) == 3:
            v = rng.standard_normal(shape) / np.sqrt(LAYER_D)
        elif len(shape) == 2:
            v = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / sum(shape))
        else:
            v = rng.standard_normal(shape) * 0.2
        sd[k] = v.astype(F32)
    return sd


def layer_inputs(seed, B, T, S, left_padded=True):
    """ETALayer's input dict: ids [B] for the user and item features, [B,T] / [B,S] series drawn from a small pool per
    row; the long series is padded at random positions, the short one on the left (where 'reference' and 'valid' differ);
    row 0 has no valid step in either.  'weight' [B,1] is the upstream of the output."""
    rng = np.random.default_rng(900 + seed)
    ins = {k: rng.integers(1, LAYER_V, B) for k in USER + ITEM}
    for names, n in ((LONG, T), (SHORT, S)):
        pool = rng.integers(1, LAYER_V, (B, POOL, len(names)))
        ser = np.ascontiguousarray(pool[np.arange(B)[:, None], rng.integers(0, POOL, (B, n))])
        if names is LONG:
            ser[rng.random((B, n)) < 0.3] = 0
        else:
            pad = rng.integers(0, n + 1, B)
            mask = np.arange(n)[None, :] < pad[:, None]
            ser[mask if left_padded else mask[:, ::-1]] = 0
        ser[0] = 0
        for i, k in enumerate(names):
            ins[k] = np.ascontiguousarray(ser[:, :, i])
    ins["weight"] = rng.standard_normal((B, 1)).astype(F32)
    return ins


def _ids(ins, names):
    return torch.stack([torch.as_tensor(np.asarray(ins[k])).long() for k in names], -1)


def layer_undecided(sd, ins):
    """undecided() of the layer's long-term search"""
    table = np.asarray(sd["embed.embeddings"])
    series = _ids(ins, LONG).numpy()
    q = lookup(table, _ids(ins, ITEM).numpy()).reshape(len(series), -1)
    return undecided(table, series, q, sd["projection_matrix"], 0)


def _mlp_torch(p, h):
    for i in (0, 3):
        h = h @ p["final_mlp.layers.%d.kernel" % i] + p["final_mlp.layers.%d.bias" % i]
        mean, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
        h = (h - mean) / torch.sqrt(var + 1e-3) * p["final_mlp.layers.%d.gamma" % (i + 1)] \
            + p["final_mlp.layers.%d.beta" % (i + 1)]
        h = torch.relu(h)
    return torch.sigmoid(h @ p["final_mlp.layers.6.kernel"] + p["final_mlp.layers.6.bias"])


def eta_layer_torch(sd, ins, dtype, mask_mode, k=3, weight=None):
    """ETALayer.call (:607-626) op for op on the CPU at ``dtype`` under sum(output * weight): the output, the chosen
    positions and the dense gradient of every trainable entry.  The one deviation is the documented one: the padded
    steps rank as -inf (torch.where) instead of the reference's 0 * -inf."""
    p = {n: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=n != "projection_matrix") for n, v in sd.items()}
    table, H = p["embed.embeddings"], p["projection_matrix"]
    B = len(ins[USER[0]])
    X_item = table[_ids(ins, ITEM)].reshape(B, 1, -1)
    X_user = table[_ids(ins, USER)].reshape(B, -1)
    short_ids, long_ids = _ids(ins, SHORT), _ids(ins, LONG)
    X_short = table[short_ids].reshape(B, short_ids.shape[1], -1)
    X_long = table[long_ids].reshape(B, long_ids.shape[1], -1)
    shortterm_mask, longterm_mask = short_ids[:, :, 0] == 0, long_ids[:, :, 0] == 0

    def mha(name, value, attend):
        w = [p["%s.%s.%s" % (name, m, n)] for m in MHA_PARTS for n in ("kernel", "bias")]
        return SR.mha_torch(X_item, value, attend[:, None, :], *w)[0][:, 0]

    def prefix(count, n):                                                    # tf.sequence_mask
        return torch.arange(n)[None, :] < count[:, None]
    # generate_shorterm_interest
    if mask_mode == "reference":
        attend = prefix((~shortterm_mask).sum(1), shortterm_mask.shape[1])
    else:
        attend = ~shortterm_mask
    shortterm_interest = mha("shortterm_mha", X_short, attend)
    # generate_longterm_interest
    series_codes = torch.sign(torch.einsum("ble,em->blm", X_long, H))
    item_codes = torch.sign(torch.einsum("ble,em->blm", X_item, H))
    scores = (series_codes == item_codes).to(dtype).sum(-1)
    scores = torch.where(longterm_mask, torch.full_like(scores, -np.inf), scores)
    chosen = torch.sort(scores, dim=-1, descending=True, stable=True).indices[:, :k]
    top = torch.gather(X_long, 1, chosen.unsqueeze(-1).expand(-1, -1, X_long.shape[2]))
    top_mask = torch.gather(longterm_mask, 1, chosen)
    longterm_interest = mha("longterm_mha", top, prefix((~top_mask).sum(1), top_mask.shape[1]))
    out = _mlp_torch(p, torch.cat([X_item[:, 0], X_user, shortterm_interest, longterm_interest], 1))
    w = np.asarray(ins["weight"] if weight is None else weight)
    loss = (out * torch.tensor(w, dtype=dtype)).sum()
    names = [n for n in p if n != "projection_matrix"]
    grads = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
    return {"output": SR._f64(out), "chosen": chosen.numpy(),
            "grads": {n: (np.zeros(tuple(p[n].shape)) if g is None else SR._f64(g)) for n, g in zip(names, grads)}}
