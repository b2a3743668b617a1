"""What the SDIM tests share (not a test file): the numpy reading of the hash-bucket interest
(SDIMLayer.generate_longterm_interest with once=True, 8.DMR/CustomLayers.py:816-841) as include/mi355rec.h defines it --
TensorFlow cannot be imported here -- the torch-CPU transcription of the whole SDIMLayer (:772-955) parametrised by
dtype, the inputs of a case from a fixed seed and the case lists.

The interest: bit j of a row's code is (sum_d x_d H[d,j] > 0), from fp64 projections; group g's code is bits [g m,
(g+1) m); match[s,l,g] = the codes of step l and candidate s agree in group g.  Then EXACTLY the fp32 operations and
orders the header states: Sum[s,g,d] = sum of float(w_l) k_l[d] over the matching l in increasing l from 0; cnt[s,g] the
integer sum of n_l; mean = Sum / float(cnt), 0 where not finite; out = (mean_0 + mean_1 + ..) / float(G); and gkeys[l,d]
= the sum over s, then g, from 0, of (gout[s,d] / float(G)) / float(cnt[s,g]) over the matches, +0 for a step with w_l
= 0.  mode 'reference': w_l = pad_l, n_l = 1; 'valid': w_l = n_l = !pad_l.  An id outside [0, V) reads a zero row.

Two kinds of input, as tests/eta_ref.py has them:
  exact   table values in {-8..8}/8 and H in {-4..4}/4: every projection (see eta_ref) and every bucket sum -- at most
          T <= 300 multiples of 1/8 below 1 -- is exact in fp32 in any order; the divisions are single correctly rounded
          operations.  The kernels must equal this file bit for bit, forward and backward.
  random  table U(-0.05, 0.05), H N(0, 0.05).  A projection is DECIDED when |p64| > 2 D 2^-24 sum_d |x_d H_dj|
          (eta_ref's bound).  An example with an undecided projection in a candidate or in any step that enters a sum or a
          count -- in 'reference' mode every step, in 'valid' mode the valid ones -- is left out, at most
          eta_ref.MAX_LEFT_OUT of the examples (asserted).  On the others the integer outputs are equal and the float
          outputs lie within `out_bound` / `gkeys_bound` of the fp64 evaluation.

The bounds.  u = 2^-24, gamma(N) = N u / (1 - N u).  out[s,d] = sum_g sum_{l in bucket g} x_l / (cnt_g G) with x_l =
w_l k_l[d] exact (w is 0 or 1), cnt_g and G exact in fp32.  On its way into out a leaf x_l passes through at most
n_g - 1 additions of the bucket sum (n_g terms), one division, G - 1 additions over the groups and one division: N =
n_g + G roundings at the most, each of relative size u, so |out32 - out64| <= gamma(n + G) sum_g sum_l |x_l| / (cnt_g
G) with n = the largest bucket of the example (the standard bound of a sum evaluated in any fixed order).  In the same
way a leaf gout[s,d] / (G cnt[s,g]) of gkeys[l,d] passes two divisions and at most S G additions: |gkeys32 - gkeys64|
<= gamma(S G + 2) sum_{s,g: match} |gout[s,d]| / (G cnt[s,g]).  Neither is tuned or taken from a run.
"""
import numpy as np
import torch

from tests import eta_ref as ER
from tests import sim_ref as SR

F32, F64 = np.float32, np.float64
V_CASE, POOL, ZERO_ROW, NAN_ROW, MAX_LEFT_OUT = ER.V_CASE, ER.POOL, ER.ZERO_ROW, ER.NAN_ROW, ER.MAX_LEFT_OUT
rel_err, lookup, keys_of = ER.rel_err, ER.lookup, ER.keys_of
MODES = ("reference", "valid")
U = 2.0 ** -24

# (B, T, C, E, G, m, S): D = C E.  The reference's __main__ shape first; T on both sides of the 64-lane wave and of the
# 256-thread workgroup; G m at 1, 12, 16 | 17, 31 and 32 (the 16- and 32-column kernels); E at 1 and 2 (scalar row loads),
# 16, 48, 64, 256 (four 16-byte loads), 22 and 85 (odd strides); S at 1 and 16; D at 2 .. 256
REFERENCE = (3, 6, 3, 16, 4, 3, 1)
CASES = (REFERENCE, (5, 1, 1, 2, 1, 1, 1), (6, 63, 3, 16, 4, 4, 1), (6, 64, 1, 48, 31, 1, 3), (6, 65, 3, 22, 4, 8, 2),
         (5, 257, 1, 64, 2, 8, 16), (5, 257, 3, 85, 32, 1, 1), (5, 65, 1, 256, 1, 17, 4), (7, 300, 3, 1, 5, 1, 3))
# random inputs: large batches, so that the share left out is a share; (case, seed) for which this file alone stays under
# the cap in both modes; one 16-byte load per row (E = 4) is among them
RANDOM_CASES = (((256, 64, 3, 16, 4, 3, 1), 0), ((256, 65, 1, 48, 2, 8, 3), 0), ((128, 257, 3, 4, 31, 1, 2), 0),
                ((256, 64, 3, 16, 4, 3, 1), 1))


def dims(case):
    B, T, C, E, G, m, S = case
    return B, T, C, E, G, m, S, C * E


def projections(x, H):
    """fp64 x [.., D] times H [D, G, m] -> [.., G m]"""
    H = np.asarray(H, F64)
    with np.errstate(invalid="ignore"):
        return np.einsum("...d,dj->...j", np.asarray(x, F64), H.reshape(H.shape[0], -1))


def pack(bits):
    """bool [.., n <= 32] -> int32 [..], bit j from column j"""
    word = (bits.astype(np.uint64) << np.arange(bits.shape[-1], dtype=np.uint64)).sum(-1)
    return word.astype(np.uint32).view(np.int32)


def flags(pad, mode):
    """-> (w, n) bool [B,T]"""
    assert mode in MODES
    return (pad, np.ones_like(pad)) if mode == "reference" else (~pad, ~pad)


def interest_numpy(table, series, q, H, padding_index, mode, gout=None):
    """table [V,E], series [B,T,C], q [B,S,D], H [D,G,m] -> out f32 [B,S,D], codes int32 [B,T], qcodes int32 [B,S], cnt
    int32 [B,S,G], out64 (the same in fp64 throughout), match bool [B,S,T,G], pad [B,T], terms int [B] (the largest
    number of summed steps of a bucket) and, with gout [B,S,D], gkeys f32 [B,T,D] and gkeys64"""
    series = np.asarray(series, np.int64)
    G, m = H.shape[1:]
    x = keys_of(table, series)                                                  # [B,T,D] fp32
    with np.errstate(invalid="ignore"):
        kb, qb = projections(x, H) > 0, projections(q, H) > 0                   # NaN > 0 is False
    B, T, D = x.shape
    S = q.shape[1]
    match = (kb.reshape(B, 1, T, G, m) == qb.reshape(B, S, 1, G, m)).all(-1)    # [B,S,T,G]
    pad = series[:, :, 0] == padding_index
    w, n = flags(pad, mode)
    cnt = (match & n[:, None, :, None]).sum(2).astype(np.int32)                 # [B,S,G]
    res = {"codes": pack(kb), "qcodes": pack(qb), "cnt": cnt, "match": match, "pad": pad,
           "terms": (match & w[:, None, :, None]).sum(2).max((1, 2))}
    for dt, tag in ((F32, ""), (F64, "64")):
        xw = x.astype(dt) * w[:, :, None].astype(dt)                            # float(w_l) k_l[d]
        acc = np.zeros((B, S, G, D), dt)
        with np.errstate(all="ignore"):
            for l in range(T):                                                  # in increasing l
                acc = np.where(match[:, :, l, :, None], acc + xw[:, None, l, None, :], acc)
            mean = acc / cnt.astype(dt)[..., None]
            mean = np.where(np.isfinite(mean), mean, dt(0))
            out = mean[:, :, 0]
            for g in range(1, G):                                               # in increasing g
                out = out + mean[:, :, g]
            out = out / dt(G)
        assert out.dtype == dt
        res["out" + tag] = out
        if gout is not None:
            gd = np.asarray(gout, dt) / dt(G)
            acc = np.zeros((B, T, D), dt)
            with np.errstate(all="ignore"):
                for s in range(S):                                              # over s, then over g
                    for g in range(G):
                        term = gd[:, s, None, :] / cnt.astype(dt)[:, s, g, None, None]
                        acc = np.where(match[:, s, :, g, None], acc + term, acc)
            res["gkeys" + tag] = np.where(w[:, :, None], acc, dt(0))
            assert res["gkeys" + tag].dtype == dt
    return res


def gamma(N):
    return N * U / (1.0 - N * U)


def out_bound(table, series, ref, mode, G):
    """[B,S,D]: gamma(n + G) sum_g sum_{l in bucket} |w_l k_l[d]| / (cnt_g G), the module docstring's derivation"""
    x = np.abs(np.asarray(keys_of(table, np.asarray(series, np.int64)), F64))
    w, _ = flags(ref["pad"], mode)
    mass = np.einsum("bslg,bld->bsgd", (ref["match"] & w[:, None, :, None]).astype(F64), x)
    with np.errstate(all="ignore"):
        mass = np.where(ref["cnt"][..., None] > 0, mass / ref["cnt"][..., None], 0.0).sum(2) / G
    return gamma(ref["terms"] + G)[:, None, None] * mass


def gkeys_bound(gout, ref, mode):
    """[B,T,D]: gamma(S G + 2) sum_{s,g: match} |gout[s,d]| / (G cnt[s,g])"""
    B, S, T, G = ref["match"].shape
    w, _ = flags(ref["pad"], mode)
    with np.errstate(all="ignore"):
        inv = np.where(ref["cnt"] > 0, 1.0 / (G * ref["cnt"].astype(F64)), 0.0)          # [B,S,G]
    mass = np.einsum("bslg,bsg,bsd->bld", ref["match"].astype(F64), inv, np.abs(np.asarray(gout, F64)))
    return gamma(S * G + 2) * mass * w[:, :, None]


def undecided(table, series, q, H, padding_index, mode):
    """bool [B]: the examples with a projection, of a candidate or of a step that enters a sum or a count, whose fp32
    sign is not decided"""
    x = np.asarray(keys_of(table, np.asarray(series, np.int64)), F64)
    D = x.shape[-1]
    H64 = np.abs(np.asarray(H, F64)).reshape(D, -1)

    def open_(v):
        bound = 2.0 * D * U * np.einsum("...d,dj->...j", np.abs(v), H64)
        return (np.abs(projections(v, H)) <= bound) & (bound > 0)                # every term zero: exactly 0 in any order
    pad = np.asarray(series)[:, :, 0] == padding_index
    enters = np.ones_like(pad) if mode == "reference" else ~pad
    return open_(np.asarray(q, F64)).any((-1, -2)) | (open_(x).any(-1) & enters).any(-1)


# ---- inputs -----------------------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs(case, kind="exact", seed=0, padding_index=0):
    """One case's table [V,E], H [D,G,m], series [B,T,C], items [B,S,C], q [B,S,D] (the items' rows) and an exact-valued
    gout [B,S,D].  Every row draws its steps from POOL items of its own, and half of its candidates from the same pool, so
    that a candidate meets steps with ITS ids (equal codes bit for bit) whatever m is.  About 30 % of the steps have the
    padding index in the first column and ordinary ids in the others, some are padded in every column, some read the
    zero row.  With B >= 4: row 0 is one step repeated T times (all valid) and its first candidate is that step, row 1
    has no valid step, row 2 has one valid step, row 3's first candidate is the zero row and, with S >= 2, its second
    the padding row itself (the one candidate sure to meet the fully padded steps, which 'reference' mode sums)."""
    key = (case, kind, seed, padding_index)
    if key in _INPUTS:
        return _INPUTS[key]
    B, T, C, E, G, m, S, D = dims(case)
    rng = np.random.default_rng([seed, B, T, C, E, G, m, S])
    if kind == "exact":
        table = (rng.integers(-8, 9, (V_CASE, E)) / 8.0).astype(F32)
        H = (rng.integers(-4, 5, (D, G, m)) / 4.0).astype(F32)
    else:
        table = rng.uniform(-0.05, 0.05, (V_CASE, E)).astype(F32)
        H = (rng.standard_normal((D, G, m)) * 0.05).astype(F32)
    table[ZERO_ROW] = 0

    def ids(shape):                                       # ordinary ids: never the padding index
        v = rng.integers(1, V_CASE, shape)
        return np.where(v == padding_index, (padding_index + 1) % V_CASE or 1, v)
    n_pool = POOL if kind == "exact" else max(POOL, T)      # random: distinct steps, so that undecided signs do occur
    pool = ids((B, n_pool, C))
    rows = np.arange(B)[:, None]
    series = np.ascontiguousarray(pool[rows, rng.integers(0, n_pool, (B, T))]).astype(np.int64)
    series[rng.random((B, T)) < 0.08] = ZERO_ROW
    series[rng.random((B, T)) < 0.3, 0] = padding_index                     # the first column alone decides
    series[rng.random((B, T)) < 0.1] = padding_index
    from_pool = pool[rows, rng.integers(0, n_pool, (B, S))]
    items = np.where((rng.random((B, S)) < 0.5)[..., None], from_pool, ids((B, S, C))).astype(np.int64)
    if B >= 4:
        series[0] = pool[0, 0]
        items[0, 0] = pool[0, 0]
        series[1, :, 0] = padding_index
        series[2, :, 0] = padding_index
        series[2, T // 2] = pool[2, 1]
        items[3, 0] = ZERO_ROW
        if S >= 2:
            items[3, 1] = padding_index
    c = {"table": table, "H": H, "series": series, "items": items, "q": lookup(table, items).reshape(B, S, D),
         "gout": (rng.integers(-8, 9, (B, S, D)) / 8.0).astype(F32), "padding_index": padding_index}
    _INPUTS[key] = c
    return c


_CACHE = {}


def reference(case, mode, kind="exact", seed=0, padding_index=0):
    """interest_numpy of a case's inputs with its gout, computed once and shared; nobody writes to it"""
    key = (case, mode, kind, seed, padding_index)
    if key not in _CACHE:
        c = inputs(case, kind, seed, padding_index)
        _CACHE[key] = interest_numpy(c["table"], c["series"], c["q"], c["H"], padding_index, mode, c["gout"])
    return _CACHE[key]


def dense_table_grad(c, gkeys, V=V_CASE):
    """the table's dense gradient: gkeys' rows added at the series' ids in fp64, rounded once (exact for the exact-valued
    inputs only where the tests say so)"""
    E = c["table"].shape[1]
    ids = c["series"].reshape(-1)
    g = np.zeros((V, E), F64)
    ok = (ids >= 0) & (ids < V)
    np.add.at(g, ids[ok], np.asarray(gkeys, F64).reshape(-1, E)[ok])
    return g


# ---- the layer ----------------------------------------------------------------------------------------------------------
USER, ITEM, LONG, SHORT = ER.USER, ER.ITEM, ER.LONG, ER.SHORT
LAYER_V, LAYER_B, LAYER_E, LAYER_HEADS, LAYER_DK = 300, 48, 16, 8, 4
LAYER_G, LAYER_M = 4, 3
LAYER_D = len(ITEM) * LAYER_E
MHA_PARTS = ER.MHA_PARTS


def state_shapes():
    """SDIMLayer(feature_dims=LAYER_V).state_dict(): name -> shape (the reference's longterm_mha is never called, so
    Keras builds no weights for it)"""
    s = {k: v for k, v in ER.state_shapes().items() if not k.startswith("longterm_mha")}
    s["projection_matrix"] = (LAYER_D, LAYER_G, LAYER_M)
    return s


def layer_state(seed):
    rng = np.random.default_rng(1700 + seed)
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


def layer_inputs(seed, B, T, Ns, S=1, left_padded=True, item_rank=None):
    """SDIMLayer's input dict: eta_ref.layer_inputs (user ids [B], a long series [B,T] padded at random positions, a
    short one [B,Ns] padded on the left, row 0 without a valid step in either) with S candidates per example: item
    features [B,S] -- [B] or [B,1] for S = 1 as ``item_rank`` (1 or 2) says -- half of them steps of the example's long
    series.  'weight' [B,S,1] is the upstream of the output."""
    ins = ER.layer_inputs(seed, B, T, Ns, left_padded)
    rng = np.random.default_rng(1900 + seed)
    long_ids = np.stack([ins[k] for k in LONG], -1)                           # [B,T,C]
    picked = long_ids[np.arange(B)[:, None], rng.integers(0, T, (B, S))]
    fresh = rng.integers(1, LAYER_V, (B, S, len(ITEM)))
    items = np.where((rng.random((B, S)) < 0.5)[..., None] & (picked[..., :1] != 0), picked, fresh)
    for i, k in enumerate(ITEM):
        col = np.ascontiguousarray(items[:, :, i])
        if S == 1 and item_rank is not None:
            col = col.reshape(B) if item_rank == 1 else col.reshape(B, 1)
        ins[k] = col
    ins["weight"] = rng.standard_normal((B, S, 1)).astype(F32)
    return ins


def _ids(ins, names):
    cols = [torch.as_tensor(np.asarray(ins[k])).long() for k in names]
    return torch.stack(cols, -1)


def _item_ids(ins):
    B = len(ins[USER[0]])
    return torch.stack([torch.as_tensor(np.asarray(ins[k])).long().reshape(B, -1) for k in ITEM], -1)      # [B,S,C]


def layer_undecided(sd, ins, mode):
    """undecided() of the layer's long-term interest"""
    table = np.asarray(sd["embed.embeddings"])
    series = _ids(ins, LONG).numpy()
    items = _item_ids(ins).numpy()
    q = lookup(table, items).reshape(items.shape[0], items.shape[1], -1)
    return undecided(table, series, q, sd["projection_matrix"], 0, mode)


def sdim_layer_torch(sd, ins, dtype, mask_mode, weight=None):
    """SDIMLayer.call (:933-955) op for op on the CPU at ``dtype`` under sum(output * weight): the output [B,S,1], the
    counts and the dense gradient of every trainable entry.  Two things are spelled differently.  The one-hot of the 2^m
    codes is replaced by the equality of the codes, which selects the same steps.  And the empty bucket is divided by 1
    behind the same where: 0 / 0 behind tf.where sends NaN back through the division, and the defined gradient there is
    zero."""
    p = {n: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=n != "projection_matrix") for n, v in sd.items()}
    table, H = p["embed.embeddings"], p["projection_matrix"]
    B = len(ins[USER[0]])
    item_ids = _item_ids(ins)
    S = item_ids.shape[1]
    X_item = table[item_ids].reshape(B, S, -1)
    X_user = table[_ids(ins, USER)].reshape(B, 1, -1)
    short_ids, long_ids = _ids(ins, SHORT), _ids(ins, LONG)
    X_short = table[short_ids].reshape(B, short_ids.shape[1], -1)
    X_long = table[long_ids].reshape(B, long_ids.shape[1], -1)
    shortterm_mask, longterm_mask = short_ids[:, :, 0] == 0, long_ids[:, :, 0] == 0
    # generate_shorterm_interest
    if mask_mode == "reference":
        attend = torch.arange(shortterm_mask.shape[1])[None, :] < (~shortterm_mask).sum(1)[:, None]     # sequence_mask
    else:
        attend = ~shortterm_mask
    w = [p["shortterm_mha.%s.%s" % (m, n)] for m in MHA_PARTS for n in ("kernel", "bias")]
    shortterm_interest = SR.mha_torch(X_item, X_short, attend[:, None, :], *w)[0]
    # generate_longterm_interest, once=True
    series_binary = torch.einsum("ble,egm->blgm", X_long, H) > 0             # where(sign == 1, 1, 0)
    items_binary = torch.einsum("bse,egm->bsgm", X_item, H) > 0
    same = (series_binary[:, None] == items_binary[:, :, None]).all(-1).to(dtype)                       # [B,S,T,G]
    if mask_mode == "reference":
        mask, counted = longterm_mask.to(dtype), torch.ones(longterm_mask.shape, dtype=dtype)
    else:
        mask = counted = (~longterm_mask).to(dtype)
    masked_series_embedding = X_long * mask[:, :, None]
    c_specific_embedding = torch.einsum("bslg,ble->bsge", same, masked_series_embedding)
    valid_count = torch.einsum("bslg,bl->bsg", same, counted)
    division_result = c_specific_embedding / valid_count.clamp(min=1).unsqueeze(-1)
    keep = torch.isfinite(division_result) & (valid_count > 0).unsqueeze(-1)
    safe_result = torch.where(keep, division_result, torch.zeros_like(division_result))
    longterm_interest = safe_result.mean(2)
    X_combined = torch.cat([X_item, X_user.expand(-1, S, -1), shortterm_interest, longterm_interest], 2)
    out = ER._mlp_torch(p, X_combined)
    wgt = np.asarray(ins["weight"] if weight is None else weight)
    loss = (out * torch.tensor(wgt, dtype=dtype)).sum()
    names = [n for n in p if n != "projection_matrix"]
    grads = torch.autograd.grad(loss, [p[n] for n in names], allow_unused=True)
    return {"output": SR._f64(out), "cnt": valid_count.detach().numpy().astype(np.int64),
            "interest": SR._f64(longterm_interest),
            "grads": {n: (np.zeros(tuple(p[n].shape)) if g is None else SR._f64(g)) for n, g in zip(names, grads)}}


# ---- the projection's arithmetic ----------------------------------------------------------------------------------------
# (B, T, C, E, G, m, S) with C = 2: the 16- and the 32-column kernels, each with four 16-byte loads, one, and scalar loads
ARITHMETIC_CASES = ((32, 65, 2, 16, 4, 3, 4), (32, 65, 2, 4, 4, 4, 4), (32, 65, 2, 5, 2, 8, 4),
                    (32, 65, 2, 48, 4, 8, 4), (32, 65, 2, 12, 31, 1, 4), (32, 65, 2, 22, 17, 1, 4))


def projections_fp32(x, H):
    """the projection as the header states it, in fp32: p = p + x_d H[d,:] for d in order from 0, the product rounded
    before the sum (numpy rounds every operation; nothing is fused) -> fp32 [.., G m]"""
    x, H = np.asarray(x, F32), np.asarray(H, F32).reshape(np.shape(H)[0], -1)
    p = np.zeros(x.shape[:-1] + (H.shape[1],), F32)
    for d in range(H.shape[0]):
        p = p + x[..., d, None] * H[d]
    assert p.dtype == F32
    return p


def projections_fused(x, H):
    """the same sum with the product NOT rounded (a fused multiply-add: the exact product, fp64 holds it, added and
    rounded once), what a contracted build computes: for the generator's own check that its inputs tell the two apart"""
    x, H = np.asarray(x, F64), np.asarray(H, F64).reshape(np.shape(H)[0], -1)
    p = np.zeros(x.shape[:-1] + (H.shape[1],), F32)
    for d in range(H.shape[0]):
        p = (p.astype(F64) + x[..., d, None] * H[d]).astype(F32)
    return p


def arithmetic_inputs(case, seed=0):
    """Random inputs on which the SIGN of a projection is a matter of its rounding: C = 2, the second half of H is minus
    the first, and two steps in three carry the same id in both columns, so that their projections are what the
    roundings of sum_e x_e H_e - sum_e x_e H_e leave over: zero or a few ulps of either sign, different ones under any
    other order or fusion of the operations.  No step is padded.  Candidate s of an example is a copy of its step 7 s
    mod T.  -> table, H, series [B,T,2], items [B,S,2], q [B,S,D]"""
    B, T, C, E, G, m, S, D = dims(case)
    assert C == 2
    rng = np.random.default_rng([77, seed, E, G, m])
    table = rng.uniform(-0.05, 0.05, (V_CASE, E)).astype(F32)
    half = (rng.standard_normal((E, G, m)) * 0.05).astype(F32)
    H = np.concatenate([half, -half], 0)
    series = rng.integers(1, V_CASE, (B, T, 2)).astype(np.int64)
    same = rng.random((B, T)) < 2 / 3
    series[same, 1] = series[same, 0]
    items = np.ascontiguousarray(series[:, (7 * np.arange(S)) % T])
    return {"table": table, "H": H, "series": series, "items": items, "q": lookup(table, items).reshape(B, S, D)}
