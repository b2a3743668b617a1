"""Tensor-level wrappers over the C ABI (include/mi355rec.h).

torch is plumbing here: it owns device memory and the current HIP stream; every function below hands raw
device pointers and the stream handle to libmi355rec.so and returns torch tensors that view the results.
Nothing in this file computes on the CPU or through torch ops -- a non-CUDA tensor is an error.

A wrapper of a kernel family is five steps, each with its policy in one helper below: (1) check the operands against
each other (_req, _expect, _expect_all, _vec, _keyed_head, _caps_head) and against the family's limits (its own
*_check_shape); (2) allocate the outputs -- _new / _new_like for what the launch writes in full, which is zeros where
the batch is empty and nothing is launched, torch.zeros / torch.zeros_like for what kernels add into or leave alone;
(3) launch nothing for an empty batch; (4) make one _call, or one _call_ws where the entry point ends in (workspace,
nbytes, stream): _call alone appends the stream and checks the status, _workspace alone turns the answer of a
rec_*_workspace_bytes query into memory; (5) return the tensors.
"""
import ctypes as C

import torch

from ._lib import lib, check, tops, LIMITS, ENUMS

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_SIGMOID, EPI_BIAS_TANH, EPI_CROSS, EPI_ADD = (
    ENUMS["REC_EPI_" + k] for k in ("NONE", "BIAS", "BIAS_RELU", "BIAS_SIGMOID", "BIAS_TANH", "CROSS", "ADD"))
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = (ENUMS["REC_ACT_" + k] for k in ("NONE", "RELU", "SIGMOID", "TANH"))
ACT_CODE = {None: ACT_NONE, "linear": ACT_NONE, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH}
EPI_OF_ACT = {ACT_NONE: EPI_BIAS, ACT_RELU: EPI_BIAS_RELU, ACT_SIGMOID: EPI_BIAS_SIGMOID, ACT_TANH: EPI_BIAS_TANH}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _req(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on the MI355X (got %r): the HIP path has no CPU fallback"
                           % (name, getattr(t, "device", type(t))))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _f32(t, name):
    return _req(t, torch.float32, name)


def _i64(t, name):
    return _req(t, torch.int64, name)


def _expect(t, shape, name, label=None, dtype=torch.float32, optional=False):
    """``t`` is a contiguous tensor of ``dtype`` and ``shape`` on the device (or, with ``optional``, None); ``label``
    spells the shape in the error, which shows a one-dimensional shape as [n]"""
    if t is None and optional:
        return
    if tuple(_req(t, dtype, name).shape) != tuple(shape):
        want = "[%d]" % tuple(shape) if len(shape) == 1 else tuple(shape)
        raise ValueError("%s must be %s, got %s"
                         % (name, want if label is None else "%s = %s" % (label, want), tuple(t.shape)))


def _expect_all(named):
    """_expect over (tensor, shape, name) each: the saved tensors and upstream gradients of a backward, of which a
    missing one is a shape error"""
    for t, shape, name in named:
        if t is None:
            raise ValueError("%s must be %s, got None" % (name, tuple(shape)))
        _expect(t, shape, name)


def _vec(t, n, name):
    """``t`` holds n floats in any shape"""
    if _f32(t, name).numel() != n:
        raise ValueError("%s must hold %d floats, got %s" % (name, n, tuple(t.shape)))
    return t


def _keyed_head(x, values, E=None, F=None, name="dx"):
    """The head of a keyed input stage, whose last ``values.shape[1]`` of F fields are scaled by ``values``: ``x`` is X
    [B,F] int64 beside a table of width ``E`` (the forward) or, with ``F`` given, the fp32 [B, F E] called ``name`` (the
    backward); ``values`` is None or fp32 [B,Fk] with 0 <= Fk <= F.  -> (B, F, E, Fk); the limits are the family's."""
    if F is None:
        if _i64(x, "X").dim() != 2:
            raise ValueError("X must be [B, fields]")
        B, F = x.shape
    else:
        if _f32(x, name).dim() != 2 or F < 1 or x.shape[1] % F:
            raise ValueError("%s must be [B, fields * embedding_dims] with fields=%d, got %s" % (name, F, tuple(x.shape)))
        B, E = x.shape[0], x.shape[1] // F
    Fk = 0 if values is None else (values.shape[1] if values.dim() == 2 else -1)
    if not 0 <= Fk <= F:
        raise ValueError("values must be [B, continuous fields <= %d], got %s" % (F, tuple(values.shape)))
    if Fk > 0:
        _expect(values, (B, Fk), "values", "[B,Fk]")
    return B, F, E, Fk


def _new(shape, dev, B=1, dtype=torch.float32):
    """an output the launch writes in full; zeros where the batch ``B`` is empty and nothing is launched"""
    return (torch.zeros if B == 0 else torch.empty)(shape, dtype=dtype, device=dev)


def _new_like(t, B=1):
    """_new in the shape of the contiguous ``t``: the gradient of a weight, the result of a row-wise op"""
    return (torch.zeros_like if B == 0 else torch.empty_like)(t)


def _ptrs(tensors):
    return [_ptr(t) for t in tensors]


def _ptr_array(tensors):
    """a host array of device pointers, for the entry points that take a list of tensors"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


def _call(fn, *args):
    check(getattr(lib, fn)(*args, _stream()), fn)


def _workspace(nbytes, what, device):
    """Scratch for one ABI call, nbytes as its rec_*_workspace_bytes answered.  `what` names that entry point where its
    answer is 0 for a shape the kernels do not cover; None where 0 bytes only means that nothing is needed."""
    if nbytes == 0 and what is not None:
        raise NotImplementedError("%s: unsupported shape" % what)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def _call_ws(query, query_args, fn, dev, *args, may_need_none=False):
    """``fn`` with the workspace that ``query`` asks for at ``query_args``, for the entry points that end in (workspace,
    nbytes, stream); ``may_need_none``: 0 bytes is an answer, not an uncovered shape"""
    nbytes = getattr(lib, query)(*query_args)
    ws = _workspace(nbytes, None if may_need_none else query, dev)
    _call(fn, *args, _ptr(ws), nbytes)


def _table(t, name):
    """A table may be a strided row view (fused layout): 2-D fp32 CUDA with unit inner stride."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on the MI355X: the HIP path has no CPU fallback" % name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError("%s must be a 2-D fp32 table with unit inner stride" % name)
    return t


def fused_row_stride(E):
    """Row stride (floats) of the fused [embed(E) | w | pad] layout: next power of two >= E+1, at least 16."""
    ld = 16
    while ld < E + 1:
        ld *= 2
    return ld


# ---------------------------------------------------------------------------------------------------
# K1 / K2 / K3
# ---------------------------------------------------------------------------------------------------

def index_pack(cols, out=None, col0=0):
    """cols: list of int64 tensors with the same number of elements ([B], [B,1] or [B,T]).
    Returns X [rows, F] int64 (expand_dims + concat(axis=1), 2.FM/CustomLayers.py:138-144)."""
    F = len(cols)
    rows = cols[0].numel()
    for c in cols:
        _i64(c, "index column")
        if c.numel() != rows:
            raise ValueError("index columns differ in length")
    return tops.index_pack(list(cols), out, col0)


def new_flag(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


def emb_gather(table, idx, oob=None):
    _table(table, "table"); _i64(idx, "idx")
    return tops.emb_gather(table, idx, oob)


def emb_fm_fwd(embed, w, bias, X, want_prob=False, want_rows=False, want_sum=True, oob=None):
    """Fused w(X), embed(X) and the FM sum-square trick.  Returns z [B], prob [B]|None, rows [B,F,E]|None,
    sumvec [B,E]|None."""
    _table(embed, "embed"); _table(w, "w"); _f32(bias, "bias"); _i64(X, "X")
    return tops.emb_fm_fwd(embed, w, bias, X, want_prob, want_rows, want_sum, oob)


def emb_fm_bwd_vals(embed, X, gz, sumvec, rows=None, extra=None):
    """IndexedSlices values of the FM part: [B*F, E]."""
    return tops.emb_fm_bwd_vals(embed, X, _f32(gz, "gz"), sumvec, rows, extra)


# ---------------------------------------------------------------------------------------------------
# K4 de-duplication
# ---------------------------------------------------------------------------------------------------

class DedupPlan:
    """Sorted-unique plan of a flat id list; reusable for every table indexed by the same ids.

    ``list_counts`` (int64 device tensor [P]): the ids are P ascending duplicate-free lists laid end to end (what P
    requesters send to a shard owner after de-duplicating their own batches); the plan is then a rank merge instead
    of a radix sort (rec_dedup_plan_sorted_lists_i64)."""

    def __init__(self, ids, V, list_counts=None):
        ids = _i64(ids.reshape(-1), "ids")
        n = ids.numel()
        dev = ids.device
        self.n = n
        if list_counts is None:
            self.uniq_ids, self.seg_start, self.perm, self.n_uniq = tops.dedup_plan(ids, V)
        else:
            lc = _i64(list_counts.reshape(-1), "list_counts")
            self.uniq_ids = _new(max(n, 1), dev, dtype=torch.int64)
            self.seg_start = _new(n + 1, dev, dtype=torch.int32)
            self.perm = _new(max(n, 1), dev, dtype=torch.int32)
            self.n_uniq = _new(1, dev, dtype=torch.int64)
            _call_ws("rec_dedup_workspace_bytes", (n,), "rec_dedup_plan_sorted_lists_i64", dev, _ptr(ids), n, _ptr(lc),
                     lc.numel(), V, _ptr(self.uniq_ids), _ptr(self.seg_start), _ptr(self.perm), _ptr(self.n_uniq),
                     may_need_none=True)

    def segment_sum(self, vals, E, row_div=1, wide=False):
        """vals [n/row_div, E] -> [n, E]; rows >= n_uniq are zero.  ``wide``: rows of more than 256 columns go through
        the wide-row kernel in one launch (a workgroup per unique id) instead of 256-column slices."""
        if E > 256 and not wide:      # wide rows (FFM's F*E): the kernel takes up to 256 columns at a time
            out = _new((max(self.n, 1), E), vals.device)
            for c0 in range(0, E, 256):
                c1 = min(E, c0 + 256)
                out[:, c0:c1] = self.segment_sum(vals[:, c0:c1].contiguous(), c1 - c0, row_div)
            return out
        return tops.segment_sum(_f32(vals, "vals"), E, self.perm, self.seg_start, self.n, row_div)


def l2_used_rows(table, plan, factor):
    """factor * l2_loss(table[unique ids of the plan]) (5.DIN/ModelManager.py:188-190) -> (loss [1], its gradient as
    rows [n,E] aligned with plan.uniq_ids; zero beyond n_uniq)."""
    _table(table, "table")
    V, E = table.shape
    n = plan.n
    dev = table.device
    rows, loss = _new((max(n, 1), E), dev), _new(1, dev)
    ws = _workspace(lib.rec_l2_rows_workspace_bytes(n, E), None, dev)
    _call("rec_l2_rows_f32", _ptr(table), table.stride(0), V, E, _ptr(plan.uniq_ids), _ptr(plan.n_uniq), n,
          float(factor), _ptr(rows), _ptr(loss), _ptr(ws))
    return loss, rows


# ---------------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------------

def gemm(A, B, transA=False, transB=False, epi=EPI_NONE, bias=None, e0=None, e1=None, split_k=None, out=None,
         aux=None):
    """C = epi(op(A) @ op(B)) on the fp32 matrix cores.  A, B are 2-D row-major (leading dim = stride(0)).
    ``split_k=None``: chosen by split_k_for (a deep reduction over few output tiles is cut into slices that are added
    in slice order -- e.g. DIN's gq = gMext . Wcat^T, [4096,3492] x [3492,96], ran on 32 workgroups)."""
    for t, nm in ((A, "A"), (B, "B")):
        if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError("%s must be a 2-D fp32 CUDA tensor with unit inner stride" % nm)
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != K2:
        raise ValueError("gemm inner dimensions differ: %d vs %d" % (K, K2))
    if out is None:
        out = _new((M, N), A.device)
    if out.dim() != 2 or tuple(out.shape) != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise ValueError("out must be a 2-D fp32 [%d,%d] tensor with unit inner stride" % (M, N))
    if aux is not None:
        # the kernel writes U with C's leading dimension: a contiguous aux beside a column-slice `out` would be
        # written out of bounds
        if (tuple(aux.shape) != (M, N) or aux.dtype != torch.float32 or aux.stride(1) != 1
                or aux.stride(0) != out.stride(0)):
            raise ValueError("aux must be fp32 [%d,%d] with the same row stride as out (%d), got stride %s"
                             % (M, N, out.stride(0), tuple(aux.stride())))
    if split_k is None:
        skinny = (not transA) and (not transB) and N <= 64 and M >= 256      # the no-LDS kernel splits K over its waves
        split_k = 1 if skinny else split_k_for(K, M, N, transA, transB)
    return tops.gemm(A, B, bool(transA), bool(transB), epi, bias, e0, e1, int(split_k), out, aux)


def act_fwd(act, x, x2=None):
    """y = act(x + x2)."""
    return tops.act_fwd(act, _f32(x, "x"), x2)


def crossnet_mat_bwd_elem(g, x0, u, gx0, accumulate):
    """h = g*x0 (returned); gx0 (+)= g*u in place."""
    return tops.crossnet_mat_bwd_elem(_f32(g, "g"), x0, u, gx0, bool(accumulate))


def act_bwd(act, post, dpost):
    return tops.act_bwd(act, _f32(post, "post"), _f32(dpost, "dpost"))


def colsum(X, out=None):
    return tops.colsum(X, out)


def axpby(a, x, b, y):
    return tops.axpby(float(a), _f32(x, "x"), float(b), _f32(y, "y"))


def copy_cols(src, dst_view):
    """dst_view[:, :] = src, both 2-D with unit inner stride (dst may be a column block of a wider buffer)."""
    rows, w = src.shape
    _call("rec_copy_cols_f32", _ptr(src), src.stride(0), _ptr(dst_view), dst_view.stride(0), rows, w)
    return dst_view


def split_k_for(K, M, N, transA=False, transB=False):
    """Heuristic split of a reduction over the batch.  The tile kernels keep up to three workgroups per CU, and the time of
    a few-tile weight gradient [M,N] = X^T dY with K = batch is a staircase in tiles x slices: it is best just below a
    multiple of the 256 CUs (measured, M = N = 835, K = 16384, 49 tiles: 8 slices 324 us, 10: 265, 12: 313, 15: 260,
    21: 300; M = N = 323, 9 tiles: 24 slices 79 us, 56: 64, 57: 77).  So: the largest number of slices that keeps
    tiles x slices <= 768 (512 for very few tiles, whose partials are cheap to add either way), at least 64 k per slice
    and at most 64 MB of partials; these are added in slice order by the split-K reduce."""
    t = 128 if (M > 64 and N > 64) else 64          # tile edge the kernel will use
    tiles = ((M + t - 1) // t) * ((N + t - 1) // t)
    if tiles >= 512 or K < 1024:
        return 1
    slots = 512 if tiles < 16 else 768
    split = max(1, min(256, slots // max(tiles, 1), K // 64))
    cap = max(8, (64 << 20) // max(1, 4 * M * N))       # the partials are written and read again
    return int(min(split, cap))


# ---------------------------------------------------------------------------------------------------
# CrossNet vector mode, cosine, BCE, Adam
# ---------------------------------------------------------------------------------------------------

def crossnet_vec_fwd(x0, w, b, save=True):
    B, D = x0.shape
    L = w.shape[0]
    _f32(x0, "x0"); _f32(w, "w"); _f32(b, "b")
    y = _new_like(x0)
    xs = _new((L, B, D), x0.device) if save else None
    _call("rec_crossnet_vec_fwd_f32", _ptr(x0), B, D, L, _ptr(w), _ptr(b), _ptr(y), _ptr(xs))
    return y, xs


def crossnet_vec_bwd(x0, w, xs, gy):
    B, D = x0.shape
    L = w.shape[0]
    _f32(gy, "gy")
    gx0, dw, db = _new_like(x0), _new_like(w, B), _new_like(w, B)
    ws = _workspace(lib.rec_crossnet_vec_bwd_workspace_bytes(B, D, L), None, x0.device)
    _call("rec_crossnet_vec_bwd_f32", _ptr(x0), B, D, L, _ptr(w), _ptr(xs), _ptr(gy), _ptr(gx0), _ptr(dw), _ptr(db),
          _ptr(ws))
    return gx0, dw, db


def cosine_fwd(u, i):
    return tops.cosine_fwd(_f32(u, "u"), _f32(i, "i"))


def cosine_bwd(u, i, gout):
    return tops.cosine_bwd(u, i, _f32(gout, "gout"))


def bce_fwd_bwd(y, p, want_dp=True, want_dz=False):
    y = _f32(y.reshape(-1), "y")
    p = _f32(p.reshape(-1), "p")
    return tops.bce_fwd_bwd(y, p, bool(want_dp), bool(want_dz))


def adam_dense(var, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    """Keras' dense Adam apply on a contiguous parameter of any shape; m, v and g have that shape"""
    shape = tuple(_f32(var, "var").shape)
    for x, name in ((m, "m"), (v, "v"), (g, "g")):
        _expect(x, shape, name, "the shape of var")
    _call("rec_adam_dense_f32", _ptr(var), _ptr(m), _ptr(v), _ptr(g), var.numel(), t, lr, b1, b2, eps)


def _adam_rows_head(var, m, v, uniq_ids, g_rows, n_uniq):
    """The operands of a sparse Adam step: var a table [V,E] (a strided row view of the fused layout may be), m and v
    contiguous [V,E], g_rows [cap,E] the gradient rows of the int64 uniq_ids (cap ids or more), of which the int64
    device scalar n_uniq counts the used ones.  -> (V, E, cap)"""
    V, E = _table(var, "var").shape
    _expect(m, (V, E), "m", "[V,E]")
    _expect(v, (V, E), "v", "[V,E]")
    if _f32(g_rows, "g_rows").dim() != 2 or g_rows.shape[1] != E:
        raise ValueError("g_rows must be [cap,E] = (cap, %d), got %s" % (E, tuple(g_rows.shape)))
    cap = g_rows.shape[0]
    if _i64(uniq_ids, "uniq_ids").dim() != 1 or uniq_ids.numel() < cap:
        raise ValueError("uniq_ids must hold the [%d] ids of g_rows or more, got %s" % (cap, tuple(uniq_ids.shape)))
    if _i64(n_uniq, "n_uniq").numel() != 1:
        raise ValueError("n_uniq must be one int64 on the device, got %s" % (tuple(n_uniq.shape),))
    return V, E, cap


def adam_sparse_keras(var, m, v, uniq_ids, g_rows, n_uniq, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    V, E, cap = _adam_rows_head(var, m, v, uniq_ids, g_rows, n_uniq)
    side = _new((cap, 3, E), var.device)                 # the touched rows' new (var, m, v), patched in after the sweep
    _call("rec_adam_sparse_keras_f32", _ptr(var), var.stride(0), _ptr(m), _ptr(v), V, E, _ptr(uniq_ids), _ptr(g_rows),
          _ptr(n_uniq), cap, _ptr(side), t, lr, b1, b2, eps)


def adam_rows(var, m, v, uniq_ids, g_rows, n_uniq, t, lr, b1=0.9, b2=0.999, eps=1e-7):
    V, E, cap = _adam_rows_head(var, m, v, uniq_ids, g_rows, n_uniq)
    _call("rec_adam_rows_f32", _ptr(var), var.stride(0), _ptr(m), _ptr(v), V, E, _ptr(uniq_ids), _ptr(g_rows),
          _ptr(n_uniq), cap, t, lr, b1, b2, eps)


# ---------------------------------------------------------------------------------------------------
# sharding
# ---------------------------------------------------------------------------------------------------

def shard_bucketize(ids, rows_per_shard, n_shard, oob=None):
    ids = _i64(ids.reshape(-1), "ids")
    n = ids.numel()
    dev = ids.device
    perm, counts, local = (_new(k, dev, dtype=torch.int64) for k in (n, n_shard, n))
    _call_ws("rec_shard_bucketize_workspace_bytes", (n, n_shard), "rec_shard_bucketize_i64", dev, _ptr(ids), n,
             rows_per_shard, n_shard, _ptr(perm), _ptr(counts), _ptr(local), _ptr(oob), may_need_none=True)
    return perm, counts, local


def permute_rows(x, perm, scatter):
    """scatter=True: out[perm[i]] = x[i];  scatter=False: out[i] = x[perm[i]]."""
    n, E = _f32(x, "x").shape
    out = _new_like(x)
    _call("rec_permute_rows_f32", _ptr(x), _ptr(_i64(perm, "perm")), n, E, int(scatter), _ptr(out))
    return out


# ---------------------------------------------------------------------------------------------------
# retrieval
# ---------------------------------------------------------------------------------------------------
def l2_normalize_rows(x):
    """x / ||x||_2 per row (2.FM/OfflineLoader.py:140)."""
    _table(x, "x")                                       # 2-D fp32 CUDA, unit inner stride, any row stride
    y = _new(tuple(x.shape), x.device)
    _call("rec_l2_normalize_rows_f32", _ptr(x), x.shape[0], x.shape[1], x.stride(0), _ptr(y), y.stride(0))
    return y


def topk_l2(queries, items, k):
    """BallTree(items).query(queries, k) of the reference, brute force: (dist [nq,k] ascending, ind [nq,k] int64)."""
    _table(queries, "queries"); _table(items, "items")   # row views of wider buffers are fine
    if queries.shape[1] != items.shape[1]:
        raise ValueError("queries [nq,d] and items [n,d] must share d")
    nq, d = queries.shape
    n = items.shape[0]
    dev = queries.device
    ind, dist = _new((nq, k), dev, dtype=torch.int64), _new((nq, k), dev)
    _call_ws("rec_topk_l2_workspace_bytes", (nq, n, k), "rec_topk_l2_f32", dev, _ptr(queries), nq, d, queries.stride(0),
             _ptr(items), n, items.stride(0), k, _ptr(ind), _ptr(dist), may_need_none=True)
    return dist, ind


# ---------------------------------------------------------------------------------------------------
# DIN
# ---------------------------------------------------------------------------------------------------
DACT_NONE, DACT_RELU, DACT_SIGMOID, DACT_TANH, DACT_DICE, DACT_PRELU = (
    ENUMS["REC_DACT_" + k] for k in ("NONE", "RELU", "SIGMOID", "TANH", "DICE", "PRELU"))
DACT_CODE = {None: DACT_NONE, "linear": DACT_NONE, "relu": DACT_RELU, "sigmoid": DACT_SIGMOID, "tanh": DACT_TANH,
             "dice": DACT_DICE, "prelu": DACT_PRELU}


def din_prepare(W1, b1, D, H):
    """W1 [3D+D*D, H], b1 [H] -> Wcat [D, D*H+H], Wkd [D,H], bext [D*H+H]."""
    dev = W1.device
    N = D * H + H
    Wcat, Wkd, bext = _new((D, N), dev), _new((D, H), dev), _new(N, dev)
    _call("rec_din_prepare_f32", _ptr(_f32(W1, "W1")), _ptr(_f32(b1, "b1")), D, H, _ptr(Wcat), _ptr(Wkd), _ptr(bext))
    return Wcat, Wkd, bext


def din_prepare_bwd(gWcat, gWkd, D, H):
    gW1 = _new((3 * D + D * D, H), gWcat.device)
    _call("rec_din_prepare_bwd_f32", _ptr(_f32(gWcat, "gWcat")), _ptr(_f32(gWkd, "gWkd")), D, H, _ptr(gW1))
    return gW1


DIN_MAX_D, DIN_MAX_H, DIN_WIDE_D, DIN_WIDE_MAX_H = (LIMITS["REC_DIN_" + k] for k in ("MAX_D", "MAX_H", "WIDE_D",
                                                                                     "WIDE_MAX_H"))


def din_attn_check_shape(D, H):
    """Raises what rec_din_attn_fwd_f32 / _bwd_f32 would answer with -2, before anything is allocated or launched: key
    width D = E * C and hidden units H.  The envelope is the backward's and holds for the forward too."""
    if D > DIN_MAX_D or H > DIN_MAX_H or (D > DIN_WIDE_D and H > DIN_WIDE_MAX_H):
        raise NotImplementedError(
            "DIN attention kernels cover key width <= %d and hidden units <= %d, and beyond key width %d only hidden "
            "units <= %d; got key width=%d, hidden units=%d" % (DIN_MAX_D, DIN_MAX_H, DIN_WIDE_D, DIN_WIDE_MAX_H, D, H))


def _attn_common(embed, series, Mext, Wkd, act, alpha, mean, var, w2, b2, padding_index, mask_valid):
    _table(embed, "embed"); _i64(series, "series")
    V, E = embed.shape
    B, T, Cn = series.shape
    H = Wkd.shape[1]
    din_attn_check_shape(Cn * E, H)
    return [_ptr(embed), embed.stride(0), V, E, Cn, _ptr(series), B, T, _ptr(_f32(Mext, "Mext")), _ptr(_f32(Wkd, "Wkd")),
            H, act, _ptr(alpha), _ptr(mean), _ptr(var), _ptr(_f32(w2, "w2")), _ptr(_f32(b2, "b2")), int(padding_index),
            int(bool(mask_valid))], (B, T, Cn * E, H)


def din_attn_fwd(embed, series, Mext, Wkd, act, alpha, mean, var, w2, b2, padding_index, mask_valid, oob=None):
    args, (B, T, D, H) = _attn_common(embed, series, Mext, Wkd, act, alpha, mean, var, w2, b2, padding_index,
                                      mask_valid)
    scores, pooled = _new((B, T), embed.device), _new((B, D), embed.device)
    _call("rec_din_attn_fwd_f32", *args, _ptr(scores), _ptr(pooled), _ptr(oob))
    return scores, pooled


def din_attn_bwd(embed, series, Mext, Wkd, act, alpha, mean, var, w2, b2, padding_index, mask_valid, scores, gpooled,
                 gkeys=None, gscores=None):
    """``gkeys``: optional preallocated contiguous [B,T,D] destination (the tail of a shared value buffer).
    ``gscores``: optional [B,T] gradient at the raw scores, added to the one that arrives through pooled."""
    args, (B, T, D, H) = _attn_common(embed, series, Mext, Wkd, act, alpha, mean, var, w2, b2, padding_index,
                                      mask_valid)
    dev = embed.device
    _f32(scores, "scores"); _f32(gpooled, "gpooled")
    _expect(gscores, (B, T), "gscores", "[B,T]", optional=True)
    if gkeys is None:
        gkeys = _new((B, T, D), dev)
    _f32(gkeys, "gkeys")
    gMext, gw2p, galphap, gb2p = _new((B, D * H + H), dev), _new((B, H), dev), _new((B, H), dev), _new((B, 1), dev)
    _call("rec_din_attn_bwd_f32", *args, _ptr(scores), _ptr(gpooled), _ptr(gscores), _ptr(gkeys), _ptr(gMext),
          _ptr(gw2p), _ptr(galphap), _ptr(gb2p))
    return gkeys, gMext, gw2p, galphap, gb2p


def feat_act_fwd(kind, x, alpha=None, mean=None, var=None):
    M, N = _f32(x, "x").shape
    y = _new_like(x)
    _call("rec_feat_act_fwd_f32", kind, _ptr(x), _ptr(alpha), _ptr(mean), _ptr(var), _ptr(y), M, N)
    return y


def feat_act_bwd(kind, x, gy, alpha=None, mean=None, var=None, want_alpha=False):
    M, N = x.shape
    _f32(gy, "gy")
    gx = _new_like(x)
    ga = _new_like(x) if want_alpha else None
    _call("rec_feat_act_bwd_f32", kind, _ptr(x), _ptr(gy), _ptr(alpha), _ptr(mean), _ptr(var), _ptr(gx), _ptr(ga), M, N)
    return gx, ga


def layernorm_fwd(x, gamma, beta, epsilon=None):
    """``epsilon`` None: Keras' default 1e-3 through the entry point that fixes it; a given one is a positive float"""
    M, N = _f32(x, "x").shape
    _f32(gamma, "gamma"); _f32(beta, "beta")
    y, xhat, rstd = _new_like(x), _new_like(x), _new(M, x.device)
    if epsilon is None:
        _call("rec_layernorm_fwd_f32", _ptr(x), _ptr(gamma), _ptr(beta), M, N, _ptr(y), _ptr(xhat), _ptr(rstd))
    else:
        _call("rec_layernorm_eps_fwd_f32", _ptr(x), _ptr(gamma), _ptr(beta), M, N, float(epsilon), _ptr(y), _ptr(xhat),
              _ptr(rstd))
    return y, xhat, rstd


def layernorm_bwd(gy, xhat, rstd, gamma):
    M, N = _f32(gy, "gy").shape
    gx, gg = _new_like(gy), _new_like(gy)
    _call("rec_layernorm_bwd_f32", _ptr(gy), _ptr(xhat), _ptr(rstd), _ptr(gamma), M, N, _ptr(gx), _ptr(gg))
    return gx, gg


def softmax_fwd(x):
    M, N = _f32(x, "x").shape
    y = _new_like(x)
    _call("rec_softmax_fwd_f32", _ptr(x), M, N, _ptr(y))
    return y


def softmax_bwd(y, gy):
    M, N = y.shape
    _f32(gy, "gy")
    gx = _new_like(y)
    _call("rec_softmax_bwd_f32", _ptr(y), _ptr(gy), M, N, _ptr(gx))
    return gx


# ---------------------------------------------------------------------------------------------------
# f4: sibling interaction layers on the same gather (PNN inner product, NFM bi-interaction, SIM GSU attention)
# ---------------------------------------------------------------------------------------------------

def emb_ipn_fwd(table, X, oob=None):
    """[Flatten(embed(X)) | <e_i,e_j> for i<j]  ->  [B, F*E + F(F-1)/2]  (2.FM/CustomLayers.py:737-745,755-792)."""
    _table(table, "table"); _i64(X, "X")
    V, E = table.shape
    B, F = X.shape
    W = F * E + F * (F - 1) // 2
    out = _new((B, W), table.device)
    _call("rec_emb_ipn_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, _ptr(out), W, _ptr(oob))
    return out


def emb_ipn_bwd_vals(out, g, F, E):
    _f32(out, "out"); _f32(g, "g")
    B, W = out.shape
    vals = _new((B * F, E), out.device)
    _call("rec_emb_ipn_bwd_vals_f32", _ptr(out), W, _ptr(g), g.shape[1], B, F, E, _ptr(vals))
    return vals


def emb_bi_fwd(table, X, out=None, oob=None):
    """NFM bi-interaction 0.5*((sum e)^2 - sum e^2) -> the leading E columns of `out` (a [B, >=E] fp32 buffer, fresh
    [B,E] when None) and sumvec [B,E]."""
    _table(table, "table"); _i64(X, "X")
    V, E = table.shape
    B, F = X.shape
    if out is None:
        out = _new((B, E), table.device)
    _f32(out, "out")
    S = _new((B, E), table.device)
    _call("rec_emb_bi_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, _ptr(out), out.shape[1], _ptr(S),
          _ptr(oob))
    return out, S


def emb_bi_bwd_vals(table, X, g, S):
    """g: [B, >=E] (only the leading E columns are read)."""
    _table(table, "table"); _i64(X, "X"); _f32(g, "g"); _f32(S, "S")
    V, E = table.shape
    B, F = X.shape
    vals = _new((B * F, E), table.device)
    _call("rec_emb_bi_bwd_vals_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, _ptr(g), g.shape[1], _ptr(S),
          _ptr(vals))
    return vals


def batchnorm_fwd(x, gamma, beta, moving_mean, moving_var, training, eps=1e-3, momentum=0.99, save=True):
    """Keras BatchNormalization on [B,N]; moving statistics are updated in place when training."""
    _f32(x, "x")
    B, N = x.shape
    y = _new_like(x)
    xhat = _new_like(x) if save else None
    rstd = _new(N, x.device) if save else None
    ws = _workspace(lib.rec_batchnorm_workspace_bytes(B, N), None, x.device)
    _call("rec_batchnorm_fwd_f32", _ptr(x), N, B, N, _ptr(gamma), _ptr(beta), float(eps), float(momentum),
          1 if training else 0, _ptr(moving_mean), _ptr(moving_var), _ptr(y), _ptr(xhat), _ptr(rstd), _ptr(ws))
    return y, xhat, rstd


def batchnorm_bwd(g, xhat, rstd, gamma, training):
    _f32(g, "g")
    B, N = g.shape
    gx, ggamma, gbeta = _new_like(g), _new(N, g.device, B), _new(N, g.device, B)
    ws = _workspace(lib.rec_batchnorm_workspace_bytes(B, N), None, g.device)
    _call("rec_batchnorm_bwd_f32", _ptr(g), _ptr(xhat), _ptr(rstd), B, N, _ptr(gamma), 1 if training else 0, _ptr(gx),
          _ptr(ggamma), _ptr(gbeta), _ptr(ws))
    return gx, ggamma, gbeta


def ffm_fwd(v, w, bias, X, want_prob=False, oob=None):
    """v [V,F,E] field-aware table, w [V,1], bias [1], X [B,F] -> z [B] (and prob [B])."""
    _f32(v, "v"); _table(w, "w"); _f32(bias, "bias"); _i64(X, "X")
    V, F, E = v.shape
    B = X.shape[0]
    if X.shape[1] != F:
        raise ValueError("X has %d fields, the table %d" % (X.shape[1], F))
    z = _new(B, v.device)
    prob = _new(B, v.device) if want_prob else None
    _call("rec_ffm_fwd_f32", _ptr(v), F * E, _ptr(w), w.stride(0), _ptr(bias), V, E, _ptr(X), B, F, _ptr(z), _ptr(prob),
          _ptr(oob))
    return z, prob


def ffm_bwd_rows(v, X, gz, plan):
    """-> g_rows [B*F, F, E] aligned with plan.uniq_ids (zero beyond n_uniq)."""
    _f32(v, "v"); _i64(X, "X"); _f32(gz, "gz")
    V, F, E = v.shape
    B = X.shape[0]
    rows = _new((max(B * F, 1), F, E), v.device)
    _call("rec_ffm_bwd_rows_f32", _ptr(v), F * E, V, E, _ptr(X), B, F, _ptr(gz), _ptr(plan.perm), _ptr(plan.seg_start),
          _ptr(plan.n_uniq), _ptr(rows))
    return rows


# ---- xDeepFM CIN (csrc/cin.hip)
CIN_MAX_F, CIN_MAX_E, CIN_MAX_L, CIN_MAX_H = (LIMITS["REC_CIN_MAX_" + d] for d in "FELH")


def cin_check_shape(F, E, cin_size):
    """NotImplementedError for shapes the CIN kernels do not cover (the ABI would return -2)."""
    L = len(cin_size)
    if not (1 <= F <= CIN_MAX_F and 1 <= E <= CIN_MAX_E and 1 <= L <= CIN_MAX_L
            and all(1 <= int(h) <= CIN_MAX_H for h in cin_size)):
        raise NotImplementedError(
            "CIN kernels cover 1 <= fields <= %d, 1 <= embedding_dims <= %d, 1 <= len(cin_size) <= %d and "
            "1 <= cin_size[k] <= %d; got fields=%d, embedding_dims=%d, cin_size=%s"
            % (CIN_MAX_F, CIN_MAX_E, CIN_MAX_L, CIN_MAX_H, F, E, list(cin_size)))


def _cin_args(x0, Ws):
    B, F, E = x0.shape
    H = [int(w.shape[-1]) for w in Ws]
    cin_check_shape(F, E, H)
    for k, w in enumerate(Ws):
        _f32(w, "W%d" % k)
    return B, F, E, H, _ints(H), _ptr_array(Ws)


def cin_fwd(x0, Ws):
    """x0 [B,F,E], Ws: the L CIN weights (1, F*H_k, H_{k+1}) -> (cin_part [B, sum H], states [B, sum H, E]).  An empty
    batch is an error of the entry point (REC_E_ARG), unlike every other family's."""
    _f32(x0, "x0")
    B, F, E, H, Hh, Wh = _cin_args(x0, Ws)
    SH = sum(H)
    states, cin_part = _new((B, SH, E), x0.device), _new((B, SH), x0.device)
    _call("rec_cin_fwd_f32", _ptr(x0), B, F, E, len(H), Hh, Wh, _ptr(states), _ptr(cin_part))
    return cin_part, states


def cin_bwd(x0, states, g, Ws):
    """-> (dx0 [B,F,E], [dW_k] shaped as Ws) from g = dLoss/dcin_part [B, sum H]."""
    B, F, E, H, Hh, Wh = _cin_args(x0, Ws)
    _f32(states, "states")
    _f32(g, "g")
    dx0 = _new_like(x0)
    dWs = [_new_like(w) for w in Ws]
    _call_ws("rec_cin_workspace_bytes", (B, F, E, len(H), Hh), "rec_cin_bwd_f32", x0.device, _ptr(x0), _ptr(states),
             _ptr(g), B, F, E, len(H), Hh, Wh, _ptr(dx0), _ptr_array(dWs))
    return dx0, dWs


# ---- FiBiNet SENet + bilinear interaction (csrc/fibinet.hip)
FIBINET_MAX_F, FIBINET_MAX_E, FIBINET_MAX_C = (LIMITS["REC_FIBINET_MAX_" + d] for d in "FEC")
FIBINET_TYPES = {k: ENUMS["REC_FIBINET_TYPE_" + k.upper()] for k in ("all", "each", "interaction")}


def fibinet_num_weights(F, bilinear_type):
    """Bilinear matrices of one layer: 1 ('all'), F-1 ('each'), F(F-1)/2 ('interaction')."""
    return {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[bilinear_type]


def fibinet_check_shape(F, E, C, mid):
    """NotImplementedError for shapes the FiBiNet kernels do not cover (the ABI would return -2)."""
    if not (2 <= F <= FIBINET_MAX_F and 1 <= E <= FIBINET_MAX_E and 0 <= C <= FIBINET_MAX_C and 1 <= mid <= F):
        raise NotImplementedError(
            "FiBiNet kernels cover 2 <= fields <= %d, 1 <= embedding_dims <= %d, 0 <= continuous features <= %d and "
            "1 <= SENet units <= fields; got fields=%d, embedding_dims=%d, continuous=%d, SENet units=%d"
            % (FIBINET_MAX_F, FIBINET_MAX_E, FIBINET_MAX_C, F, E, C, mid))


def fibinet_fwd(x_emb, x_cont, S0, S1, W, type_code):
    """x_emb [B,F,E], x_cont [B,C], S0 [F,mid], S1 [mid,F], W [nW,E,E] -> (dnn_in [B, 2PE + C], A [B,F], H1 [B,mid])."""
    _f32(x_emb, "x_emb"); _f32(x_cont, "x_cont"); _f32(S0, "S0"); _f32(S1, "S1"); _f32(W, "W")
    B, F, E = x_emb.shape
    C, mid = x_cont.shape[1], S0.shape[1]
    fibinet_check_shape(F, E, C, mid)
    P = F * (F - 1) // 2
    dev = x_emb.device
    dnn_in, A, H1 = _new((B, 2 * P * E + C), dev), _new((B, F), dev), _new((B, mid), dev)
    if B > 0:
        _call("rec_fibinet_fwd_f32", _ptr(x_emb), _ptr(x_cont) if C > 0 else None, _ptr(S0), _ptr(S1), _ptr(W), B, F, E,
              C, mid, type_code, _ptr(dnn_in), _ptr(A), _ptr(H1))
    return dnn_in, A, H1


def fibinet_bwd(x_emb, g, A, H1, S0, S1, W, type_code):
    """-> (dx_emb [B,F,E], dW [nW,E,E], dS0, dS1) from g = dLoss/d dnn_in [B, 2PE + C]."""
    _f32(x_emb, "x_emb"); _f32(g, "g"); _f32(A, "A"); _f32(H1, "H1"); _f32(S0, "S0"); _f32(S1, "S1"); _f32(W, "W")
    B, F, E = x_emb.shape
    mid = S0.shape[1]
    C = g.shape[1] - F * (F - 1) * E
    fibinet_check_shape(F, E, C, mid)
    dx, dW, dS0, dS1 = _new_like(x_emb), _new_like(W, B), _new_like(S0, B), _new_like(S1, B)
    if B > 0:
        _call_ws("rec_fibinet_workspace_bytes", (B, F, E, mid, type_code), "rec_fibinet_bwd_f32", x_emb.device,
                 _ptr(x_emb), _ptr(g), _ptr(A), _ptr(H1), _ptr(S0), _ptr(S1), _ptr(W), B, F, E, C, mid, type_code,
                 _ptr(dx), _ptr(dW), _ptr(dS0), _ptr(dS1))
    return dx, dW, dS0, dS1


# ---- AutoInt multi-head field attention (csrc/autoint.hip)
AUTOINT_MAX_F, AUTOINT_MAX_E = (LIMITS["REC_AUTOINT_MAX_" + d] for d in "FE")
AUTOINT_RES = {key: ENUMS["REC_AUTOINT_RES_" + k] for key, k in (                       # (use_res, res_learnable)
    ((False, False), "NONE"), ((False, True), "NONE"), ((True, False), "ADD"), ((True, True), "LEARNED"))}


def autoint_check_shape(F, E, H, C=0):
    """NotImplementedError for shapes the AutoInt kernels do not cover (the ABI would return -2); ValueError when the
    embedding width does not split into the heads (the reference asserts E % H == 0)."""
    if H >= 1 and E % H != 0:
        raise ValueError("embedding_dims=%d is not divisible by num_heads=%d" % (E, H))
    if not (1 <= F <= AUTOINT_MAX_F and 1 <= E <= AUTOINT_MAX_E and 1 <= H <= E and 0 <= C < F):
        raise NotImplementedError(
            "AutoInt kernels cover 1 <= fields <= %d, 1 <= embedding_dims <= %d, 1 <= num_heads <= embedding_dims and "
            "fewer continuous than total fields; got fields=%d, embedding_dims=%d, num_heads=%d, continuous=%d"
            % (AUTOINT_MAX_F, AUTOINT_MAX_E, F, E, H, C))


def autoint_fwd(x, Wq, Wk, Wv, Wres, num_heads, res, scaling, x_cont=None, cemb=None, want_o=False):
    """One attention layer.  x [B,Fc,E] (plus C continuous fields cemb[c] * x_cont[:, c] appended last when x_cont
    [B,C] and cemb [C,E] are given), W* [E,E] (Wres only for res == 2) -> (y [B,F,E], stats [2,H,F,F], o [B,F,E] or
    None).  res: 0 none, 1 + X, 2 + X Wres.  The softmax runs over the batch axis (see csrc/autoint.hip)."""
    for t, n in ((x, "x"), (Wq, "Wq"), (Wk, "Wk"), (Wv, "Wv")):
        _f32(t, n)
    B, Fc, E = x.shape
    C = 0 if x_cont is None else x_cont.shape[1]
    if C:
        _expect(x_cont, (B, C), "x_cont", "[B,C]"); _expect(cemb, (C, E), "cemb", "[C,E]")
    else:
        x_cont = cemb = None
    if res == 2:
        _f32(Wres, "Wres")
    else:
        Wres = None
    F, H = Fc + C, int(num_heads)
    autoint_check_shape(F, E, H, C)
    _expect_all([(t, (E, E), n) for t, n in ((Wq, "Wq"), (Wk, "Wk"), (Wv, "Wv"), (Wres, "Wres")) if t is not None])
    dev = x.device
    y = _new((B, F, E), dev)
    o = _new((B, F, E), dev) if want_o else None
    stats = _new((2, H, F, F), dev, B)
    if B > 0:
        _call_ws("rec_autoint_workspace_bytes", (B, F, E, H, C, res), "rec_autoint_fwd_f32", dev, _ptr(x), _ptr(x_cont),
                 _ptr(cemb), _ptr(Wq), _ptr(Wk), _ptr(Wv), _ptr(Wres), B, F, E, H, C, res, int(bool(scaling)), _ptr(y),
                 _ptr(o), _ptr(stats))
    return y, stats, o


def autoint_bwd(x, Wq, Wk, Wv, Wres, y, dy, stats, num_heads, res, scaling, x_cont=None, cemb=None):
    """-> (dx [B,Fc,E], dWq, dWk, dWv, dWres (res == 2, else None), dcemb [C,E] (C > 0, else None))."""
    for t, n in ((x, "x"), (Wq, "Wq"), (Wk, "Wk"), (Wv, "Wv")):
        _f32(t, n)
    B, Fc, E = x.shape
    C = 0 if x_cont is None else x_cont.shape[1]
    if not C:
        x_cont = cemb = None
    if res != 2:
        Wres = None
    F, H = Fc + C, int(num_heads)
    autoint_check_shape(F, E, H, C)
    _expect_all([(y, (B, F, E), "y"), (dy, (B, F, E), "dy"), (stats, (2, H, F, F), "stats")])
    dev = x.device
    dx = _new_like(x)
    dWq, dWk, dWv = (torch.zeros((E, E), dtype=torch.float32, device=dev) for _ in range(3))
    dWres = torch.zeros((E, E), dtype=torch.float32, device=dev) if res == 2 else None
    dcemb = torch.zeros((C, E), dtype=torch.float32, device=dev) if C else None
    if B > 0:
        _call_ws("rec_autoint_workspace_bytes", (B, F, E, H, C, res), "rec_autoint_bwd_f32", dev, _ptr(x), _ptr(x_cont),
                 _ptr(cemb), _ptr(Wq), _ptr(Wk), _ptr(Wv), _ptr(Wres), _ptr(y), _ptr(dy), _ptr(stats), B, F, E, H, C,
                 res, int(bool(scaling)), _ptr(dx), _ptr(dWq), _ptr(dWk), _ptr(dWv), _ptr(dWres), _ptr(dcemb))
    return dx, dWq, dWk, dWv, dWres, dcemb


# ---- Attentional FM, fused with the lookup (csrc/afm.hip)
AFM_MAX_F, AFM_MAX_E, AFM_MAX_A = (LIMITS["REC_AFM_MAX_" + d] for d in "FEA")


def afm_check_shape(F, E, A):
    """NotImplementedError for shapes the AFM kernels do not cover (the ABI would return -2)."""
    if not (2 <= F <= AFM_MAX_F and 1 <= E <= AFM_MAX_E and 1 <= A <= AFM_MAX_A):
        raise NotImplementedError(
            "AFM kernels cover 2 <= fields <= %d, 1 <= embedding_dims <= %d and 1 <= attn_size <= %d; got fields=%d, "
            "embedding_dims=%d, attn_size=%d" % (AFM_MAX_F, AFM_MAX_E, AFM_MAX_A, F, E, A))


def _afm_params(E, Wa, ba, hv, bh):
    for t, n in ((Wa, "Wa"), (ba, "ba"), (hv, "hv"), (bh, "bh")):
        _f32(t, n)
    A = Wa.shape[1]
    if Wa.dim() != 2 or Wa.shape[0] != E or ba.numel() != A or hv.numel() != A or bh.numel() != 1:
        raise ValueError("attention weights must be Wa [E,A], ba [A], hv [A,1], bh [1] with E = %d, got %s %s %s %s"
                         % (E, tuple(Wa.shape), tuple(ba.shape), tuple(hv.shape), tuple(bh.shape)))
    return A


def emb_afm_fwd(table, X, Wa, ba, hv, bh, oob=None, want_rows=False):
    """Lookup + pairwise products + attention pooling in one launch: -> (o [B,E], stats [B,2] = (max, sum exp) of the
    pair softmax, rows [B,F,E] or None)."""
    _table(table, "table"); _i64(X, "X")
    V, E = table.shape
    B, F = X.shape
    A = _afm_params(E, Wa, ba, hv, bh)
    afm_check_shape(F, E, A)
    dev = table.device
    o, stats = _new((B, E), dev), _new((B, 2), dev)
    rows = _new((B, F, E), dev) if want_rows else None
    _call("rec_emb_afm_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, A, _ptr(Wa), _ptr(ba), _ptr(hv),
          _ptr(bh), _ptr(o), _ptr(stats), _ptr(rows), _ptr(oob))
    return o, stats, rows


def emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, dout, rows=None):
    """-> (vals [B*F,E] IndexedSlices values in the order of X, dWa [E,A], dba [A], dhv (shape of hv), dbh [1]).  With
    the forward's ``rows`` the table is not read again."""
    _table(table, "table"); _i64(X, "X")
    V, E = table.shape
    B, F = X.shape
    A = _afm_params(E, Wa, ba, hv, bh)
    afm_check_shape(F, E, A)
    _expect_all([(o, (B, E), "o"), (stats, (B, 2), "stats"), (dout, (B, E), "dout")])
    _expect(rows, (B, F, E), "rows", "[B,F,E]", optional=True)
    dev = table.device
    vals = _new((B * F, E), dev)
    dWa, dba, dhv, dbh = (torch.zeros_like(t) for t in (Wa, ba, hv, bh))
    if B > 0:
        _call_ws("rec_afm_workspace_bytes", (B, F, E, A), "rec_emb_afm_bwd_f32", dev, _ptr(table), V, E, table.stride(0),
                 _ptr(X), B, F, A, _ptr(Wa), _ptr(ba), _ptr(hv), _ptr(bh), _ptr(o), _ptr(stats), _ptr(rows), _ptr(dout),
                 _ptr(vals), _ptr(dWa), _ptr(dba), _ptr(dhv), _ptr(dbh))
    return vals, dWa, dba, dhv, dbh


# ---- field-conv stacks: what CCPM and FGCNN share (csrc/field_conv.h): the limits and the flat K_1 | b_1 | K_2 | ...
_FIELD_CONV_MAX = [LIMITS["REC_FIELD_CONV_MAX_" + d] for d in ("F", "E", "L", "C", "KW")]
CCPM_MAX_F, CCPM_MAX_E, CCPM_MAX_L, CCPM_MAX_C, CCPM_MAX_KW = _FIELD_CONV_MAX       # fields, embedding_dims, layers,
FGCNN_MAX_F, FGCNN_MAX_E, FGCNN_MAX_L, FGCNN_MAX_C, FGCNN_MAX_KW = _FIELD_CONV_MAX  # filters, kernel_width


def field_conv_param_count(filters, kernel_width):
    cins = [1] + list(filters[:-1])
    return sum(kw * cin * c + c for kw, cin, c in zip(kernel_width, cins, filters))


def _field_conv_params(params, filters, kernel_width):
    n = field_conv_param_count(filters, kernel_width)
    if _f32(params, "params").numel() != n:
        raise ValueError("params must hold %d floats for filters %r and kernel_width %r, got %d"
                         % (n, list(filters), list(kernel_width), params.numel()))


# ---- CCPM: field convolutions + k-max pooling, fused with the lookup (csrc/ccpm.hip)
def ccpm_k(E, L):
    """The k of every KMaxPool of CCPMBaseLayer.build (3.DCN/CustomLayers.py:657-667), the expression as written.  Its
    ``fields_num`` is input_shape[-1], the EMBEDDING width, not the field count: a reference quirk that is kept."""
    fields_num = int(E)
    layers_num = int(L)
    return [max(1, int((1 - pow(j / layers_num, layers_num - j)) * fields_num)) if j < layers_num else 3
            for j in range(1, layers_num + 1)]


def ccpm_check_shape(F, E, filters, kernel_width):
    """ValueError for a configuration the reference itself cannot run (a KMaxPool whose k exceeds the height it pools:
    tf.nn.top_k raises), NotImplementedError for shapes the CCPM kernels do not cover (the ABI would return -2)."""
    filters, kernel_width = [int(c) for c in filters], [int(k) for k in kernel_width]
    if len(filters) != len(kernel_width) or len(filters) < 1:
        raise ValueError("filters and kernel_width must be lists of one length >= 1, got %r and %r"
                         % (filters, kernel_width))
    if min(filters) < 1 or min(kernel_width) < 1 or F < 1 or E < 1:
        raise ValueError("fields, embedding_dims, filters and kernel_width must be positive")
    ks, h = ccpm_k(E, len(filters)), F
    for j, k in enumerate(ks):
        if k > h:
            raise ValueError("KMaxPool %d takes k = %d of %d values (k comes from embedding_dims = %d, fields = %d): "
                             "tf.nn.top_k raises" % (j + 1, k, h, E, F))
        h = k
    if lib.rec_ccpm_workspace_bytes(1, F, E, len(filters), _ints(filters), _ints(kernel_width), _ints(ks)) == 0:
        raise NotImplementedError(
            "CCPM kernels cover fields <= %d, embedding_dims <= %d, at most %d layers, filters <= %d, kernel_width <= %d "
            "and a column state within the LDS of a CU; got fields=%d, embedding_dims=%d, filters=%r, kernel_width=%r"
            % (CCPM_MAX_F, CCPM_MAX_E, CCPM_MAX_L, CCPM_MAX_C, CCPM_MAX_KW, F, E, filters, kernel_width))
    return ks


def emb_ccpm_fwd(table, X, params, filters, kernel_width, oob=None, want_rows=False):
    """Lookup + L x (field conv, tanh, k-max pool) + Flatten in one launch: params is the flat K_1 | b_1 | K_2 | ...
    -> (out [B, 3 E C_L], rows [B,F,E] or None)."""
    _table(table, "table"); _i64(X, "X"); _f32(params, "params")
    V, E = table.shape
    B, F = X.shape
    ks = ccpm_check_shape(F, E, filters, kernel_width)
    _field_conv_params(params, filters, kernel_width)
    dev = table.device
    out = _new((B, ks[-1] * E * int(filters[-1])), dev)
    rows = _new((B, F, E), dev) if want_rows else None
    _call("rec_emb_ccpm_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, len(ks), _ints(filters),
          _ints(kernel_width), _ints(ks), _ptr(params), _ptr(out), _ptr(rows), _ptr(oob))
    return out, rows


def emb_ccpm_bwd(table, X, params, filters, kernel_width, dout, rows=None):
    """-> (vals [B*F,E] IndexedSlices values in the order of X, dparams in the layout of params).  With the forward's
    ``rows`` the table is not read again."""
    _table(table, "table"); _i64(X, "X"); _f32(params, "params"); _f32(dout, "dout")
    V, E = table.shape
    B, F = X.shape
    ks = ccpm_check_shape(F, E, filters, kernel_width)
    _field_conv_params(params, filters, kernel_width)
    _expect(dout, (B, ks[-1] * E * int(filters[-1])), "dout", "[B, k_L E C_L]")
    _expect(rows, (B, F, E), "rows", "[B,F,E]", optional=True)
    dev = table.device
    vals = _new((B * F, E), dev)
    dparams = torch.zeros_like(params)
    if B > 0:
        stack = (len(ks), _ints(filters), _ints(kernel_width), _ints(ks))
        _call_ws("rec_ccpm_workspace_bytes", (B, F, E, *stack), "rec_emb_ccpm_bwd_f32", dev, _ptr(table), V, E,
                 table.stride(0), _ptr(X), B, F, *stack, _ptr(params), _ptr(rows), _ptr(dout), _ptr(vals), _ptr(dparams))
    return vals, dparams


# ---- FGCNN: field convolutions + max pooling, every pooled map an output, fused with the lookup (csrc/fgcnn.hip)
FGCNN_MAX_PW = LIMITS["REC_FGCNN_MAX_PW"]
FGCNN_BWD_GRID = LIMITS["REC_FIELD_CONV_BWD_GRID"]   # workgroups of the backward: beyond it a workgroup takes a second tile


def fgcnn_heights(F, pooling_width):
    """H_1..H_L of the pooled maps: MaxPool2D((pw, 1)) with stride pw and VALID padding keeps H // pw rows."""
    out, h = [], int(F)
    for pw in pooling_width:
        h = h // int(pw)
        out.append(h)
    return out


def fgcnn_dense_units(F, E, dnn_maps, pooling_width):
    """The units of every recombination Dense of FGCNNBaseLayer.build (3.DCN/CustomLayers.py:752-754), the expression
    as written: from the ORIGINAL field count at every layer, not from the height that layer pools: a reference quirk
    that is kept."""
    return [int(m) * int(F) * int(E) // int(pw) for m, pw in zip(dnn_maps, pooling_width)]


def fgcnn_check_shape(F, E, filters, kernel_width, pooling_width, dnn_maps=None):
    """ValueError for a configuration the reference itself cannot run (a pooling that leaves no row; with ``dnn_maps``, a
    Dense whose units the reshape to [-1, N, E] cannot split), NotImplementedError for shapes the FGCNN kernels do not
    cover (the ABI would return -2).  -> the heights H_1..H_L."""
    filters, kernel_width = [int(c) for c in filters], [int(k) for k in kernel_width]
    pooling_width = [int(w) for w in pooling_width]
    L = len(filters)
    if L < 1 or len(kernel_width) != L or len(pooling_width) != L or (dnn_maps is not None and len(dnn_maps) != L):
        raise ValueError("filters, kernel_width, dnn_maps and pooling_width must be lists of one length >= 1, got %r, "
                         "%r, %r and %r" % (filters, kernel_width, dnn_maps, pooling_width))
    if min(filters) < 1 or min(kernel_width) < 1 or min(pooling_width) < 1 or F < 1 or E < 1:
        raise ValueError("fields, embedding_dims, filters, kernel_width and pooling_width must be positive")
    heights = fgcnn_heights(F, pooling_width)
    for j, h in enumerate(heights):
        if h < 1:
            raise ValueError("MaxPool2D %d (pooling_width %d) leaves no row of %d: heights %r from %d fields"
                             % (j + 1, pooling_width[j], ([F] + heights)[j], heights, F))
    if dnn_maps is not None:
        for j, u in enumerate(fgcnn_dense_units(F, E, dnn_maps, pooling_width)):
            if u < 1 or u % E:
                raise ValueError("Dense %d has %d units (dnn_maps %d x %d fields x %d // pooling_width %d), which the "
                                 "reshape to [-1, N, %d] cannot split" % (j + 1, u, dnn_maps[j], F, E, pooling_width[j], E))
    if lib.rec_fgcnn_workspace_bytes(1, F, E, L, _ints(filters), _ints(kernel_width), _ints(pooling_width)) == 0:
        raise NotImplementedError(
            "FGCNN kernels cover fields <= %d, embedding_dims <= %d, at most %d layers, filters <= %d, kernel_width <= "
            "%d, pooling_width <= %d and a column state within the LDS of a CU; got fields=%d, embedding_dims=%d, "
            "filters=%r, kernel_width=%r, pooling_width=%r"
            % (FGCNN_MAX_F, FGCNN_MAX_E, FGCNN_MAX_L, FGCNN_MAX_C, FGCNN_MAX_KW, FGCNN_MAX_PW, F, E, filters,
               kernel_width, pooling_width))
    return heights


def emb_fgcnn_fwd(table, X, params, filters, kernel_width, pooling_width, oob=None):
    """Lookup + L x (field conv, tanh, max pool) in one launch: params is the flat K_1 | b_1 | K_2 | ... -> (rows
    [B,F,E], [p_1 .. p_L]) with p_j [B, H_j E C_j] the Flatten of the j-th pooled map."""
    _table(table, "table"); _i64(X, "X")
    V, E = table.shape
    B, F = X.shape
    hs = fgcnn_check_shape(F, E, filters, kernel_width, pooling_width)
    _field_conv_params(params, filters, kernel_width)
    dev = table.device
    rows = _new((B, F, E), dev)
    pooled = [_new((B, h * E * int(c)), dev) for h, c in zip(hs, filters)]
    _call("rec_emb_fgcnn_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), B, F, len(hs), _ints(filters),
          _ints(kernel_width), _ints(pooling_width), _ptr(params), _ptr(rows), _ptr_array(pooled), _ptr(oob))
    return rows, pooled


def emb_fgcnn_bwd(rows, params, filters, kernel_width, pooling_width, dpooled, drows_direct=None):
    """rows [B,F,E] as the forward gathered them, dpooled = [dLoss/dp_1 .. dLoss/dp_L], drows_direct = dLoss/drows from
    the other consumers of the rows (None: zeros) -> (vals [B*F,E] IndexedSlices values in the order of X, the direct
    gradient included, dparams in the layout of params)."""
    _f32(rows, "rows")
    if rows.dim() != 3:
        raise ValueError("rows must be [B,F,E]")
    B, F, E = rows.shape
    hs = fgcnn_check_shape(F, E, filters, kernel_width, pooling_width)
    _field_conv_params(params, filters, kernel_width)
    if len(dpooled) != len(hs):
        raise ValueError("dpooled must hold %d tensors, got %d" % (len(hs), len(dpooled)))
    _expect_all([(d, (B, h * E * int(c)), "dpooled[%d]" % j) for j, (d, h, c) in enumerate(zip(dpooled, hs, filters))])
    _expect(drows_direct, (B, F, E), "drows_direct", "[B,F,E]", optional=True)
    dev = rows.device
    vals = _new((B * F, E), dev)
    dparams = torch.zeros_like(params)
    if B > 0:
        stack = (len(hs), _ints(filters), _ints(kernel_width), _ints(pooling_width))
        _call_ws("rec_fgcnn_workspace_bytes", (B, F, E, *stack), "rec_emb_fgcnn_bwd_f32", dev, E, B, F, *stack,
                 _ptr(params), _ptr(rows), _ptr_array(dpooled), _ptr(drows_direct), _ptr(vals), _ptr(dparams))
    return vals, dparams


# ---- MaskNet: lookup + per-field LayerNorm, and the mask block (csrc/masknet.hip)
MASKNET_MAX_F, MASKNET_MAX_E, MASKNET_MAX_D, MASKNET_MAX_P, MASKNET_MAX_O, MASKNET_MAX_R = (
    LIMITS["REC_MASKNET_MAX_" + d] for d in "FEDPOR")


def masknet_ln_check_shape(F, E, Fk=0):
    """ValueError for sizes that describe no input stage, NotImplementedError for shapes the kernels do not cover (the
    ABI would return -2)."""
    if F < 1 or E < 1 or not 0 <= Fk <= F:
        raise ValueError("fields and embedding_dims must be positive and 0 <= continuous fields <= fields, got fields=%d, "
                         "embedding_dims=%d, continuous=%d" % (F, E, Fk))
    if F > MASKNET_MAX_F or E > MASKNET_MAX_E:
        raise NotImplementedError("MaskNet input-stage kernels cover fields <= %d and embedding_dims <= %d; got "
                                  "fields=%d, embedding_dims=%d" % (MASKNET_MAX_F, MASKNET_MAX_E, F, E))


def mask_block_check_shape(D, P, O, R):
    """The same for one mask block: x_emb width D, guided width P, output width O, reduction rate R."""
    if min(D, P, O, R) < 1:
        raise ValueError("mask block sizes must be positive, got D=%d, P=%d, O=%d, R=%d" % (D, P, O, R))
    if D > MASKNET_MAX_D or P > MASKNET_MAX_P or O > MASKNET_MAX_O or R > MASKNET_MAX_R:
        raise NotImplementedError(
            "mask-block kernels cover D <= %d, P <= %d, block_output_dim <= %d and reduction_rate <= %d; got D=%d, P=%d, "
            "block_output_dim=%d, reduction_rate=%d"
            % (MASKNET_MAX_D, MASKNET_MAX_P, MASKNET_MAX_O, MASKNET_MAX_R, D, P, O, R))


def emb_masknet_ln_fwd(table, X, values, gamma, beta, oob=None):
    """Lookup (the last ``values.shape[1]`` columns of X are the keys of continuous features, their rows scaled by
    ``values``) + one LayerNorm per field in one launch -> (x_emb [B, F E], x_norm [B, F E], stats [B, F, 2])."""
    V, E = _table(table, "table").shape
    B, F, E, Fk = _keyed_head(X, values, E)
    masknet_ln_check_shape(F, E, Fk)
    _expect(gamma, (F, E), "gamma", "[fields, embedding_dims]")
    _expect(beta, (F, E), "beta", "[fields, embedding_dims]", optional=True)
    dev = table.device
    x_emb, x_norm, stats = _new((B, F * E), dev), _new((B, F * E), dev), _new((B, F, 2), dev)
    _call("rec_emb_masknet_ln_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), _ptr(values), B, F, Fk, _ptr(gamma),
          _ptr(beta), _ptr(x_emb), _ptr(x_norm), _ptr(stats), _ptr(oob))
    return x_emb, x_norm, stats


def emb_masknet_ln_bwd(x_emb, stats, values, gamma, dx_norm, dx_emb=None):
    """x_emb / stats as the forward wrote them, dx_norm [B, F E], dx_emb = dLoss/dx_emb from its other consumers (None:
    zeros) -> (vals [B*F, E] IndexedSlices values in the order of X, dgamma [F, E], dbeta [F, E])."""
    if _f32(stats, "stats").dim() != 3 or stats.shape[2] != 2:
        raise ValueError("stats must be [B, fields, 2]")
    B, F, E, Fk = _keyed_head(x_emb, values, F=stats.shape[1], name="x_emb")
    masknet_ln_check_shape(F, E, Fk)
    _expect(stats, (B, F, 2), "stats", "[B, fields, 2]")
    _expect(gamma, (F, E), "gamma", "[fields, embedding_dims]")
    _expect(dx_norm, (B, F * E), "dx_norm", "[B, F E]")
    _expect(dx_emb, (B, F * E), "dx_emb", "[B, F E]", optional=True)
    dev = x_emb.device
    vals = _new((B * F, E), dev)
    dgamma = torch.zeros((F, E), dtype=torch.float32, device=dev)
    dbeta = torch.zeros((F, E), dtype=torch.float32, device=dev)
    if B > 0:
        _call_ws("rec_masknet_ln_workspace_bytes", (B, F, E), "rec_emb_masknet_ln_bwd_f32", dev, _ptr(x_emb), _ptr(stats),
                 _ptr(values), _ptr(gamma), _ptr(dx_norm), _ptr(dx_emb), B, F, Fk, E, _ptr(vals), _ptr(dgamma),
                 _ptr(dbeta))
    return vals, dgamma, dbeta


def _mask_block_args(x_emb, v, W1, W2, W3):
    """-> (B, D, P, O, R) of a block's operands, checked against each other and the limits."""
    for t, n in ((x_emb, "x_emb"), (v, "v"), (W1, "W1"), (W2, "W2"), (W3, "W3")):
        if _f32(t, n).dim() != 2:
            raise ValueError("%s must be 2-D, got %s" % (n, tuple(t.shape)))
    B, D = x_emb.shape
    P, O = W3.shape
    H = W1.shape[1]
    if v.shape != (B, P) or W1.shape[0] != D or tuple(W2.shape) != (H, P) or P < 1 or H % P:
        raise ValueError("a mask block takes x_emb [B,D], v [B,P], W1 [D,R P], W2 [R P,P], W3 [P,O]; got %s %s %s %s %s"
                         % tuple(tuple(t.shape) for t in (x_emb, v, W1, W2, W3)))
    R = H // P
    mask_block_check_shape(D, P, O, R)
    return B, D, P, O, R


def mask_block_fwd(x_emb, v, W1, b1, W2, b2, W3, b3, gamma, beta, save=True):
    """One mask block in one launch: y = relu(LayerNorm((v * (relu(x_emb W1 + b1) W2 + b2)) W3 + b3)) -> (y [B,O],
    saved) with saved = (h [B,R P], m [B,P], xhat [B,O], rstd [B]) for the backward, or None (``save=False``: inference,
    only y is written)."""
    B, D, P, O, R = _mask_block_args(x_emb, v, W1, W2, W3)
    for t, n, name in ((b1, R * P, "b1"), (b2, P, "b2"), (b3, O, "b3"), (gamma, O, "gamma"), (beta, O, "beta")):
        _vec(t, n, name)
    dev = x_emb.device
    y = _new((B, O), dev)
    saved = (_new((B, R * P), dev), _new((B, P), dev), _new((B, O), dev), _new((B,), dev)) if save else None
    _call("rec_mask_block_fwd_f32", _ptr(x_emb), _ptr(v), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(W3), _ptr(b3),
          _ptr(gamma), _ptr(beta), B, D, P, O, R, _ptr(y), *_ptrs(saved or (None,) * 4))
    return y, saved


def mask_block_bwd(x_emb, v, W1, W2, W3, gamma, y, saved, dy, dx_emb=None, accumulate=False):
    """-> (dv [B,P], dx_emb [B,D], (dW1, db1, dW2, db2, dW3, db3, dgamma, dbeta)).  ``accumulate``: the block's
    dLoss/dx_emb is added to the given ``dx_emb`` in place (the blocks of a stack share one buffer)."""
    B, D, P, O, R = _mask_block_args(x_emb, v, W1, W2, W3)
    h, m, xhat, rstd = saved
    _vec(gamma, O, "gamma")
    _expect_all([(y, (B, O), "y"), (dy, (B, O), "dy"), (h, (B, R * P), "h"), (m, (B, P), "m"), (xhat, (B, O), "xhat"),
                 (rstd, (B,), "rstd")])
    dev = x_emb.device
    if dx_emb is None:
        if accumulate:
            raise ValueError("accumulate needs the dx_emb to add to")
        dx_emb = _new((B, D), dev, B)
    else:
        _expect(dx_emb, (B, D), "dx_emb", "[B,D]")
    dv = _new((B, P), dev)
    grads = tuple(torch.zeros(shp, dtype=torch.float32, device=dev)
                  for shp in ((D, R * P), (R * P,), (R * P, P), (P,), (P, O), (O,), (O,), (O,)))
    if B > 0:
        _call_ws("rec_masknet_block_workspace_bytes", (B, D, P, O, R), "rec_mask_block_bwd_f32", dev, _ptr(x_emb),
                 _ptr(v), _ptr(W1), _ptr(W2), _ptr(W3), _ptr(gamma), _ptr(y), _ptr(h), _ptr(m), _ptr(xhat), _ptr(rstd),
                 _ptr(dy), B, D, P, O, R, _ptr(dv), _ptr(dx_emb), int(bool(accumulate)), *_ptrs(grads))
    return dv, dx_emb, grads


# ---- ContextNet: lookup x value, and the block (csrc/contextnet.hip).  The limits are MaskNet's.
def contextnet_check_shape(F, E, R=3, Fk=0):
    """ValueError for sizes that describe no ContextNet block, NotImplementedError for shapes the kernels do not cover
    (the ABI would return -2): fields F, embedding_dims E, reduction rate R of the contextual-embedding MLP."""
    if F < 1 or E < 1 or R < 1 or not 0 <= Fk <= F:
        raise ValueError("fields, embedding_dims and the reduction rate must be positive and 0 <= continuous fields <= "
                         "fields, got fields=%d, embedding_dims=%d, reduction_rate=%d, continuous=%d" % (F, E, R, Fk))
    if F > MASKNET_MAX_F or E > MASKNET_MAX_E or F * E > MASKNET_MAX_D or R > MASKNET_MAX_R:
        raise NotImplementedError(
            "ContextNet kernels cover fields <= %d, embedding_dims <= %d, fields * embedding_dims <= %d and "
            "reduction_rate <= %d; got fields=%d, embedding_dims=%d, fields * embedding_dims=%d, reduction_rate=%d"
            % (MASKNET_MAX_F, MASKNET_MAX_E, MASKNET_MAX_D, MASKNET_MAX_R, F, E, F * E, R))


def emb_contextnet_in_fwd(table, X, values, oob=None):
    """Lookup with the rows of the last ``values.shape[1]`` columns of X (the keys of continuous features) scaled by
    ``values``, one launch -> x [B, F E]."""
    V, E = _table(table, "table").shape
    B, F, E, Fk = _keyed_head(X, values, E)
    contextnet_check_shape(F, E, 1, Fk)
    x = _new((B, F * E), table.device)
    _call("rec_emb_contextnet_in_fwd_f32", _ptr(table), V, E, table.stride(0), _ptr(X), _ptr(values), B, F, Fk, _ptr(x),
          _ptr(oob))
    return x


def emb_contextnet_in_bwd(dx, values, F):
    """dx [B, F E] = dLoss/dx -> vals [B*F, E], the IndexedSlices values in the order of X, the key fields' multiplied by
    their value."""
    B, F, E, Fk = _keyed_head(dx, values, F=F)
    contextnet_check_shape(F, E, 1, Fk)
    vals = _new((B * F, E), dx.device)
    _call("rec_emb_contextnet_in_bwd_f32", _ptr(values), _ptr(dx), B, F, Fk, E, _ptr(vals))
    return vals


def _contextnet_block_args(x, Wa, Wb, W1, W2, gamma):
    """-> (B, F, E, R, pointwise) of a block's operands, checked against each other and the limits.  W2 None: single
    mode."""
    for t, n, d in ((x, "x", 2), (Wa, "Wa", 2), (Wb, "Wb", 2), (W1, "W1", 3), (W2, "W2", 3), (gamma, "gamma", 2)):
        if t is not None and _f32(t, n).dim() != d:
            raise ValueError("%s must be %d-D, got %s" % (n, d, tuple(t.shape)))
    B, D = x.shape
    F, E = W1.shape[0], W1.shape[2]
    H = Wa.shape[1]
    if (F * E != D or W1.shape[1] != E or Wa.shape[0] != D or tuple(Wb.shape) != (H, D) or D < 1 or H % D
            or (W2 is not None and W2.shape != W1.shape) or tuple(gamma.shape) != (F, E)):
        raise ValueError("a ContextNet block takes x [B,F E], Wa [F E,R F E], Wb [R F E,F E], W1 (and W2) [F,E,E], gamma "
                         "[F,E]; got %s" % ", ".join(str(None if t is None else tuple(t.shape))
                                                      for t in (x, Wa, Wb, W1, W2, gamma)))
    R = H // D
    contextnet_check_shape(F, E, R)
    return B, F, E, R, int(W2 is not None)


def contextnet_block_fwd(x, Wa, ba, Wb, bb, W1, W2, gamma, beta, save=True):
    """One ContextNet block in one launch: u = x * (relu(x Wa + ba) Wb + bb), per field r_f = relu(u_f W1_f) W2_f + u_f
    (``W2`` None: r_f = u_f W1_f), y_f = LayerNorm_f(r_f) -> (y [B, F E], saved) with saved = (h [B,R F E], m [B,F E],
    xhat [B,F E], rstd [B,F], a [B,F E] or None) for the backward, or None (``save=False``: inference, only y is
    written)."""
    B, F, E, R, pw = _contextnet_block_args(x, Wa, Wb, W1, W2, gamma)
    D = F * E
    for t, n, name in ((ba, R * D, "ba"), (bb, D, "bb"), (beta, D, "beta")):
        _vec(t, n, name)
    dev = x.device
    y = _new((B, D), dev)
    saved = (_new((B, R * D), dev), _new((B, D), dev), _new((B, D), dev), _new((B, F), dev),
             _new((B, D), dev) if pw else None) if save else None
    _call("rec_contextnet_block_fwd_f32", _ptr(x), _ptr(Wa), _ptr(ba), _ptr(Wb), _ptr(bb), _ptr(W1), _ptr(W2),
          _ptr(gamma), _ptr(beta), B, F, E, R, pw, _ptr(y), *_ptrs(saved or (None,) * 5))
    return y, saved


def contextnet_block_bwd(x, Wa, Wb, W1, W2, gamma, saved, dy):
    """-> (dx [B, F E], (dWa, dba, dWb, dbb, dW1, dW2 or None, dgamma, dbeta))."""
    B, F, E, R, pw = _contextnet_block_args(x, Wa, Wb, W1, W2, gamma)
    D = F * E
    h, m, xhat, rstd, a = saved
    _expect_all([(dy, (B, D), "dy"), (h, (B, R * D), "h"), (m, (B, D), "m"), (xhat, (B, D), "xhat"),
                 (rstd, (B, F), "rstd")] + ([(a, (B, D), "a")] if pw else []))
    dev = x.device
    dx = _new((B, D), dev, B)
    shapes = ((D, R * D), (R * D,), (R * D, D), (D,), (F, E, E), (F, E, E) if pw else None, (F, E), (F, E))
    grads = tuple(None if s is None else torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes)
    if B > 0:
        _call_ws("rec_contextnet_block_workspace_bytes", (B, F, E, R, pw), "rec_contextnet_block_bwd_f32", dev, _ptr(x),
                 _ptr(Wa), _ptr(Wb), _ptr(W1), _ptr(W2), _ptr(gamma), _ptr(h), _ptr(m), _ptr(xhat), _ptr(rstd), _ptr(a),
                 _ptr(dy), B, F, E, R, pw, _ptr(dx), *_ptrs(grads))
    return dx, grads


# ---- FiBiNet++: lookup x value + BatchNorm / per-field LayerNorm, and the SENet+ / bilinear+ block (csrc/fibinetplus.hip).
# The limits are FiBiNet's and MaskNet's.
def fibinetplus_check_shape(F, E, G=1, mid=1, O=1, Fk=0, min_fields=2):
    """ValueError for sizes that describe no FiBiNet++ layer, NotImplementedError for shapes the kernels do not cover
    (the ABI would return -2): fields F, embedding_dims E, SENet+ groups G and hidden units mid, bilinear+ output
    width O, continuous fields Fk.  The body needs a pair of fields (``min_fields`` 2), the input stage one."""
    if min(F, E, G, mid, O) < 1 or not 0 <= Fk <= F or E % G:
        raise ValueError("fields, embedding_dims, groups, SENet units and the bilinear output width must be positive, the "
                         "groups divide embedding_dims and 0 <= continuous fields <= fields; got fields=%d, "
                         "embedding_dims=%d, groups=%d, SENet units=%d, output width=%d, continuous=%d"
                         % (F, E, G, mid, O, Fk))
    if not (min_fields <= F <= FIBINET_MAX_F and E <= FIBINET_MAX_E and F * E <= MASKNET_MAX_D and O <= MASKNET_MAX_O
            and mid <= MASKNET_MAX_P):
        raise NotImplementedError(
            "FiBiNet++ kernels cover %d <= fields <= %d, embedding_dims <= %d, fields * embedding_dims <= %d, bilinear "
            "output width <= %d and SENet units <= %d; got fields=%d, embedding_dims=%d, fields * embedding_dims=%d, "
            "output width=%d, SENet units=%d"
            % (min_fields, FIBINET_MAX_F, FIBINET_MAX_E, MASKNET_MAX_D, MASKNET_MAX_O, MASKNET_MAX_P, F, E, F * E, O, mid))


def fibinetplus_mid(F, G, reduction_ratio):
    """SENetPlusLayer's hidden width (11.FiBiNet++/CustomLayers.py:191)."""
    return max(1, 2 * G * F // reduction_ratio)


def _fibinetplus_in_gammas(F, E, Fk, gamma_bn, gamma_ln):
    """what both directions of the input stage check after the keyed head: the limits and the two scales"""
    fibinetplus_check_shape(F, E, Fk=Fk, min_fields=1)
    if Fk < F:
        _vec(gamma_bn, E, "gamma_bn")
    if Fk > 0:
        _expect(gamma_ln, (Fk, E), "gamma_ln", "[Fk,E]")


def emb_fibinetplus_in_fwd(table, X, values, gamma_bn, beta_bn, gamma_ln, beta_ln, moving_mean, moving_var, training,
                           oob=None, save=True):
    """Lookup, x value on the last ``values.shape[1]`` columns of X, ONE BatchNorm over the categorical rows (training:
    batch statistics and the moving averages updated on the device; else the moving statistics) and a LayerNorm per key
    field -> (x [B, F E], saved) with saved = (xhat [B, F E], rstd_bn [E], rstd_ln [B, Fk]) or None (``save=False``)."""
    V, E = _table(table, "table").shape
    B, F, E, Fk = _keyed_head(X, values, E)
    _fibinetplus_in_gammas(F, E, Fk, gamma_bn, gamma_ln)
    if Fk < F:
        for t, name in ((beta_bn, "beta_bn"), (moving_mean, "moving_mean"), (moving_var, "moving_var")):
            _vec(t, E, name)
    if Fk > 0:
        _vec(beta_ln, Fk * E, "beta_ln")
    dev = table.device
    x = _new((B, F * E), dev)
    saved = (_new((B, F * E), dev), _new((E,), dev), _new((B, max(Fk, 1)), dev)) if save else None
    if B > 0:
        _call_ws("rec_emb_fibinetplus_in_workspace_bytes", (B, F, Fk, E), "rec_emb_fibinetplus_in_fwd_f32", dev,
                 _ptr(table), V, E, table.stride(0), _ptr(X), _ptr(values), _ptr(gamma_bn), _ptr(beta_bn), _ptr(gamma_ln),
                 _ptr(beta_ln), B, F, Fk, int(bool(training)), _ptr(moving_mean), _ptr(moving_var), _ptr(x),
                 *_ptrs(saved or (None,) * 3), _ptr(oob))
    return x, saved


def emb_fibinetplus_in_bwd(dx, values, saved, gamma_bn, gamma_ln, F, training):
    """dx [B, F E] = dLoss/dx -> (vals [B*F, E], the IndexedSlices values in the order of X with the key fields'
    multiplied by their value, dgamma_bn [E], dbeta_bn [E], dgamma_ln [Fk, E], dbeta_ln [Fk, E])."""
    B, F, E, Fk = _keyed_head(dx, values, F=F)
    _fibinetplus_in_gammas(F, E, Fk, gamma_bn, gamma_ln)
    xhat, rstd_bn, rstd_ln = saved
    _expect(xhat, (B, F * E), "xhat", "[B, F E]")
    _vec(rstd_bn, E, "rstd_bn"); _vec(rstd_ln, B * max(Fk, 1), "rstd_ln")
    dev = dx.device
    # the gradients of a kind of field the batch does not have are left alone by the call: zeros, as for an empty batch
    Bc, Bk = (B if Fk < F else 0), (B if Fk > 0 else 0)
    vals = _new((B * F, E), dev, B)
    dg_bn, db_bn, dg_ln, db_ln = _new((E,), dev, Bc), _new((E,), dev, Bc), _new((Fk, E), dev, Bk), _new((Fk, E), dev, Bk)
    if B > 0:
        _call_ws("rec_emb_fibinetplus_in_workspace_bytes", (B, F, Fk, E), "rec_emb_fibinetplus_in_bwd_f32", dev,
                 _ptr(dx), _ptr(values), _ptr(xhat), _ptr(rstd_bn), _ptr(rstd_ln), _ptr(gamma_bn), _ptr(gamma_ln), B, F,
                 Fk, E, int(bool(training)), _ptr(vals), _ptr(dg_bn), _ptr(db_bn), _ptr(dg_ln), _ptr(db_ln))
    return vals, dg_bn, db_bn, dg_ln, db_ln


def _fibinetplus_block_args(x, W, Wr, S0, S1, G, type_code):
    """-> (B, F, E, G, mid, O, type) of a block's operands, checked against each other and the limits."""
    for t, n, d in ((x, "x", 2), (W, "W", 3), (Wr, "Wr", 2), (S0, "S0", 2), (S1, "S1", 2)):
        if _f32(t, n).dim() != d:
            raise ValueError("%s must be %d-D, got %s" % (n, d, tuple(t.shape)))
    B, D = x.shape
    nW, E = W.shape[0], W.shape[2]
    P, O = Wr.shape
    mid = S0.shape[1]
    F = D // E if E > 0 and D % E == 0 else -1
    G = int(G)
    if type_code not in FIBINET_TYPES.values():
        raise ValueError("type_code must be one of %s, got %r" % (sorted(FIBINET_TYPES.values()), type_code))
    name = [k for k, v in FIBINET_TYPES.items() if v == type_code][0]
    if (F < 2 or W.shape[1] != E or P != F * (F - 1) // 2 or nW != fibinet_num_weights(F, name) or G < 1 or E % G
            or S0.shape[0] != 2 * G * F or tuple(S1.shape) != (mid, D) or min(mid, O) < 1):
        raise ValueError("a FiBiNet++ block takes x [B,F E], W [nW,E,E], Wr [F(F-1)/2,O], S0 [2 G F,mid], S1 [mid,F E] "
                         "with G dividing E; got %s, G=%d" % (", ".join(str(tuple(t.shape)) for t in (x, W, Wr, S0, S1)),
                                                              G))
    fibinetplus_check_shape(F, E, G, mid, O)
    return B, F, E, G, mid, O, int(type_code)


def fibinetplus_block_fwd(x, W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1, G, type_code, save=True):
    """The FiBiNet++ body in one launch: q = LN(p Wr + br) with p the pair scalars x_i W x_j^T, v = x * relu(LN(relu(LN(
    s S0 + b0)) S1 + b1)) with s the group means and maxima -> (out [B, O + F E] = [q | v], saved) with saved = (p,
    xhat_q, s, xhat0, h, xhat1, rstd [B,3]) for the backward, or None (``save=False``: inference, only out is
    written)."""
    B, F, E, G, mid, O, tc = _fibinetplus_block_args(x, W, Wr, S0, S1, G, type_code)
    D, P = F * E, F * (F - 1) // 2
    for t, n, name in ((br, O, "br"), (gq, O, "gamma_q"), (bq, O, "beta_q"), (b0, mid, "b0"), (g0, mid, "gamma0"),
                       (be0, mid, "beta0"), (b1, D, "b1"), (g1, D, "gamma1"), (be1, D, "beta1")):
        _vec(t, n, name)
    dev = x.device
    out = _new((B, O + D), dev)
    saved = tuple(_new((B, w), dev) for w in (P, O, 2 * G * F, mid, mid, D, 3)) if save else None
    _call("rec_fibinetplus_block_fwd_f32", *_ptrs((x, W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1)), B, F, E, G,
          mid, O, tc, _ptr(out), *_ptrs(saved or (None,) * 7))
    return out, saved


def fibinetplus_block_bwd(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, G, type_code, saved, dout):
    """-> (dx [B, F E], (dW, dWr, dbr, dgamma_q, dbeta_q, dS0, db0, dgamma0, dbeta0, dS1, db1, dgamma1, dbeta1))."""
    B, F, E, G, mid, O, tc = _fibinetplus_block_args(x, W, Wr, S0, S1, G, type_code)
    D, P = F * E, F * (F - 1) // 2
    shapes = ((B, P), (B, O), (B, 2 * G * F), (B, mid), (B, mid), (B, D), (B, 3))
    names = ("p", "xhat_q", "s", "xhat0", "h", "xhat1", "rstd")
    _expect_all(list(zip(saved, shapes, names)) + [(dout, (B, O + D), "dout")])
    dev = x.device
    dx = _new((B, D), dev, B)
    grads = tuple(_new(s, dev, B) for s in (tuple(W.shape), (P, O), (O,), (O,), (O,), (2 * G * F, mid), (mid,), (mid,),
                                            (mid,), (mid, D), (D,), (D,), (D,)))
    if B > 0:
        _call_ws("rec_fibinetplus_block_workspace_bytes", (B, F, E, G, mid, O, tc), "rec_fibinetplus_block_bwd_f32", dev,
                 *_ptrs((x, W, Wr, gq, S0, g0, be0, S1, g1, be1)), *_ptrs(saved), _ptr(dout), B, F, E, G, mid, O, tc,
                 _ptr(dx), *_ptrs(grads))
    return dx, grads


# ---- MMOE / ESMM: experts, gates, gate mixture and towers in one launch each way (csrc/mmoe.hip).  The limits are
# MaskNet's.
def mmoe_check_shape(D, n, T=2, H1=64, O=8, H2=64, O2=8):
    """ValueError for sizes that describe no MMOE body, NotImplementedError for shapes the kernel does not cover (the ABI
    would return -2): input width D, n experts, T tasks, hidden width H1 of experts and gates, expert output width O,
    tower widths H2 and O2."""
    if min(D, n, T, H1, O, H2, O2) < 1:
        raise ValueError("every size of an MMOE body must be positive, got D=%d, experts=%d, tasks=%d, H1=%d, O=%d, "
                         "H2=%d, O2=%d" % (D, n, T, H1, O, H2, O2))
    N1 = (n + T) * H1
    if (D > MASKNET_MAX_D or N1 > MASKNET_MAX_P or T > MASKNET_MAX_R
            or max(H1, H2, O2, n * O, n * T) > MASKNET_MAX_O):
        raise NotImplementedError(
            "MMOE kernels cover fields * embedding_dims <= %d, (experts + tasks) * H1 <= %d, tasks <= %d and each of H1, "
            "H2, O2, experts * O and experts * tasks <= %d; got fields * embedding_dims=%d, (experts + tasks) * H1=%d, "
            "tasks=%d, H1=%d, H2=%d, O2=%d, experts * O=%d, experts * tasks=%d"
            % (MASKNET_MAX_D, MASKNET_MAX_P, MASKNET_MAX_R, MASKNET_MAX_O, D, N1, T, H1, H2, O2, n * O, n * T))


_MMOE_WEIGHTS = ("W1", "b1", "We2", "be2", "Wg2", "bg2", "Wt1", "bt1", "Wt2", "bt2", "Wt3", "bt3")


def _mmoe_args(x, w, passes, ctcvr):
    """-> (B, D, n, T, H1, O, H2, O2) of the packed weights ``w`` (a dict or sequence in the order of _MMOE_WEIGHTS),
    checked against each other, the flags and the limits."""
    W1, b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 = w
    for t, name, dim in ((x, "x", 2), (W1, "W1", 2), (We2, "We2", 3), (Wg2, "Wg2", 3), (Wt1, "Wt1", 3), (Wt2, "Wt2", 3),
                         (Wt3, "Wt3", 2)):
        if _f32(t, name).dim() != dim:
            raise ValueError("%s must be %d-D, got %s" % (name, dim, tuple(t.shape)))
    B, D = x.shape
    n, H1, O = We2.shape
    T, H2, O2 = Wt2.shape
    if (tuple(W1.shape) != (D, (n + T) * H1) or tuple(Wg2.shape) != (T, H1, n) or tuple(Wt1.shape) != (T, n * O, H2)
            or tuple(Wt3.shape) != (T, O2)):
        raise ValueError("an MMOE body takes x [B,D], W1 [D,(n+T) H1], We2 [n,H1,O], Wg2 [T,H1,n], Wt1 [T,n O,H2], Wt2 "
                         "[T,H2,O2], Wt3 [T,O2]; got %s" % ", ".join(str(tuple(t.shape))
                                                                      for t in (x, W1, We2, Wg2, Wt1, Wt2, Wt3)))
    if passes not in (1, 2) or ctcvr not in (0, 1, False, True) or (ctcvr and T != 2):
        raise ValueError("gate_softmax_passes is 1 or 2 and ctcvr needs two tasks, got passes=%r, ctcvr=%r, tasks=%d"
                         % (passes, ctcvr, T))
    mmoe_check_shape(D, n, T, H1, O, H2, O2)
    for t, cnt, name in ((b1, (n + T) * H1, "b1"), (be2, n * O, "be2"), (bg2, T * n, "bg2"), (bt1, T * H2, "bt1"),
                         (bt2, T * O2, "bt2"), (bt3, T, "bt3")):
        _vec(t, cnt, name)
    return B, D, n, T, H1, O, H2, O2


def mmoe_fwd(x, weights, gate_softmax_passes=1, ctcvr=False, save=True):
    """The MMOE / ESMM body in one launch: experts and gates over x [B, D], softmax gates (``gate_softmax_passes`` 1 or
    2), the gate-weighted expert outputs flattened into the towers -> (out [B, T], saved) with out[:, t] the task
    probability (``ctcvr``: out[:, 1] = p_0 p_1) and saved = (h [B,(n+T) H1], e [B,n O], z [B,T n], g [B,T n], a1
    [B,T H2], a2 [B,T O2], p [B,T]) for the backward, or None (``save=False``: inference, only out is written).
    ``weights``: W1, b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 as include/mi355rec.h packs them."""
    B, D, n, T, H1, O, H2, O2 = _mmoe_args(x, weights, gate_softmax_passes, ctcvr)
    dev = x.device
    out = _new((B, T), dev)
    saved = tuple(_new((B, w), dev) for w in ((n + T) * H1, n * O, T * n, T * n, T * H2, T * O2, T)) if save else None
    _call("rec_mmoe_fwd_f32", _ptr(x), *_ptrs(weights), B, D, n, T, H1, O, H2, O2, int(gate_softmax_passes),
          int(bool(ctcvr)), _ptr(out), *_ptrs(saved or (None,) * 7))
    return out, saved


def mmoe_bwd(x, weights, saved, dout, gate_softmax_passes=1, ctcvr=False):
    """-> (dx [B, D], grads) with grads the gradient of every packed weight, in the order of ``weights``."""
    B, D, n, T, H1, O, H2, O2 = _mmoe_args(x, weights, gate_softmax_passes, ctcvr)
    shapes = ((B, (n + T) * H1), (B, n * O), (B, T * n), (B, T * n), (B, T * H2), (B, T * O2), (B, T))
    _expect_all(zip(tuple(saved) + (dout,), shapes + ((B, T),), ("h", "e", "z", "g", "a1", "a2", "p", "dout")))
    dev = x.device
    dx = _new((B, D), dev, B)
    grads = [_new_like(t, B) for t in weights]
    if B > 0:
        W1, _, We2, _, Wg2, _, Wt1, _, Wt2, _, Wt3, _ = weights
        _call_ws("rec_mmoe_workspace_bytes", (B, D, n, T, H1, O, H2, O2), "rec_mmoe_bwd_f32", dev, _ptr(x),
                 *_ptrs((W1, We2, Wg2, Wt1, Wt2, Wt3)), *_ptrs(saved), _ptr(dout), B, D, n, T, H1, O, H2, O2,
                 int(gate_softmax_passes), int(bool(ctcvr)), _ptr(dx), *_ptrs(grads))
    return dx, grads


# ---- PLE: one CGC level (experts, task gates, the shared gate, the gated sums, the towers of the last level) in one
# launch each way (csrc/ple.hip).  The limits are MaskNet's.
def ple_check_shape(Din, Gin, T, S, Sh, H1=64, O=8, Og=8, last=False):
    """ValueError for sizes that describe no CGC level, NotImplementedError for shapes the kernels do not cover (the ABI
    would return -2): input width Din of each of Gin in {1, T + 1} input groups, T tasks, S specific experts per task, Sh
    shared experts, hidden width H1, expert output width O, gate MLP output width Og."""
    if min(Din, Gin, T, S, Sh, H1, O, Og) < 1:
        raise ValueError("every size of a PLE level must be positive, got Din=%d, Gin=%d, tasks=%d, specific=%d, "
                         "shared=%d, H1=%d, O=%d, Og=%d" % (Din, Gin, T, S, Sh, H1, O, Og))
    if Gin not in (1, T + 1):
        raise ValueError("a PLE level reads one input group or tasks + 1 = %d of them, got %d" % (T + 1, Gin))
    ne = T * S + Sh
    GW = T * (S + Sh) + (0 if last else ne)
    if (Din > MASKNET_MAX_D or T > MASKNET_MAX_R or max(H1, ne * O, (T + 1) * Og, GW) > MASKNET_MAX_O
            or (Gin > 1 and Gin * Din > MASKNET_MAX_O)):
        raise NotImplementedError(
            "PLE kernels cover Din <= %d, tasks <= %d, each of H1, experts * O, (tasks + 1) * Og and the gate columns "
            "tasks * (specific + shared) [+ experts] <= %d, and Gin * Din <= %d for a grouped level; got Din=%d, Gin=%d, "
            "tasks=%d, H1=%d, experts * O=%d, (tasks + 1) * Og=%d, gate columns=%d"
            % (MASKNET_MAX_D, MASKNET_MAX_R, MASKNET_MAX_O, MASKNET_MAX_O, Din, Gin, T, H1, ne * O, (T + 1) * Og, GW))


def _ple_args(xin, w, T, S, Sh, last):
    """-> (B, Din, Gin, H1, O, Og) of xin [B, Gin, Din] and the packed weights ``w`` = (W1, b1, We2, be2, Wg2, bg2, Wg3s,
    Wg3h, Wtw, btw) (Wg3h None iff last; Wtw, btw None unless last), checked against each other and the limits."""
    if len(w) != 10:
        raise ValueError("a PLE level takes ten packed weights (None for the absent ones), got %d" % len(w))
    W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h, Wtw, btw = w
    last = bool(last)
    if last and (Wg3h is not None or Wtw is None or btw is None):
        raise ValueError("the last level has towers (Wtw, btw) and no shared gate (Wg3h)")
    if not last and (Wg3h is None or Wtw is not None or btw is not None):
        raise ValueError("a level before the last has a shared gate (Wg3h) and no towers (Wtw, btw)")
    for t, name, dim in ((xin, "xin", 3), (W1, "W1", 2), (We2, "We2", 3), (Wg2, "Wg2", 3), (Wg3s, "Wg3s", 3)):
        if _f32(t, name).dim() != dim:
            raise ValueError("%s must be %d-D, got %s" % (name, dim, tuple(t.shape)))
    T, S, Sh = int(T), int(S), int(Sh)
    B, Gin, Din = xin.shape
    _, H1, O = We2.shape
    Og = Wg2.shape[2]
    ple_check_shape(Din, Gin, T, S, Sh, H1, O, Og, last)
    ne, ns, Gout = T * S + Sh, S + Sh, T if last else T + 1
    want = [(Din, (ne + Gout) * H1), (ne, H1, O), (Gout, H1, Og), (T, Og, ns)]
    got = [tuple(t.shape) for t in (W1, We2, Wg2, Wg3s)]
    if last:
        want.append((T, O))
        got.append(tuple(_f32(Wtw, "Wtw").shape))
    else:
        want.append((Og, ne))
        got.append(tuple(_f32(Wg3h, "Wg3h").shape))
    if want != got:
        raise ValueError("a PLE level takes W1 [Din,(ne+Gout) H1], We2 [ne,H1,O], Wg2 [Gout,H1,Og], Wg3s [T,Og,S+Sh] and "
                         "Wg3h [Og,ne] or Wtw [T,O]: expected %s, got %s" % (want, got))
    for t, cnt, name in ((b1, (ne + Gout) * H1, "b1"), (be2, ne * O, "be2"), (bg2, Gout * Og, "bg2")) + \
            (((btw, T, "btw"),) if last else ()):
        _vec(t, cnt, name)
    return B, Din, Gin, H1, O, Og


def ple_cgc_fwd(xin, weights, T, S, Sh, last=False, save=True):
    """One CGC level in one launch: xin [B, Gin, Din] (Gin = 1: one input for every MLP; Gin = T + 1: each task and the
    shared branch reads its own) -> (y [B, Gout, O], out [B, T] or None, saved) with Gout = T (``last``) or T + 1, out
    the tower probabilities of the last level, and saved = (h [B, N1], e [B, ne O], q [B, Gout Og], g [B, GW]) for the
    backward, or None (``save=False``: inference, the same y and out).  ``weights``: W1, b1, We2, be2, Wg2, bg2, Wg3s,
    Wg3h, Wtw, btw as include/mi355rec.h packs them, None for Wg3h of the last level and for Wtw, btw of the others."""
    B, Din, Gin, H1, O, Og = _ple_args(xin, weights, T, S, Sh, last)
    last = int(bool(last))
    ne, Gout = T * S + Sh, T if last else T + 1
    GW = T * (S + Sh) + (0 if last else ne)
    dev = xin.device
    y = _new((B, Gout, O), dev)
    out = _new((B, T), dev) if last else None
    saved = tuple(_new((B, w), dev) for w in ((ne + Gout) * H1, ne * O, Gout * Og, GW)) if save else None
    _call("rec_ple_cgc_fwd_f32", _ptr(xin), *_ptrs(weights), B, Din, Gin, T, S, Sh, H1, O, Og, last, _ptr(y), _ptr(out),
          *_ptrs(saved or (None,) * 4))
    return y, out, saved


def ple_cgc_bwd(xin, weights, saved, y, out, dy, dout, T, S, Sh, last=False):
    """-> (dxin [B, Gin, Din], grads) with grads the gradient of every packed weight in the order of ``weights`` (None
    where the weight is None).  ``dy`` [B, Gout, O] may be None for the last level; ``dout`` [B, T] and ``out`` belong to
    the last level alone."""
    B, Din, Gin, H1, O, Og = _ple_args(xin, weights, T, S, Sh, last)
    last = int(bool(last))
    ne, Gout = T * S + Sh, T if last else T + 1
    GW = T * (S + Sh) + (0 if last else ne)
    if saved is None or len(saved) != 4:
        raise ValueError("the backward of a PLE level needs the four save buffers h, e, q, g")
    named = list(zip(tuple(saved) + (y,), ((B, (ne + Gout) * H1), (B, ne * O), (B, Gout * Og), (B, GW), (B, Gout, O)),
                     ("h", "e", "q", "g", "y")))
    if last:
        named += [(out, (B, T), "out"), (dout, (B, T), "dout")]
    elif out is not None or dout is not None:
        raise ValueError("out and dout belong to the last level")
    if dy is not None or not last:
        named.append((dy, (B, Gout, O), "dy"))
    _expect_all(named)
    dev = xin.device
    dxin = _new((B, Gin, Din), dev, B)
    grads = [None if t is None else _new_like(t, B) for t in weights]
    if B > 0:
        W1, _, We2, _, Wg2, _, Wg3s, Wg3h, Wtw, _ = weights
        _call_ws("rec_ple_cgc_workspace_bytes", (B, Din, Gin, T, S, Sh, H1, O, Og, last), "rec_ple_cgc_bwd_f32", dev,
                 _ptr(xin), *_ptrs((W1, We2, Wg2, Wg3s, Wg3h, Wtw)), *_ptrs(saved), _ptr(y), _ptr(out), _ptr(dy),
                 _ptr(dout), B, Din, Gin, T, S, Sh, H1, O, Og, last, _ptr(dxin), *_ptrs(grads))
    return dxin, grads


# ---- MIND: capsule routing and label-aware attention + sampled-softmax loss, one launch each way (csrc/mind.hip).  The
# limits are DIN's key width and AFM's attention size, the rounds and the LDS fit are the header's.
MIND_MAX_ROUNDS = LIMITS["REC_CAPSULE_MAX_R"]
_TILE_LDS_CAP = LIMITS["REC_TILE_LDS_CAP"]    # the launch cap of every one-example / one-tile kernel _lds_fit guards


def _odd(n):
    return n | 1


# what the MIND, ComiRec and CAN wrappers share
def _caps_limits(family, D, Dc, K, R, rounds):
    """NotImplementedError past the limits of the capsule kernels; ``rounds`` is the format R is shown with"""
    if D > DIN_MAX_D or Dc > DIN_MAX_D or K > AFM_MAX_A or (R is not None and R > MIND_MAX_ROUNDS):
        raise NotImplementedError(
            "%s kernels cover key width and capsule width <= %d, capsules <= %d and routing rounds <= %d; got key "
            "width=%d, capsule width=%d, capsules=%d, rounds=%s"
            % (family, DIN_MAX_D, AFM_MAX_A, MIND_MAX_ROUNDS, D, Dc, K, rounds % (R,)))


def _lds_fit(nbytes, holds, formula, at):
    """NotImplementedError where what a kernel holds in LDS (``nbytes`` = 4 (``formula``)) passes the launch cap"""
    if nbytes > _TILE_LDS_CAP:
        raise NotImplementedError("%s in LDS: 4 (%s) <= %d bytes; got %d at %s"
                                  % (holds, formula, _TILE_LDS_CAP, nbytes, at))


def _items_fit(family, Ns, Dc, K):
    _lds_fit(mind_laa_lds_bytes(Ns, Dc, K), "%s attention holds one example" % family,
             "(K + Ns) (Dc|1) + 2 K Ns + 2 Ns", "Ns=%d, capsule width=%d, capsules=%d" % (Ns, Dc, K))


def _caps_head(what, embed, *named):
    """The checks and the arguments every capsule entry point starts with: the table, then ``named``, (tensor, "name
    [a,b,..]", dtype if not fp32) each -- the int64 ids [B, n, C] first -- of that dtype and with as many dimensions as
    its label.  -> the leading ABI arguments (table, stride, V, E, C, ids, B, n) and (V, E, B, n, C)."""
    _table(embed, "embed")
    for t, label, *dtype in named:
        _req(t, dtype[0] if dtype else torch.float32, label.split()[0])
    if any(t.dim() != label.count(",") + 1 for t, label, *_ in named):
        raise ValueError("%s takes %s and %s; got %s" % (what, ", ".join(x[1] for x in named[:-1]), named[-1][1],
                                                         ", ".join(str(tuple(x[0].shape)) for x in named)))
    (V, E), (B, n, Cn) = embed.shape, named[0][0].shape
    return [_ptr(embed), embed.stride(0), V, E, Cn, _ptr(named[0][0]), B, n], (V, E, B, n, Cn)


def _series_head(embed, series, what, *weights):
    return _caps_head(what, embed, (series, "series [B,T,C]", torch.int64), *weights)


def _items_head(embed, items, m, what, *more):
    return _caps_head(what, embed, (items, "items [B,Ns,C]", torch.int64), (m, "m [B,K,Dc]"), *more)


def mind_routing_lds_bytes(T, D, Dc, K, R):
    """LDS of one workgroup of the routing backward (include/mi355rec.h): what both directions are held to."""
    return 4 * (T * _odd(D) + 2 * T * _odd(Dc) + (R + 2) * K * T + 2 * K * _odd(Dc) + T)


def mind_laa_lds_bytes(Ns, Dc, K):
    """LDS of one example of the label-aware attention (include/mi355rec.h)."""
    return 4 * ((K + Ns) * _odd(Dc) + 2 * K * Ns + 2 * Ns)


def mind_check_shape(D, Dc, K, R=3, T=None, Ns=None):
    """ValueError for sizes that describe no MIND body, NotImplementedError naming the limit for shapes the kernels do
    not cover (the ABI would return -2): key width D = E C, capsule width Dc, K capsules, R routing rounds, and -- where
    given -- the series length T (routing) and the number of sampled items Ns (attention: its rows have Dc columns)."""
    sizes = [D, Dc, K, R] + [v for v in (T, Ns) if v is not None]
    if min(sizes) < 1:
        raise ValueError("every size of a MIND body must be positive, got D=%d, Dc=%d, capsules=%d, rounds=%d, T=%r, "
                         "Ns=%r" % (D, Dc, K, R, T, Ns))
    _caps_limits("MIND", D, Dc, K, R, "%d")
    if T is not None:
        _lds_fit(mind_routing_lds_bytes(T, D, Dc, K, R), "MIND routing holds one example",
                 "T (D|1) + 2 T (Dc|1) + (R + 2) K T + 2 K (Dc|1) + T",
                 "T=%d, key width=%d, capsule width=%d, capsules=%d, rounds=%d" % (T, D, Dc, K, R))
    if Ns is not None:
        _items_fit("MIND label-aware", Ns, Dc, K)


def _mind_routing_args(embed, series, S, B0, R, padding_index):
    args, (V, E, B, T, Cn) = _series_head(embed, series, "capsule routing", (S, "S [D,Dc]"), (B0, "B0 [K,T]"))
    D, Dc = S.shape
    K = B0.shape[0]
    if D != Cn * E or B0.shape[1] != T:
        raise ValueError("capsule routing: S must have C E = %d rows and B0 T = %d columns; got S %s, B0 %s"
                         % (Cn * E, T, tuple(S.shape), tuple(B0.shape)))
    mind_check_shape(D, Dc, K, int(R), T=T)
    return args + [_ptr(S), _ptr(B0), Dc, K, int(R), int(padding_index)], (B, T, Cn, E, D, Dc, K)


def mind_routing_fwd(embed, series, S, B0, routing_rounds=3, padding_index=0, oob=None):
    """Capsule routing of MultiInterestExtractorLayer over the looked-up series in one launch: series ids [B,T,C] into
    ``embed``, S [C E, Dc], B0 [K, T] -> the squashed capsules of the last round [B, K, Dc].  Nothing else is saved."""
    args, (B, T, Cn, E, D, Dc, K) = _mind_routing_args(embed, series, S, B0, routing_rounds, padding_index)
    out = _new((B, K, Dc), embed.device)
    if B > 0:                                            # an empty batch answers from the sizes alone
        _call("rec_mind_routing_fwd_f32", *args, _ptr(out), _ptr(oob))
    return out


def mind_routing_bwd(embed, series, S, B0, gout, routing_rounds=3, padding_index=0):
    """-> (gkeys [B,T,C E], the IndexedSlices values of the series lookups, dS [C E, Dc]) from gout [B,K,Dc]; the rounds
    are run again from the ids and differentiated through, all of them.  B0 has no gradient."""
    args, (B, T, Cn, E, D, Dc, K) = _mind_routing_args(embed, series, S, B0, routing_rounds, padding_index)
    _expect(gout, (B, K, Dc), "gout", "[B,K,Dc]")
    dev = embed.device
    gkeys, dS = _new((B, T, D), dev), _new((D, Dc), dev, B)
    if B > 0:
        _call_ws("rec_mind_routing_workspace_bytes", (B, T, E, Cn, Dc, K, int(routing_rounds)),
                 "rec_mind_routing_bwd_f32", dev, *args, _ptr(gout), _ptr(gkeys), _ptr(dS))
    return gkeys, dS


def _mind_laa_args(embed, items, m, kv):
    args, (V, E, B, Ns, Cn) = _items_head(embed, items, m, "label-aware attention", (kv, "kv [B]", torch.int32))
    K, Dc = m.shape[1:]
    if m.shape[0] != B or kv.shape[0] != B or Dc != Cn * E:
        raise ValueError("label-aware attention: m must be [B, K, C E] = [%d, K, %d] and kv [%d]; got m %s, kv %s"
                         % (B, Cn * E, B, tuple(m.shape), tuple(kv.shape)))
    mind_check_shape(Dc, Dc, K, 1, Ns=Ns)
    return args + [_ptr(m), _ptr(kv), K], (B, Ns, Dc, K)


def mind_laa_fwd(embed, items, m, kv, oob=None):
    """LabelAwareAttention over the looked-up sampled items, the inner products and the sampled-softmax loss in one
    launch: item ids [B,Ns,C] into ``embed``, capsules m [B,K,C E], valid capsule counts kv int32 [B] -> (out [B,Ns],
    loss [B]) with the label at sample 0."""
    args, (B, Ns, Dc, K) = _mind_laa_args(embed, items, m, kv)
    out, loss = _new((B, Ns), embed.device), _new((B,), embed.device)
    if B > 0:
        _call("rec_mind_laa_fwd_f32", *args, _ptr(out), _ptr(loss), _ptr(oob))
    return out, loss


def mind_laa_bwd(embed, items, m, kv, gout=None, gloss=None):
    """-> (gm [B,K,C E], gitems [B,Ns,C E], the IndexedSlices values of the item lookups) from gout [B,Ns] and / or
    gloss [B] in one launch; with neither, zeros."""
    args, (B, Ns, Dc, K) = _mind_laa_args(embed, items, m, kv)
    dev = embed.device
    if gout is None and gloss is None:
        return _new((B, K, Dc), dev, B=0), _new((B, Ns, Dc), dev, B=0)
    _expect(gout, (B, Ns), "gout", "[B,Ns]", optional=True)
    _expect(gloss, (B,), "gloss", "[B]", optional=True)
    gm, gitems = _new((B, K, Dc), dev), _new((B, Ns, Dc), dev)
    if B > 0:
        _call("rec_mind_laa_bwd_f32", *args, _ptr(gout), _ptr(gloss), _ptr(gm), _ptr(gitems))
    return gm, gitems


# ---- ComiRec: dynamic routing with unshared weights, the self-attentive extractor and hard attention + sampled-softmax
# loss (csrc/comirec.hip).  The limits are MIND's, the LDS fits are the header's formulas.
def comirec_dr_lds_bytes(T, Dc, R):
    """LDS of one row (b, k) of the dynamic-routing backward (include/mi355rec.h): what both directions are held to."""
    return 4 * (T * _odd(Dc) + (2 * R + 3) * T + 2 * R * _odd(Dc))


def comirec_sa_lds_bytes(T, D, Dc, K):
    """LDS of one workgroup of the self-attentive backward (include/mi355rec.h)."""
    return 4 * (T * _odd(D) + 2 * T * _odd(Dc) + 2 * K * T + 3 * K * _odd(Dc) + T)


def comirec_check_shape(D, Dc, K, R=None, T=None, mode="DR", Ns=None):
    """ValueError for sizes that describe no ComiRec body, NotImplementedError naming the limit for shapes the kernels do
    not cover (the ABI would return -2): key width D = E C, capsule width Dc, K capsules and -- where given -- R routing
    rounds and the series length T of mode 'DR' or 'SA', or the number of sampled items Ns of the hard attention."""
    sizes = [D, Dc, K] + [v for v in (R, T, Ns) if v is not None]
    if min(sizes) < 1:
        raise ValueError("every size of a ComiRec body must be positive, got D=%d, Dc=%d, capsules=%d, rounds=%r, T=%r, "
                         "Ns=%r" % (D, Dc, K, R, T, Ns))
    _caps_limits("ComiRec", D, Dc, K, R, "%r")
    if T is not None and mode == "DR":
        _lds_fit(comirec_dr_lds_bytes(T, Dc, R), "ComiRec dynamic routing holds one row (b, k)",
                 "T (Dc|1) + (2 R + 3) T + 2 R (Dc|1)", "T=%d, capsule width=%d, rounds=%d" % (T, Dc, R))
    if T is not None and mode == "SA":
        _lds_fit(comirec_sa_lds_bytes(T, D, Dc, K), "ComiRec self-attention holds one example",
                 "T (D|1) + 2 T (Dc|1) + 2 K T + 3 K (Dc|1) + T",
                 "T=%d, key width=%d, capsule width=%d, capsules=%d" % (T, D, Dc, K))
    if Ns is not None:
        _items_fit("ComiRec hard", Ns, Dc, K)


def _comirec_dr_args(embed, series, W, B0, R, padding_index, keep_padding):
    args, (V, E, B, T, Cn) = _series_head(embed, series, "dynamic routing", (W, "W [K,T,D,Dc]"), (B0, "B0 [K,T]"))
    K, Tw, D, Dc = W.shape
    if D != Cn * E or Tw != T or tuple(B0.shape) != (K, T):
        raise ValueError("dynamic routing: W must be [K, T = %d, C E = %d, Dc] and B0 [K, T]; got W %s, B0 %s"
                         % (T, Cn * E, tuple(W.shape), tuple(B0.shape)))
    comirec_check_shape(D, Dc, K, int(R), T=T, mode="DR")
    return args + [_ptr(W), _ptr(B0), Dc, K, int(R), int(padding_index), int(bool(keep_padding))], \
        (B, T, Cn, E, D, Dc, K)


def comirec_dr_fwd(embed, series, W, B0, routing_rounds=3, padding_index=0, keep_padding=True, oob=None):
    """ComiRecDynamicRoutingLayer over the looked-up series: series ids [B,T,C] into ``embed``, W [K,T,C E,Dc], B0 [K,T]
    -> the squashed capsules of the last round [B,K,Dc].  Position t takes part iff (series[b,t,0] == padding_index) ==
    keep_padding.  Nothing else is saved."""
    args, (B, T, Cn, E, D, Dc, K) = _comirec_dr_args(embed, series, W, B0, routing_rounds, padding_index, keep_padding)
    out = _new((B, K, Dc), embed.device)
    if B > 0:                                            # an empty batch answers from the sizes alone
        _call_ws("rec_comirec_dr_workspace_bytes", (B, T, E, Cn, Dc, K, int(routing_rounds)), "rec_comirec_dr_fwd_f32",
                 embed.device, *args, _ptr(out), _ptr(oob))
    return out


def comirec_dr_bwd(embed, series, W, B0, gout, routing_rounds=3, padding_index=0, keep_padding=True):
    """-> (gkeys [B,T,C E], the IndexedSlices values of the series lookups, dW [K,T,C E,Dc]) from gout [B,K,Dc]; the
    projection and the rounds are run again and differentiated through, all of them.  B0 has no gradient."""
    args, (B, T, Cn, E, D, Dc, K) = _comirec_dr_args(embed, series, W, B0, routing_rounds, padding_index, keep_padding)
    _expect(gout, (B, K, Dc), "gout", "[B,K,Dc]")
    dev = embed.device
    gkeys, dW = _new((B, T, D), dev), _new((K, T, D, Dc), dev, B)
    if B > 0:
        _call_ws("rec_comirec_dr_workspace_bytes", (B, T, E, Cn, Dc, K, int(routing_rounds)), "rec_comirec_dr_bwd_f32",
                 dev, *args, _ptr(gout), _ptr(gkeys), _ptr(dW))
    return gkeys, dW


def _comirec_sa_args(embed, series, W1, W2, pos, padding_index, keep_padding):
    args, (V, E, B, T, Cn) = _series_head(embed, series, "self-attention", (W1, "W1 [D,Dc]"), (W2, "W2 [K,Dc]"))
    D, Dc = W1.shape
    K = W2.shape[0]
    if D != Cn * E or W2.shape[1] != Dc:
        raise ValueError("self-attention: W1 must have C E = %d rows and W2 Dc = %d columns; got W1 %s, W2 %s"
                         % (Cn * E, Dc, tuple(W1.shape), tuple(W2.shape)))
    _expect(pos, (T, D), "pos", "[T,D]", optional=True)
    comirec_check_shape(D, Dc, K, T=T, mode="SA")
    return args + [_ptr(W1), _ptr(W2), _ptr(pos), Dc, K, int(padding_index), int(bool(keep_padding))], \
        (B, T, Cn, E, D, Dc, K)


def comirec_sa_fwd(embed, series, W1, W2, pos=None, padding_index=0, keep_padding=True, oob=None):
    """ComiRecSelfAttentiveLayer over the looked-up series in one launch: h = tanh((x + pos) W1), K heads h W2^T, masked
    softmax over the positions -> the weighted sums of h [B,K,Dc].  ``pos`` [T,C E] or None."""
    args, (B, T, Cn, E, D, Dc, K) = _comirec_sa_args(embed, series, W1, W2, pos, padding_index, keep_padding)
    out = _new((B, K, Dc), embed.device)
    if B > 0:
        _call("rec_comirec_sa_fwd_f32", *args, _ptr(out), _ptr(oob))
    return out


def comirec_sa_bwd(embed, series, W1, W2, gout, pos=None, padding_index=0, keep_padding=True):
    """-> (gkeys [B,T,C E], dW1 [C E,Dc], dW2 [K,Dc]) from gout [B,K,Dc]; ``pos`` is a constant."""
    args, (B, T, Cn, E, D, Dc, K) = _comirec_sa_args(embed, series, W1, W2, pos, padding_index, keep_padding)
    _expect(gout, (B, K, Dc), "gout", "[B,K,Dc]")
    dev = embed.device
    gkeys, dW1, dW2 = _new((B, T, D), dev), _new((D, Dc), dev, B), _new((K, Dc), dev, B)
    if B > 0:
        _call_ws("rec_comirec_sa_workspace_bytes", (B, T, E, Cn, Dc, K), "rec_comirec_sa_bwd_f32", dev, *args,
                 _ptr(gout), _ptr(gkeys), _ptr(dW1), _ptr(dW2))
    return gkeys, dW1, dW2


def _comirec_select_args(embed, items, m):
    args, (V, E, B, Ns, Cn) = _items_head(embed, items, m, "hard attention")
    K, Dc = m.shape[1:]
    if m.shape[0] != B or Dc != Cn * E:
        raise ValueError("hard attention: m must be [B, K, C E] = [%d, K, %d]; got %s" % (B, Cn * E, tuple(m.shape)))
    comirec_check_shape(Dc, Dc, K, Ns=Ns)
    return args + [_ptr(m), K], (B, Ns, Dc, K)


def comirec_select_fwd(embed, items, m, oob=None):
    """Hard attention of ComiRecLayer over the looked-up sampled items and the sampled-softmax loss in one launch: item
    ids [B,Ns,C] into ``embed``, capsules m [B,K,C E] -> (chosen int32 [B,Ns], the smallest index of the largest inner
    product; inner [B,Ns], that product; loss [B]) with the label at sample 0."""
    args, (B, Ns, Dc, K) = _comirec_select_args(embed, items, m)
    dev = embed.device
    chosen, inner, loss = _new((B, Ns), dev, dtype=torch.int32), _new((B, Ns), dev), _new((B,), dev)
    if B > 0:
        _call("rec_comirec_select_fwd_f32", *args, _ptr(chosen), _ptr(inner), _ptr(loss), _ptr(oob))
    return chosen, inner, loss


def comirec_select_bwd(embed, items, m, chosen, ginner=None, gloss=None, gsel=None):
    """-> (gm [B,K,C E], gitems [B,Ns,C E], the IndexedSlices values of the item lookups) from ginner [B,Ns] and / or
    gloss [B] and, optionally, gsel [B,Ns,C E], the gradient of the selected capsules, in one launch; ``chosen`` is the
    forward's.  With no gradient at all, zeros."""
    args, (B, Ns, Dc, K) = _comirec_select_args(embed, items, m)
    dev = embed.device
    _expect(chosen, (B, Ns), "chosen", "[B,Ns]", torch.int32)
    if ginner is None and gloss is None and gsel is None:
        return _new((B, K, Dc), dev, B=0), _new((B, Ns, Dc), dev, B=0)
    _expect(ginner, (B, Ns), "ginner", "[B,Ns]", optional=True)
    _expect(gloss, (B,), "gloss", "[B]", optional=True)
    _expect(gsel, (B, Ns, Dc), "gsel", "[B,Ns,Dc]", optional=True)
    if ginner is None and gloss is None:                 # the ABI wants one of the two: an all-zero gloss adds nothing
        gloss = _new((B,), dev, B=0)
    gm, gitems = _new((B, K, Dc), dev), _new((B, Ns, Dc), dev)
    if B > 0:
        _call("rec_comirec_select_bwd_f32", *args, _ptr(chosen), _ptr(ginner), _ptr(gloss), _ptr(gsel), _ptr(gm),
              _ptr(gitems))
    return gm, gitems


# ---- SINE: the sparse-interest extractor with its per-example top-K of L concepts, and the auxiliary loss of the concept
# pool (csrc/sine.hip).  Key width and K are MIND's limits, L and the LDS fit are the header's.
SINE_MAX_L = LIMITS["REC_SINE_MAX_L"]
SINE_LN_EPS = 1e-3


def sine_lds_bytes(T, D, L, K):
    """LDS of one example of either direction (include/mi355rec.h)."""
    return 4 * (4 * T * _odd(D) + 4 * K * T + L + 5 * K * _odd(D) + 6 * T + 8 * _odd(D) + 128)


def sine_check_shape(D, L, K, T=None):
    """ValueError for sizes that describe no SINE body, NotImplementedError naming the limit for shapes the kernels do
    not cover (the ABI would return -2): key width D = E C, L concepts of which every example selects K and -- where
    given -- the series length T."""
    sizes = [D, L, K] + ([] if T is None else [T])
    if min(sizes) < 1:
        raise ValueError("every size of a SINE body must be positive, got D=%d, L=%d, K=%d, T=%r" % (D, L, K, T))
    if D > DIN_MAX_D or L > SINE_MAX_L or K > min(L, AFM_MAX_A):
        raise NotImplementedError("SINE kernels cover key width <= %d, concepts L <= %d and selected concepts K <= "
                                  "min(L, %d); got key width=%d, L=%d, K=%d" % (DIN_MAX_D, SINE_MAX_L, AFM_MAX_A, D, L, K))
    if T is not None:
        _lds_fit(sine_lds_bytes(T, D, L, K), "SINE holds one example",
                 "4 T (D|1) + 4 K T + L + 5 K (D|1) + 6 T + 8 (D|1) + 128", "T=%d, key width=%d, L=%d, K=%d" % (T, D, L, K))


def _sine_args(embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, K, tau, ln_eps, padding_index):
    args, (V, E, B, T, Cn) = _series_head(embed, series, "sparse interest", (pool, "pool [L,D]"), (W1, "W1 [D,D]"),
                                          (W2, "W2 [D]"), (Wk1, "Wk1 [L,D,D]"), (Wk2, "Wk2 [L,D]"), (W3, "W3 [D,D]"),
                                          (W4, "W4 [D]"))
    L, D = pool.shape
    want = {"W1": (D, D), "W2": (D,), "Wk1": (L, D, D), "Wk2": (L, D), "W3": (D, D), "W4": (D,)}
    got = {"W1": W1, "W2": W2, "Wk1": Wk1, "Wk2": Wk2, "W3": W3, "W4": W4}
    if D != Cn * E or any(tuple(got[k].shape) != s for k, s in want.items()):
        raise ValueError("sparse interest: pool must be [L, C E = %d] and the weights %s; got pool %s, %s"
                         % (Cn * E, want, tuple(pool.shape), {k: tuple(t.shape) for k, t in got.items()}))
    if not (tau > 0 and ln_eps > 0):
        raise ValueError("sparse interest: tau and ln_eps must be positive, got %r and %r" % (tau, ln_eps))
    sine_check_shape(D, L, int(K), T=T)
    return args + [_ptr(pool), _ptr(W1), _ptr(W2), _ptr(Wk1), _ptr(Wk2), _ptr(W3), _ptr(W4), L, int(K), float(tau),
                   float(ln_eps), int(padding_index)], (B, T, Cn, E, D, L)


def sine_interest_fwd(embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, K, tau=0.1, ln_eps=SINE_LN_EPS, padding_index=0,
                      oob=None):
    """SINELayer.generate_user_interest over the looked-up series in one launch: series ids [B,T,C] into ``embed``, the
    concept pool [L,C E] and the six weights -> (user_interest [B,C E], chosen int32 [B,K]: every example's top-K concepts
    in descending-similarity order, the lower index first on equal values).  Nothing else is saved."""
    args, (B, T, Cn, E, D, L) = _sine_args(embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, K, tau, ln_eps, padding_index)
    dev = embed.device
    out, chosen = _new((B, D), dev), _new((B, int(K)), dev, B, dtype=torch.int32)
    if B > 0:
        _call("rec_sine_interest_fwd_f32", *args, _ptr(out), _ptr(chosen), _ptr(oob))
    return out, chosen


def sine_interest_bwd(embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, chosen, gout, tau=0.1, ln_eps=SINE_LN_EPS,
                      padding_index=0):
    """-> (gkeys [B,T,C E], the IndexedSlices values of the series lookups, dpool, dW1, dW2, dWk1, dWk2, dW3, dW4) from
    gout [B,C E]; ``chosen`` is the forward's and is never re-selected.  Every gradient is written in full: the rows of
    dpool, dWk1 and dWk2 that no example chose are zero."""
    K = chosen.shape[1] if isinstance(chosen, torch.Tensor) and chosen.dim() == 2 else 0
    args, (B, T, Cn, E, D, L) = _sine_args(embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, K, tau, ln_eps, padding_index)
    _expect(chosen, (B, K), "chosen", "[B,K]", torch.int32)
    _expect(gout, (B, D), "gout", "[B,D]")
    dev = embed.device
    gkeys = _new((B, T, D), dev)
    grads = [_new(tuple(t.shape), dev, B) for t in (pool, W1, W2, Wk1, Wk2, W3, W4)]
    if B > 0:
        _call_ws("rec_sine_scratch_bytes", (B, T, E, Cn, L, K), "rec_sine_interest_bwd_f32", dev, *args, _ptr(chosen),
                 _ptr(gout), _ptr(gkeys), *_ptrs(grads))
    return (gkeys, *grads)


def _sine_pool(pool):
    _req(pool, torch.float32, "pool")
    if pool.dim() != 2:
        raise ValueError("the auxiliary loss takes pool [L,D]; got %s" % (tuple(pool.shape),))
    L, D = pool.shape
    sine_check_shape(D, L, 1)
    return L, D


def sine_aux_fwd(pool):
    """SINELayer.compute_auxiliary_loss: 0.5 sum_{i != j} M_ij^2 of M = Cc Cc^T, Cc the centred pool -> a scalar tensor."""
    L, D = _sine_pool(pool)
    loss = _new((1,), pool.device)
    _call("rec_sine_aux_fwd_f32", _ptr(pool), L, D, _ptr(loss))
    return loss.reshape(())


def sine_aux_bwd(pool, gloss):
    """-> dpool [L,D] = gloss (2 offdiag(M) Cc) pushed back through the centring; gloss a one-element device tensor"""
    L, D = _sine_pool(pool)
    _req(gloss, torch.float32, "gloss")
    if gloss.numel() != 1:
        raise ValueError("gloss must hold one element, got %s" % (tuple(gloss.shape),))
    dpool = _new((L, D), pool.device)
    _call("rec_sine_aux_bwd_f32", _ptr(pool), L, D, _ptr(gloss), _ptr(dpool))
    return dpool


# ---- CAN co-action: both lookups and the per-example micro-MLP in one launch each way (csrc/can.hip).  The widest layer
# is AFM's embedding limit; layers, orders and the LDS fit are the header's.
CAN_MAX_W = AFM_MAX_E
CAN_MAX_LAYERS = CAN_MAX_ORDER = LIMITS["REC_CAN_MAX_L"]


def can_widths(E, coefs):
    """[E, E c_1, ..., E c_n]: the layer widths of a co-action MLP"""
    return [int(E)] + [int(E) * int(c) for c in coefs]


def can_row_floats(E, coefs):
    """P: the floats of an induction row, W_l [w_l, w_l+1] then B_l, layer after layer"""
    w = can_widths(E, coefs)
    return sum(a * b + b for a, b in zip(w[:-1], w[1:]))


def can_lds_bytes(T, E, coefs, order):
    """LDS of one example of the co-action backward (include/mi355rec.h): what both directions are held to."""
    w = can_widths(E, coefs)
    w = w[:min(len(coefs), order) + 1]                   # the layers applied
    pv = sum(a * _odd(b) + b for a, b in zip(w[:-1], w[1:]))
    return 4 * (2 * T * E + pv + T * sum(_odd(x) for x in w) + 2 * T * _odd(max(w)) + T + 256)


def can_check_shape(E, coefs, order, T=None):
    """ValueError for sizes that describe no co-action unit, NotImplementedError naming the limit for shapes the kernels
    do not cover (the ABI would return -2): feed width E, layer_unit_coef, order and -- where given -- the number of feed
    positions T of an example."""
    coefs = [int(c) for c in coefs]
    sizes = [E, order, len(coefs)] + coefs + ([T] if T is not None else [])
    if min(sizes) < 1:
        raise ValueError("every size of a co-action unit must be positive (and layer_unit_coef not empty), got "
                         "feed_feature_dim=%d, layer_unit_coef=%r, order=%d, T=%r" % (E, coefs, order, T))
    if max(can_widths(E, coefs)) > CAN_MAX_W or len(coefs) > CAN_MAX_LAYERS or order > CAN_MAX_ORDER:
        raise NotImplementedError(
            "CAN kernels cover layer widths feed_feature_dim * coef <= %d, at most %d layers and order <= %d; got "
            "feed_feature_dim=%d, layer_unit_coef=%r, order=%d" % (CAN_MAX_W, CAN_MAX_LAYERS, CAN_MAX_ORDER, E, coefs, order))
    if T is not None:
        _lds_fit(can_lds_bytes(T, E, coefs, order), "the CAN co-action holds one example",
                 "2 T E + Pv + T sum (w_l|1) + 2 T (wmax|1) + T + 256",
                 "T=%d, feed_feature_dim=%d, layer_unit_coef=%r, order=%d" % (T, E, coefs, order))


def _can_args(feed, inds, iid, fid, coefs, order, act, padding_index):
    _table(feed, "feed"); _i64(iid, "iid"); _i64(fid, "fid")
    inds = list(inds)
    if len(inds) not in (1, int(order)):
        raise ValueError("co-action takes one induction table per order (%d) or one shared table; got %d"
                         % (order, len(inds)))
    for t in inds:
        _table(t, "induction table")
    if iid.dim() != 1 or fid.dim() != 2 or fid.shape[0] != iid.shape[0]:
        raise ValueError("co-action takes iid [B] and fid [B,T]; got %s, %s" % (tuple(iid.shape), tuple(fid.shape)))
    Vf, E = feed.shape
    Vi, P = inds[0].shape
    B, T = fid.shape
    if any(tuple(t.shape) != (Vi, P) or t.stride(0) != inds[0].stride(0) for t in inds) or P != can_row_floats(E, coefs):
        raise ValueError("co-action: every induction table must be [Vi, P = %d] with one row stride for feed width %d "
                         "and layer_unit_coef %r; got %s" % (can_row_floats(E, coefs), E, list(coefs),
                                                             [tuple(t.shape) for t in inds]))
    if act not in (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH):
        raise ValueError("co-action: unknown activation code %r" % (act,))
    if T < 1:
        raise ValueError("co-action: fid must have at least one position, got %s" % (tuple(fid.shape),))
    can_check_shape(E, coefs, int(order), T=T)
    shared = int(len(inds) == 1 and int(order) > 1)
    La = min(len(coefs), int(order))
    return [_ptr(feed), feed.stride(0), Vf, E, _ptr_array(inds), shared, inds[0].stride(0), Vi, len(coefs),
            _ints(coefs), int(order), int(act), _ptr(iid), _ptr(fid), B, T, int(padding_index)], \
        (B, T, E, P, can_widths(E, coefs)[La])


def can_fwd(feed, inds, iid, fid, coefs, order, act, padding_index=0, pooled=False, oob=None):
    """CoActionUnit over both lookups in one launch: feed table [Vf,E], ``inds`` the induction tables [Vi,P] (one per
    order, or one shared), iid [B], fid [B,T] -> out [order,B,T,Eo], or with ``pooled`` its sum over orders and positions
    [B,Eo].  min(len(coefs), order) layers are applied; a position whose feed id is ``padding_index`` is zero."""
    args, (B, T, E, P, Eo) = _can_args(feed, inds, iid, fid, coefs, order, act, padding_index)
    shape = (B, Eo) if pooled else (int(order), B, T, Eo)
    res = _new(shape, feed.device)
    if B > 0:                                            # an empty batch answers from the sizes alone
        _call("rec_can_fwd_f32", *args, None if pooled else _ptr(res), _ptr(res) if pooled else None, _ptr(oob))
    return res


def can_bwd(feed, inds, iid, fid, coefs, order, act, g, padding_index=0, pooled=False):
    """-> (gfeed [B,T,E], the IndexedSlices values of the feed lookups summed over the orders, gind [order,B,P], those of
    each order's induction lookup) from gout [order,B,T,Eo] or, with ``pooled``, gpool [B,Eo]; the forward is run again."""
    args, (B, T, E, P, Eo) = _can_args(feed, inds, iid, fid, coefs, order, act, padding_index)
    shape = (B, Eo) if pooled else (int(order), B, T, Eo)
    _expect(g, shape, "g", "the upstream gradient")
    gfeed, gind = _new((B, T, E), feed.device), _new((int(order), B, P), feed.device)
    if B > 0:
        _call("rec_can_bwd_f32", *args, None if pooled else _ptr(g), _ptr(g) if pooled else None, _ptr(gfeed), _ptr(gind))
    return gfeed, gind


# ---- FinalMLP: the two gates, the gating, both BatchNorm-MLP streams and the bilinear head over ONE packed parameter
# buffer (csrc/finalmlp.hip).  The limits are MaskNet's.
def finalmlp_check_shape(D, D1, D2, Hg1, Hg2, widths1, widths2, n, o):
    """ValueError for sizes that describe no FinalMLP body, NotImplementedError naming the limit for shapes the kernels do
    not cover (the ABI would return -2): shared width D, gate input widths D1 / D2 and hidden widths Hg1 / Hg2, the
    stream widths, n heads, o outputs."""
    widths1, widths2 = [int(w) for w in widths1], [int(w) for w in widths2]
    if len(widths1) != len(widths2) or not widths1 or min([D, D1, D2, Hg1, Hg2, n, o] + widths1 + widths2) < 1:
        raise ValueError("a FinalMLP body has positive sizes and two streams of the same depth >= 1, got D=%d, D1=%d, "
                         "D2=%d, Hg1=%d, Hg2=%d, mlp1=%r, mlp2=%r, num_heads=%d, output_dim=%d"
                         % (D, D1, D2, Hg1, Hg2, widths1, widths2, n, o))
    if widths1[-1] % n or widths2[-1] % n:
        raise ValueError("num_heads=%d must divide the last width of both streams, got %d and %d"
                         % (n, widths1[-1], widths2[-1]))
    if (max(D, D1, D2) > MASKNET_MAX_D or max([Hg1, Hg2] + widths1 + widths2) > MASKNET_MAX_O
            or len(widths1) > MASKNET_MAX_R or o > MASKNET_MAX_R or widths2[-1] // n * o > MASKNET_MAX_O):
        raise NotImplementedError(
            "FinalMLP kernels cover fields * embedding_dims and both gate inputs <= %d, gate hidden and stream widths <= "
            "%d, 1..%d stream layers, output_dim <= %d and (mlp2 width / num_heads) * output_dim <= %d; got D=%d, D1=%d, "
            "D2=%d, Hg1=%d, Hg2=%d, mlp1=%r, mlp2=%r, num_heads=%d, output_dim=%d"
            % (MASKNET_MAX_D, MASKNET_MAX_O, MASKNET_MAX_R, MASKNET_MAX_R, MASKNET_MAX_O, D, D1, D2, Hg1, Hg2, widths1,
               widths2, n, o))


def finalmlp_param_shapes(D, D1, D2, Hg1, Hg2, widths1, widths2, n, o):
    """[(name, shape)] of the packed parameters, in the order include/mi355rec.h lays them end to end"""
    out = []
    for s, (Dx, Hg) in enumerate(((D1, Hg1), (D2, Hg2)), 1):
        out += [("Wh_%d" % s, (Dx, Hg)), ("bh_%d" % s, (Hg,)), ("Wo_%d" % s, (Hg, D)), ("bo_%d" % s, (D,))]
    for s, widths in enumerate((widths1, widths2), 1):
        d = D
        for l, w in enumerate(widths):
            out += [("W_%d_%d" % (s, l), (d, w))] + [("%s_%d_%d" % (k, s, l), (w,)) for k in ("b", "gamma", "beta")]
            d = w
    d1, d2 = widths1[-1], widths2[-1]
    return out + [("W_1", (d1, o)), ("c_1", (o,)), ("W_2", (d2, o)), ("c_2", (o,)), ("W_12", (n, d1 // n, d2 // n, o))]


def _finalmlp_args(xs, x1, x2, params, dims):
    Hg1, Hg2, widths1, widths2, n, o = dims
    for t, name in ((xs, "xs"), (x1, "x1"), (x2, "x2")):
        if _f32(t, name).dim() != 2 or t.shape[0] != xs.shape[0]:
            raise ValueError("a FinalMLP body takes xs [B,D], x1 [B,D1], x2 [B,D2]; got %s"
                             % ", ".join(str(tuple(t.shape)) for t in (xs, x1, x2)))
    (B, D), D1, D2 = xs.shape, x1.shape[1], x2.shape[1]
    finalmlp_check_shape(D, D1, D2, Hg1, Hg2, widths1, widths2, n, o)
    shapes = finalmlp_param_shapes(D, D1, D2, Hg1, Hg2, widths1, widths2, n, o)
    total = 0
    for _, shape in shapes:
        cnt = 1
        for v in shape:
            cnt *= v
        total += cnt
    _expect(params, (total,), "params", "the packed parameters")
    sizes = (B, D, D1, D2, int(Hg1), int(Hg2), len(widths1), _ints(widths1), _ints(widths2), int(n), int(o))
    return sizes, sum(widths1) + sum(widths2)


def finalmlp_fwd(xs, x1, x2, params, moving_mean, moving_var, dims, training, eps=1e-3, momentum=0.99, save=True):
    """The FinalMLP body: xs [B,D] the shared rows, x1 / x2 the rows of the two gates, ``params`` the packed parameters
    (finalmlp_param_shapes), ``moving_mean`` / ``moving_var`` the 2 L moving statistics (stream 1 layer 0 .., then stream
    2), ``dims`` = (Hg1, Hg2, widths1, widths2, num_heads, output_dim) -> (out [B,o], saved) with saved = (hg [B,Hg1+Hg2],
    g [B,2 D], z [B,Z], a [B,Z], stats [2,Z]) or None.  ``training``: batch statistics in 2 L + 1 launches, and the moving
    statistics move in place on the device; else the moving statistics in one launch."""
    sizes, Z = _finalmlp_args(xs, x1, x2, params, dims)
    B, D, L, o = sizes[0], sizes[1], sizes[6], sizes[10]
    widths = list(dims[2]) + list(dims[3])
    if len(moving_mean) != 2 * L or len(moving_var) != 2 * L:
        raise ValueError("a FinalMLP body takes %d moving means and variances, got %d and %d"
                         % (2 * L, len(moving_mean), len(moving_var)))
    for t, w in zip(list(moving_mean) + list(moving_var), widths + widths):
        _expect(t, (w,), "moving statistic")
    if training and not save:
        raise ValueError("the batch-statistics forward keeps its save buffers: z carries the chain between launches")
    dev = xs.device
    out = _new((B, o), dev)
    saved = tuple(_new(s, dev, B) for s in ((B, dims[0] + dims[1]), (B, 2 * D), (B, Z), (B, Z), (2, Z))) if save else None
    if B > 0:
        args = (_ptr(xs), _ptr(x1), _ptr(x2), _ptr(params), _ptr_array(moving_mean), _ptr_array(moving_var), *sizes,
                int(bool(training)), float(eps), float(momentum), _ptr(out), *_ptrs(saved or (None,) * 5))
        if training:
            _call_ws("rec_finalmlp_scratch_bytes", sizes, "rec_finalmlp_fwd_f32", dev, *args)
        else:
            _call("rec_finalmlp_fwd_f32", *args, None, 0)
    return out, saved


def finalmlp_bwd(xs, x1, x2, params, saved, out, dout, dims, training):
    """-> (dxs [B,D], dx1 [B,D1], dx2 [B,D2], dparams in the layout of ``params``)"""
    sizes, Z = _finalmlp_args(xs, x1, x2, params, dims)
    B, D, o = sizes[0], sizes[1], sizes[10]
    shapes = ((B, dims[0] + dims[1]), (B, 2 * D), (B, Z), (B, Z), (2, Z), (B, o), (B, o))
    _expect_all(zip(tuple(saved) + (out, dout), shapes, ("hg", "g", "z", "a", "stats", "out", "dout")))
    dxs, dx1, dx2, dparams = (_new_like(t, B) for t in (xs, x1, x2, params))
    if B > 0:
        _call_ws("rec_finalmlp_scratch_bytes", sizes, "rec_finalmlp_bwd_f32", xs.device, _ptr(xs), _ptr(x1), _ptr(x2),
                 _ptr(params), *_ptrs(saved), _ptr(out), _ptr(dout), *sizes, int(bool(training)), _ptr(dxs), _ptr(dx1),
                 _ptr(dx2), _ptr(dparams))
    return dxs, dx1, dx2, dparams


# ---- DMR: both attention units over the behaviour series and the auxiliary match loss, one launch each way
# (csrc/dmr.hip).  Key width and hidden width share DIN's key-width limit; the LDS fit is the header's formula.
def dmr_lds_bytes(T, D, H, Nn):
    """LDS of one example of either direction (include/mi355rec.h)."""
    return 4 * (T * (_odd(D) + _odd(2 * H) + 7) + Nn * (_odd(D) + 3) + 8 * _odd(D) + 5 * H + 16)


def dmr_check_shape(D, H, T=None, Nn=None):
    """ValueError for sizes that describe no DMR body, NotImplementedError naming the limit for shapes the kernels do not
    cover (the ABI would return -2): key width D = E C, hidden width H of both units and -- where both are given -- the
    series length T and the number of negatives Nn per example."""
    sizes = [D, H] + [v for v in (T, Nn) if v is not None]
    if min(sizes) < 1:
        raise ValueError("every size of a DMR body must be positive, got D=%d, H=%d, T=%r, Nn=%r" % (D, H, T, Nn))
    if D > DIN_MAX_D or H > DIN_MAX_D:
        raise NotImplementedError("DMR kernels cover key width and hidden width <= %d; got key width=%d, hidden width=%d"
                                  % (DIN_MAX_D, D, H))
    if T is not None and Nn is not None:
        _lds_fit(dmr_lds_bytes(T, D, H, Nn), "DMR holds one example",
                 "T ((D|1) + (2H|1) + 7) + Nn ((D|1) + 3) + 8 (D|1) + 5 H + 16",
                 "T=%d, key width=%d, hidden width=%d, Nn=%d" % (T, D, H, Nn))


def _dmr_args(embed, series, negatives, xi, q, P, We, z, padding_index):
    args, (V, E, B, T, Cn) = _series_head(embed, series, "DMR match", (negatives, "negatives [B,Nn,C]", torch.int64),
                                          (xi, "xi [B,D]"), (q, "q [B,H]"), (P, "P [T,2H]"), (We, "We [D,2H]"),
                                          (z, "z [2,H]"))
    D, H, Nn = Cn * E, z.shape[1], negatives.shape[1]
    want = {"negatives": (B, Nn, Cn), "xi": (B, D), "q": (B, H), "P": (T, 2 * H), "We": (D, 2 * H), "z": (2, H)}
    got = {"negatives": negatives, "xi": xi, "q": q, "P": P, "We": We, "z": z}
    if any(tuple(got[k].shape) != s for k, s in want.items()):
        raise ValueError("DMR match: with series %s and z %s the operands must be %s; got %s"
                         % (tuple(series.shape), tuple(z.shape), want, {k: tuple(t.shape) for k, t in got.items()}))
    dmr_check_shape(D, H, T=T, Nn=Nn)
    return args + [_ptr(negatives), Nn, _ptr(xi), _ptr(q), _ptr(P), _ptr(We), _ptr(z), H, int(padding_index)], \
        (B, T, Cn, E, D, H, Nn)


def dmr_fwd(embed, series, negatives, xi, q, P, We, z, padding_index=0, oob=None):
    """DMRI2INetworkLayer, DMRU2INetworkLayer and compute_auxiliary_loss over the looked-up series and negatives in one
    launch: series ids [B,T,C] and negative ids [B,Nn,C] into ``embed``, the candidate's rows xi [B,C E], q = xi Wc [B,H],
    P = pos [Wp_i2i | Wp_u2i] [T,2H], We = [We_i2i | We_u2i] [C E,2H], z = [z_i2i; z_u2i] [2,H] -> (i2i [B,C E + 1]:
    pooled series | score sum, u2i [B,C E + 1]: pooled series | its inner product with xi, aux [B]).  An example with no
    valid position gives zeros.  Nothing else is saved."""
    args, (B, T, Cn, E, D, H, Nn) = _dmr_args(embed, series, negatives, xi, q, P, We, z, padding_index)
    dev = embed.device
    i2i, u2i, aux = _new((B, D + 1), dev, B), _new((B, D + 1), dev, B), _new((B,), dev, B)
    if B > 0:                                            # an empty batch answers from the sizes alone
        _call("rec_dmr_fwd_f32", *args, _ptr(i2i), _ptr(u2i), _ptr(aux), _ptr(oob))
    return i2i, u2i, aux


def dmr_bwd(embed, series, negatives, xi, q, P, We, z, g_i2i=None, g_u2i=None, g_aux=None, padding_index=0, gkeys=None,
            gneg=None):
    """-> (gkeys [B,T,C E] and gneg [B,Nn,C E], the IndexedSlices values of the two lookups, gitem [B,C E] (through the
    inner product alone), gq [B,H], dP [T,2H], dWe [C E,2H], dz [2,H]) from g_i2i [B,C E + 1], g_u2i [B,C E + 1] and
    g_aux [B], each of which may be None (exact zeros); the forward is run again from the ids.  ``gkeys`` / ``gneg``:
    optional preallocated contiguous destinations (the tail of a shared value buffer)."""
    args, (B, T, Cn, E, D, H, Nn) = _dmr_args(embed, series, negatives, xi, q, P, We, z, padding_index)
    dev = embed.device
    _expect(g_i2i, (B, D + 1), "g_i2i", "[B,D+1]", optional=True)
    _expect(g_u2i, (B, D + 1), "g_u2i", "[B,D+1]", optional=True)
    _expect(g_aux, (B,), "g_aux", "[B]", optional=True)
    if gkeys is None:
        gkeys = _new((B, T, D), dev, B)
    if gneg is None:
        gneg = _new((B, Nn, D), dev, B)
    _expect(gkeys, (B, T, D), "gkeys", "[B,T,D]")
    _expect(gneg, (B, Nn, D), "gneg", "[B,Nn,D]")
    gitem, gq = _new((B, D), dev, B), _new((B, H), dev, B)
    dP, dWe, dz = _new((T, 2 * H), dev, B), _new((D, 2 * H), dev, B), _new((2, H), dev, B)
    if B > 0:
        _call_ws("rec_dmr_scratch_bytes", (B, T, E, Cn, H, Nn), "rec_dmr_bwd_f32", dev, *args, _ptr(g_i2i), _ptr(g_u2i),
                 _ptr(g_aux), _ptr(gkeys), _ptr(gneg), _ptr(gitem), _ptr(gq), _ptr(dP), _ptr(dWe), _ptr(dz))
    return gkeys, gneg, gitem, gq, dP, dWe, dz


# ---- PEPNet: the lookup fused with the EPNet gates (csrc/epnet.hip) and the T gated MLPs of the towers, one launch each
# way (csrc/poso.hip).  The limits are MaskNet's: a gate's hidden width is held to MAX_E, tasks and chained layers to
# MAX_R.
EPNET_MAX_HG, POSO_MAX_T, POSO_MAX_L = MASKNET_MAX_E, MASKNET_MAX_R, MASKNET_MAX_R
_POSO_LDS_CAP = LIMITS["REC_POSO_LDS_CAP"]
_POSO_ACTS = (ACT_NONE, ACT_RELU, ACT_SIGMOID)


def _even(n):
    return (n + 1) & ~1


def epnet_check_shape(F, P, E, Hg=16):
    """ValueError for sizes that describe no EPNet lookup, NotImplementedError for shapes the kernel does not cover (the
    ABI would return -2): F main fields, P personalisation fields, embedding width E, gate hidden width Hg."""
    if min(F, P, E, Hg) < 1:
        raise ValueError("every size of an EPNet lookup must be positive, got fields=%d, ppnet fields=%d, "
                         "embedding_dims=%d, gate_hidden_dim=%d" % (F, P, E, Hg))
    if (F > MASKNET_MAX_F or E > MASKNET_MAX_E or Hg > EPNET_MAX_HG or P * E > MASKNET_MAX_O
            or (F + P) * E > MASKNET_MAX_D):
        raise NotImplementedError(
            "EPNet kernels cover fields <= %d, embedding_dims <= %d, gate_hidden_dim <= %d, ppnet fields * embedding_dims "
            "<= %d and (fields + ppnet fields) * embedding_dims <= %d; got fields=%d, embedding_dims=%d, "
            "gate_hidden_dim=%d, ppnet fields * embedding_dims=%d, (fields + ppnet fields) * embedding_dims=%d"
            % (MASKNET_MAX_F, MASKNET_MAX_E, EPNET_MAX_HG, MASKNET_MAX_O, MASKNET_MAX_D, F, E, Hg, P * E, (F + P) * E))


def poso_mlp_check_shape(Dm, Dg, T, units, m=2):
    """ValueError for sizes that describe no POSO-MLP, NotImplementedError for shapes the kernel does not cover (the ABI
    would return -2): main and gate input widths, T tasks, the widths of the chained layers, gate_hidden_multiple."""
    units = [int(u) for u in units]
    if min([Dm, Dg, T, m, len(units)] + units) < 1:
        raise ValueError("every size of a POSO-MLP must be positive, got main=%d, gate=%d, tasks=%d, units=%s, "
                         "gate_hidden_multiple=%d" % (Dm, Dg, T, units, m))
    L, Um = len(units), max(units)
    lds = 132 * (_even(Dg) + max(_even(m * Um), _even(Dm)) + (2 if L > 1 else 1) * _even(Um))
    if (T > POSO_MAX_T or L > POSO_MAX_L or Um > MASKNET_MAX_O or m * Um > MASKNET_MAX_P
            or max(Dm, Dg) > MASKNET_MAX_D or lds > _POSO_LDS_CAP):
        raise NotImplementedError(
            "POSO-MLP kernels cover tasks <= %d, layers <= %d, units <= %d, gate_hidden_multiple * units <= %d, input "
            "widths <= %d and a tile of %d bytes of LDS; got tasks=%d, units=%s, gate_hidden_multiple=%d, main=%d, "
            "gate=%d, a tile of %d bytes" % (POSO_MAX_T, POSO_MAX_L, MASKNET_MAX_O, MASKNET_MAX_P, MASKNET_MAX_D,
                                            _POSO_LDS_CAP, T, units, m, Dm, Dg, lds))


def pepnet_check_shape(F, P, E, Hg=16, T=3, units=(64, 16, 1), m=2, chain_layers=False):
    """Both kernels of a PEPNet of F main and P personalisation fields of width E: the EPNet lookup and the T towers
    (the last layer alone unless ``chain_layers``) over its output."""
    epnet_check_shape(F, P, E, Hg)
    poso_mlp_check_shape(F * E, (F + P) * E, T, list(units) if chain_layers else list(units)[-1:], m)


def _epnet_args(table, ids, F, A, a, Bm, bm):
    _table(table, "table")
    if _i64(ids, "ids").dim() != 2:
        raise ValueError("ids must be [B, fields + ppnet fields], got %s" % (tuple(ids.shape),))
    for t, name, dim in ((A, "A", 3), (a, "a", 2), (Bm, "Bm", 3), (bm, "bm", 2)):
        if _f32(t, name).dim() != dim:
            raise ValueError("%s must be %d-D, got %s" % (name, dim, tuple(t.shape)))
    B, FP = ids.shape
    V, E = table.shape
    P = FP - int(F)
    Hg = A.shape[2]
    if (P < 1 or tuple(A.shape) != (F, P * E, Hg) or tuple(a.shape) != (F, Hg) or tuple(Bm.shape) != (F, Hg, E)
            or tuple(bm.shape) != (F, E)):
        raise ValueError("an EPNet lookup takes ids [B,F+P] with P >= 1, A [F,P E,Hg], a [F,Hg], Bm [F,Hg,E], bm [F,E]; "
                         "got F=%d and %s" % (F, ", ".join(str(tuple(t.shape)) for t in (ids, A, a, Bm, bm))))
    epnet_check_shape(F, P, E, Hg)
    return B, V, E, P, Hg


def epnet_lookup_fwd(table, ids, F, A, a, Bm, bm, oob=None):
    """ids [B, F + P] into one table [V, E] -> u [B, (F + P) E]: the F main rows scaled by their GateNU of the P
    personalisation rows, then those rows raw (include/mi355rec.h).  An id out of range reads row 0 and sets ``oob``."""
    B, V, E, P, Hg = _epnet_args(table, ids, F, A, a, Bm, bm)
    u = _new((B, (F + P) * E), table.device, B)
    if B > 0:
        _call("rec_epnet_lookup_fwd_f32", _ptr(table), V, table.stride(0), _ptr(ids), *_ptrs((A, a, Bm, bm)), B, F, P, E,
              Hg, _ptr(u), _ptr(oob))
    return u


def epnet_lookup_bwd(table, ids, F, A, a, Bm, bm, du):
    """-> (drows [B (F + P), E], the IndexedSlices values of the lookup, (dA, da, dBm, dbm)) from du [B, (F + P) E]; the
    gates are computed again from the ids."""
    B, V, E, P, Hg = _epnet_args(table, ids, F, A, a, Bm, bm)
    _expect_all(((du, (B, (F + P) * E), "du"),))
    dev = table.device
    drows = _new((B * (F + P), E), dev, B)
    grads = [_new_like(t, B) for t in (A, a, Bm, bm)]
    if B > 0:
        _call_ws("rec_epnet_lookup_scratch_bytes", (B, F, P, E, Hg), "rec_epnet_lookup_bwd_f32", dev, _ptr(table), V,
                 table.stride(0), _ptr(ids), *_ptrs((A, a, Bm, bm)), _ptr(du), B, F, P, E, Hg, _ptr(drows),
                 *_ptrs(grads))
    return drows, grads


_POSO_WEIGHTS = ("Wg1", "bg1", "Wg2", "bg2", "W", "b", "C")


def _rows(t, name):
    """a 2-D fp32 operand on the device whose rows may be strided (a column block of a wider buffer)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on the MI355X (got %r): the HIP path has no CPU fallback"
                           % (name, getattr(t, "device", type(t))))
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1])):
        raise ValueError("%s must be a 2-D fp32 tensor with unit inner stride, got %s" % (name, tuple(t.shape)))
    return t


def _poso_args(x, g, w, units, acts, m):
    """-> (B, Dm, Dg, T, L, units, act codes) of the packed weights ``w`` (in the order of _POSO_WEIGHTS), checked against
    each other and the limits."""
    Wg1, bg1, Wg2, bg2, W, b, Cc = w
    _rows(x, "x"); _rows(g, "g")
    units = [int(u) for u in units]
    L = len(units)
    if len(acts) != L:
        raise ValueError("a POSO-MLP needs one activation per layer, got %d for %d layers" % (len(acts), L))
    codes = []
    for act in acts:
        code = ACT_CODE.get(act, act) if not isinstance(act, int) else act
        if code not in _POSO_ACTS:
            raise NotImplementedError("POSO-MLP kernels cover the activations 'relu', 'sigmoid' and 'linear', got %r"
                                      % (act,))
        codes.append(code)
    if _f32(Cc, "C").dim() != 2 or Cc.shape[1] != L or _f32(Wg1, "Wg1").dim() != 2:
        raise ValueError("a POSO-MLP takes C [T,L] and Wg1 [Dg,NG]; got %s, %s for %d layers"
                         % (tuple(Cc.shape), tuple(Wg1.shape), L))
    B, Dm = x.shape
    Dg, T = g.shape[1], Cc.shape[0]
    if g.shape[0] != B:
        raise ValueError("x and g differ in batch: %s, %s" % (tuple(x.shape), tuple(g.shape)))
    poso_mlp_check_shape(Dm, Dg, T, units, m)
    sumU = sum(units)
    ks = [Dm] + units[:-1]
    if tuple(Wg1.shape) != (Dg, T * m * sumU):
        raise ValueError("Wg1 must be [Dg, T m sum(units)] = %s, got %s" % ((Dg, T * m * sumU), tuple(Wg1.shape)))
    for t, cnt, name in ((bg1, T * m * sumU, "bg1"), (Wg2, T * sum(m * u * u for u in units), "Wg2"),
                         (bg2, T * sumU, "bg2"), (W, T * sum(k * u for k, u in zip(ks, units)), "W"),
                         (b, T * sumU, "b")):
        _vec(t, cnt, name)
    return B, Dm, Dg, T, L, units, codes


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def poso_mlp_fwd(x, g, weights, units, acts, m=2, save=True):
    """T stacked POSO-MLPs of chained layers in one launch: x [B, Dm] and g [B, Dg] (rows may be strided: column blocks
    of one buffer) -> (out [B, T, units[-1]], saved) with saved = (h [B, NG], gate, d, a [B, T sum(units)]) for the
    backward, or None (``save=False``: inference, only out is written).  ``weights``: Wg1, bg1, Wg2, bg2, W, b, C as
    include/mi355rec.h packs them."""
    B, Dm, Dg, T, L, units, codes = _poso_args(x, g, weights, units, acts, m)
    dev, sumU = x.device, sum(units)
    out = _new((B, T, units[-1]), dev, B)
    saved = tuple(_new((B, w), dev, B) for w in (T * m * sumU, T * sumU, T * sumU, T * sumU)) if save else None
    if B > 0:
        _call("rec_poso_mlp_fwd_f32", _ptr(x), _ld(x), _ptr(g), _ld(g), *_ptrs(weights), B, Dm, Dg, T, L, _ints(units),
              _ints(codes), int(m), _ptr(out), *_ptrs(saved or (None,) * 4))
    return out, saved


def poso_mlp_bwd(x, g, weights, saved, dout, units, acts, m=2):
    """-> (dx [B, Dm], dg [B, Dg], grads) with grads the gradient of every packed weight, in the order of ``weights``."""
    B, Dm, Dg, T, L, units, codes = _poso_args(x, g, weights, units, acts, m)
    sumU = sum(units)
    shapes = ((B, T * m * sumU),) + ((B, T * sumU),) * 3 + ((B, T, units[-1]),)
    _expect_all(zip(tuple(saved) + (dout,), shapes, ("h", "gate", "d", "a", "dout")))
    dev = x.device
    dx, dg = _new((B, Dm), dev, B), _new((B, Dg), dev, B)
    grads = [_new_like(t, B) for t in weights]
    if B > 0:
        Wg1, _, Wg2, _, W, _, Cc = weights
        _call_ws("rec_poso_mlp_scratch_bytes", (B, Dm, Dg, T, L, _ints(units), int(m)), "rec_poso_mlp_bwd_f32", dev,
                 _ptr(x), _ld(x), _ptr(g), _ld(g), *_ptrs((Wg1, Wg2, W, Cc)), *_ptrs(saved), _ptr(dout), B, Dm, Dg, T, L,
                 _ints(units), _ints(codes), int(m), _ptr(dx), _ptr(dg), *_ptrs(grads))
    return dx, dg, grads


# ---- DIEN: the masked Keras GRU of the interest extractor fused with the series / negative lookups and the auxiliary
# loss, and the attention scores fused with the AGRU / AUGRU of the interest evolution (csrc/dien.hip).  Every width is
# H = E C, held to DIN's wide key width; the LDS fit is the header's formula.
DIEN_GRU, DIEN_AUGRU, DIEN_AGRU = (ENUMS["REC_DIEN_" + k] for k in ("GRU", "AUGRU", "AGRU"))
DIEN_MODE = {"AUGRU": DIEN_AUGRU, "AGRU": DIEN_AGRU}


def dien_lds_bytes(T, H, mode=None):
    """LDS of a tile of 32 examples (include/mi355rec.h): the extractor (``mode`` None) or the evolution"""
    He = _even(H)
    if mode is None:
        return 132 * 8 * He + 512
    return 132 * ((7 if mode == DIEN_AUGRU else 6) * He + 2 * T) + 512


def dien_check_shape(H, T=None, mode=None):
    """ValueError for sizes that describe no DIEN body, NotImplementedError naming the limit for shapes the kernels do
    not cover (the ABI would return -2): the width H = E C of the series rows and of both recurrences, the series length
    T and -- for the evolution -- ``mode`` (DIEN_AUGRU / DIEN_AGRU)."""
    if min([H] + ([T] if T is not None else [])) < 1:
        raise ValueError("every size of a DIEN body must be positive, got H=%d, T=%r" % (H, T))
    if mode not in (None, DIEN_AUGRU, DIEN_AGRU):
        raise ValueError("the evolution's mode must be DIEN_AUGRU or DIEN_AGRU, got %r" % (mode,))
    if H > DIN_WIDE_D:
        raise NotImplementedError("DIEN kernels cover a width embedding_dims * series features <= %d; got %d"
                                  % (DIN_WIDE_D, H))
    if T is not None:
        _lds_fit(dien_lds_bytes(T, H, mode), "DIEN holds a tile of 32 examples",
                 "33 (8 He)" if mode is None else "33 ((7 or 6) He + 2 T) + 128", "T=%d, H=%d" % (T, H))


def _dien_gru_args(embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias, padding_index):
    """the leading ABI arguments of rec_dien_gru_* and (B, T, H, V, E, C): table mode (embed, series [B,T,C] and
    optionally negatives [B,T,C]) or dense mode (x [B,T,H], mask_ids [B,T])"""
    if (embed is None) == (x is None):
        raise ValueError("a DIEN GRU takes a table with series ids, or dense rows x with mask ids, not both")
    if embed is not None:
        head, (V, E, B, T, Cn) = _series_head(embed, series, "DIEN GRU")
        H = Cn * E
        if negatives is not None:
            _expect(negatives, (B, T, Cn), "negatives", "[B,T,C]", dtype=torch.int64)
        lead = head[:6] + [_ptr(negatives), None, None, B, T, H]
    else:
        if negatives is not None or series is not None:
            raise ValueError("the dense mode of a DIEN GRU takes no series or negative ids")
        if _f32(x, "x").dim() != 3:
            raise ValueError("x must be [B,T,H], got %s" % (tuple(x.shape),))
        B, T, H = x.shape
        _expect(mask_ids, (B, T), "mask_ids", "[B,T]", dtype=torch.int64)
        V, E, Cn = 0, 1, 1
        lead = [None, 0, 0, 1, 1, None, None, _ptr(x), _ptr(mask_ids), B, T, H]
    _expect_all(((kernel, (H, 3 * H), "kernel"), (recurrent_kernel, (H, 3 * H), "recurrent_kernel"),
                 (bias, (2, 3 * H), "bias")))
    dien_check_shape(H, T)
    return lead + [_ptr(kernel), _ptr(recurrent_kernel), _ptr(bias), int(padding_index)], (B, T, H, V, E, Cn)


def dien_gru_fwd(kernel, recurrent_kernel, bias, embed=None, series=None, negatives=None, x=None, mask_ids=None,
                 padding_index=0, oob=None, want_output=True, want_final=False):
    """The masked Keras GRU (reset_after=True, gate order z, r, h; the state is carried where the mask id equals
    ``padding_index``) over the looked-up series (``embed`` [V,E], ``series`` ids [B,T,C]) or over dense rows ``x``
    [B,T,H] with ``mask_ids`` [B,T] -> (gru_output [B,T,H] or None, h_final [B,H] or None, aux [1] or None); with
    ``negatives`` [B,T,C] aux is the auxiliary loss summed over the batch.  One launch (plus the slot sum of aux)."""
    args, (B, T, H, V, E, Cn) = _dien_gru_args(embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias,
                                               padding_index)
    if not (want_output or want_final):
        raise ValueError("a DIEN GRU returns gru_output, h_final or both")
    dev = kernel.device
    out = _new((B, T, H), dev, B) if want_output else None
    fin = _new((B, H), dev, B) if want_final else None
    aux = torch.zeros((1,), dtype=torch.float32, device=dev) if negatives is not None else None
    if B > 0:
        tail = (_ptr(out), _ptr(fin), _ptr(aux), _ptr(oob))
        if negatives is not None:
            _call_ws("rec_dien_gru_scratch_bytes", (B, T, H, 0), "rec_dien_gru_fwd_f32", dev, *args, *tail)
        else:
            _call("rec_dien_gru_fwd_f32", *args, *tail, None, 0)
    return out, fin, aux


def dien_gru_bwd(kernel, recurrent_kernel, bias, gru_output, dgru_output=None, dh_final=None, gaux=None, embed=None,
                 series=None, negatives=None, x=None, mask_ids=None, padding_index=0, dx=None, dneg=None):
    """-> (dx [B,T,H]: the IndexedSlices values of the series lookup or the gradient of x, dneg [B,T,H] or None: the
    values of the negative lookup, dkernel, drecurrent_kernel, dbias) from dgru_output [B,T,H], dh_final [B,H] and gaux
    [1], each of which may be None (exact zeros); the gates are computed again from ``gru_output``.  ``dx`` / ``dneg``:
    optional preallocated contiguous destinations (the tail of a shared value buffer)."""
    args, (B, T, H, V, E, Cn) = _dien_gru_args(embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias,
                                               padding_index)
    dev = kernel.device
    _expect(gru_output, (B, T, H), "gru_output", "[B,T,H]")
    _expect(dgru_output, (B, T, H), "dgru_output", "[B,T,H]", optional=True)
    _expect(dh_final, (B, H), "dh_final", "[B,H]", optional=True)
    _expect(gaux, (1,), "gaux", optional=True)
    if dx is None:
        dx = _new((B, T, H), dev, B)
    _expect(dx, (B, T, H), "dx", "[B,T,H]")
    if negatives is not None:
        if dneg is None:
            dneg = _new((B, T, H), dev, B)
        _expect(dneg, (B, T, H), "dneg", "[B,T,H]")
    grads = [_new_like(t, B) for t in (kernel, recurrent_kernel, bias)]
    if B > 0:
        _call_ws("rec_dien_gru_scratch_bytes", (B, T, H, 1), "rec_dien_gru_bwd_f32", dev, *args, _ptr(gru_output),
                 _ptr(dgru_output), _ptr(dh_final), _ptr(gaux), _ptr(dx), _ptr(dneg), *_ptrs(grads))
    return (dx, dneg if negatives is not None else None) + tuple(grads)


def _dien_augru_args(gru_output, q, mask_ids, mode, Wx, Uh, bx, padding_index, mask_valid):
    if _f32(gru_output, "gru_output").dim() != 3:
        raise ValueError("gru_output must be [B,T,H], got %s" % (tuple(gru_output.shape),))
    B, T, H = gru_output.shape
    if mode not in (DIEN_AUGRU, DIEN_AGRU):
        raise ValueError("the evolution's mode must be DIEN_AUGRU or DIEN_AGRU, got %r" % (mode,))
    ng = 3 if mode == DIEN_AUGRU else 2
    _req(mask_ids, torch.int64, "mask_ids")
    if mask_ids.dim() not in (2, 3) or tuple(mask_ids.shape[:2]) != (B, T):
        raise ValueError("mask_ids must be [B,T] or the series ids [B,T,C], got %s" % (tuple(mask_ids.shape),))
    stride = mask_ids.shape[2] if mask_ids.dim() == 3 else 1
    _expect_all(((q, (B, H), "q"), (Wx, (H, ng * H), "Wx"), (Uh, (H, ng * H), "Uh"), (bx, (ng * H,), "bx")))
    dien_check_shape(H, T, mode)
    return [_ptr(gru_output), _ptr(q), _ptr(mask_ids), stride, B, T, H, mode, _ptr(Wx), _ptr(Uh), _ptr(bx),
            int(padding_index), int(bool(mask_valid))], (B, T, H)


def dien_augru_fwd(gru_output, q, mask_ids, mode, Wx, Uh, bx, padding_index=0, mask_valid=0, save=True):
    """DienActivationLayer's scores and the AGRU / AUGRU over them in one launch: gru_output [B,T,H], q = X_item W^T
    [B,H], the mask ids ([B,T], or the series ids [B,T,C] whose first feature decides), the packed cell weights Wx, Uh
    [H, ng H] and bx [ng H] (AUGRU [z | r | h], AGRU [r | h]) -> (scores [B,T], states [B,T,H] or None, h_final [B,H]).
    ``mask_valid`` = 0 scores the PADDED positions (the reference), 1 the valid ones."""
    args, (B, T, H) = _dien_augru_args(gru_output, q, mask_ids, mode, Wx, Uh, bx, padding_index, mask_valid)
    dev = gru_output.device
    scores, fin = _new((B, T), dev, B), _new((B, H), dev, B)
    states = _new((B, T, H), dev, B) if save else None
    if B > 0:
        _call("rec_dien_augru_fwd_f32", *args, _ptr(scores), _ptr(states), _ptr(fin))
    return scores, states, fin


def dien_augru_bwd(gru_output, q, mask_ids, mode, Wx, Uh, bx, scores, states, dh_final, padding_index=0, mask_valid=0):
    """-> (dgru_output [B,T,H], dq [B,H], dWx, dUh, dbx) from dh_final [B,H] and the forward's scores and states"""
    args, (B, T, H) = _dien_augru_args(gru_output, q, mask_ids, mode, Wx, Uh, bx, padding_index, mask_valid)
    _expect_all(((scores, (B, T), "scores"), (states, (B, T, H), "states"), (dh_final, (B, H), "dh_final")))
    dev = gru_output.device
    dg, dq = _new((B, T, H), dev, B), _new((B, H), dev, B)
    grads = [_new_like(t, B) for t in (Wx, Uh, bx)]
    if B > 0:
        _call_ws("rec_dien_augru_scratch_bytes", (B, T, H, mode), "rec_dien_augru_bwd_f32", dev, *args, _ptr(scores),
                 _ptr(states), _ptr(dh_final), _ptr(dg), _ptr(dq), *_ptrs(grads))
    return (dg, dq) + tuple(grads)


# ---------------------------------------------------------------------------------------------------
# SIM (7.SIM/CustomLayers.py:130-282; csrc/sim.hip): the soft search fused with the GSU pooling, and the one-query
# multi-head attention of the exact search unit.  The limits are the header's and show through the size queries.
# ---------------------------------------------------------------------------------------------------
# the attention's widths and heads; K is the searches' as well, and a search alone covers a key width of _SEARCH_MAX_D
SIM_MAX_D, SIM_MAX_K, SIM_MAX_H = LIMITS["REC_ESU_MAX_D"], LIMITS["REC_SEARCH_MAX_K"], LIMITS["REC_ESU_MAX_H"]
_SEARCH_MAX_D = LIMITS["REC_SEARCH_MAX_D"]          # SIM, ETA and SDIM alike, and so is the launch cap of their kernels
_SEARCH_LDS_CAP = LIMITS["REC_SEARCH_LDS_CAP"]


def sim_search_lds_bytes(T, C, D, K=1):
    """LDS of one example of the search (include/mi355rec.h)"""
    return 4 * (T * C + 4 * D + T + 16)


def esu_attn_lds_bytes(K, D, H, dk):
    """LDS of a tile of 32 examples of the attention (include/mi355rec.h)"""
    return 132 * (_even(max(H * dk, H * D, D)) + 2 + 2 * H * K + H)


def sim_check_shape(D, T=None, K=None, H=None, dk=None, C=1):
    """ValueError for sizes that describe no SIM body, NotImplementedError naming the limit for shapes the kernels do not
    cover (the ABI would return -2): the key width D = E C, the series length T, the K selected positions, and -- for the
    attention -- the heads H and their width dk (None: dk = D, the reference's)."""
    given = [v for v in (D, T, K, H, dk, C) if v is not None]
    if min(given) < 1:
        raise ValueError("every size of a SIM body must be positive, got D=%r, T=%r, K=%r, H=%r, dk=%r"
                         % (D, T, K, H, dk))
    if D > _SEARCH_MAX_D:
        raise NotImplementedError("the SIM search covers a key width embedding_dims * series features <= %d; got %d"
                                  % (_SEARCH_MAX_D, D))
    if K is not None and K > SIM_MAX_K:
        raise NotImplementedError("SIM kernels cover k <= %d selected positions; got %d" % (SIM_MAX_K, K))
    if T is not None and sim_search_lds_bytes(T, C, D) > _SEARCH_LDS_CAP:
        raise NotImplementedError("the SIM search holds one example's ids and scores in LDS: 4 (T C + 4 D + T + 16) <= "
                                  "%d bytes; got %d at T=%d, C=%d, D=%d"
                                  % (_SEARCH_LDS_CAP, sim_search_lds_bytes(T, C, D), T, C, D))
    if H is not None:
        dk = D if dk is None else dk
        if D > SIM_MAX_D or dk > SIM_MAX_D or H > SIM_MAX_H or D % 2 or dk % 2:
            raise NotImplementedError("the ESU attention covers even widths D, key_dim <= %d and num_heads <= %d; got "
                                      "D=%d, key_dim=%d, num_heads=%d" % (SIM_MAX_D, SIM_MAX_H, D, dk, H))
        if K is not None:
            _lds_fit(esu_attn_lds_bytes(K, D, H, dk), "the ESU attention holds a tile of 32 examples",
                     "33 (max(H dk, H D) + 2 + 2 H K + H)", "K=%d, D=%d, H=%d, key_dim=%d" % (K, D, H, dk))


def _search_head(embed, series, q, what, K=None):
    """What every entry point that searches a series for one query starts with: _series_head, q is [B, C E] and, where
    K positions are selected, 1 <= K <= T.  -> the leading ABI arguments (.., q, its stride) and (V, E, B, T, C, D)."""
    head, (V, E, B, T, Cn) = _series_head(embed, series, what)
    D = Cn * E
    _expect(q, (B, D), "q", "[B, C E]")
    if K is not None and not 1 <= K <= T:
        raise ValueError("%s selects 1 <= K <= T positions, got K=%d at T=%d" % (what, K, T))
    return head + [_ptr(q), D], (V, E, B, T, Cn, D)


def ip_attn_fwd(embed, series, q, padding_index, oob=None):
    """series [B,T,C] int64, q [B,C*E] -> masked scores [B,T], pooled [B,C*E]  (7.SIM/CustomLayers.py:88-96).  A shape
    past the kernel's limits is the library's REC_E_ARG, a ValueError."""
    head, (V, E, B, T, Cn, D) = _search_head(embed, series, q, "the GSU attention")
    scores, pooled = _new((B, T), embed.device), _new((B, D), embed.device)
    _call("rec_ip_attn_fwd_f32", *head, int(padding_index), _ptr(scores), _ptr(pooled), D, _ptr(oob))
    return scores, pooled


def ip_attn_bwd(embed, series, q, padding_index, scores, gpooled, gkeys=None):
    """-> (gkeys [B,T,D]: the IndexedSlices values of the series lookup, gq [B,D]) from gpooled [B,D].  ``gkeys``:
    optional preallocated contiguous destination."""
    head, (V, E, B, T, Cn, D) = _search_head(embed, series, q, "the GSU attention")
    _expect_all(((scores, (B, T), "scores"), (gpooled, (B, D), "gpooled")))
    if gkeys is None:
        gkeys = _new((B, T, D), embed.device)
    _expect(gkeys, (B, T, D), "gkeys", "[B,T,D]")
    gq = _new((B, D), embed.device)
    _call("rec_ip_attn_bwd_f32", *head, int(padding_index), _ptr(scores), _ptr(gpooled), D, _ptr(gkeys), _ptr(gq))
    return gkeys, gq


def _sim_search_args(embed, series, q, padding_index, K):
    head, dims = _search_head(embed, series, q, "the SIM search", K)
    sim_check_shape(dims[5], dims[3], K, C=dims[4])
    return head + [int(padding_index), int(K)], dims


def sim_search_fwd(embed, series, q, padding_index, K, oob=None):
    """series [B,T,C] int64, q [B, C E] -> (scores [B,T], pooled [B,D], chosen int32 [B,K], sel [B,K,D], sel_valid int32
    [B,K]): rec_ip_attn's scores and pooling, the K best positions by <q, k_t> (padded steps rank as -inf, ties go to the
    lower index) and their rows  (7.SIM/CustomLayers.py:88-96, 236-260).  One launch."""
    args, (V, E, B, T, Cn, D) = _sim_search_args(embed, series, q, padding_index, K)
    dev = embed.device
    scores, pooled, sel = _new((B, T), dev, B), _new((B, D), dev, B), _new((B, K, D), dev, B)
    chosen, sel_valid = _new((B, K), dev, B, torch.int32), _new((B, K), dev, B, torch.int32)
    if B > 0:
        _call("rec_sim_search_fwd_f32", *args, _ptr(scores), _ptr(pooled), D, _ptr(chosen), _ptr(sel), _ptr(sel_valid),
              _ptr(oob))
    return scores, pooled, chosen, sel, sel_valid


def sim_search_bwd(embed, series, q, padding_index, scores, gpooled, chosen, gsel=None, gkeys=None):
    """-> (gkeys [B,T,D]: the IndexedSlices values of the series lookup, gq [B,D]) from gpooled [B,D] and gsel [B,K,D]
    (None: nothing arrives through the selected rows).  ``gkeys``: optional preallocated contiguous destination."""
    if _req(chosen, torch.int32, "chosen").dim() != 2:
        raise ValueError("chosen must be [B,K], got %s" % (tuple(chosen.shape),))
    K = chosen.shape[1]
    args, (V, E, B, T, Cn, D) = _sim_search_args(embed, series, q, padding_index, K)
    _expect(chosen, (B, K), "chosen", "[B,K]", dtype=torch.int32)
    _expect_all(((scores, (B, T), "scores"), (gpooled, (B, D), "gpooled")))
    _expect(gsel, (B, K, D), "gsel", "[B,K,D]", optional=True)
    dev = embed.device
    if gkeys is None:
        gkeys = _new((B, T, D), dev, B)
    _expect(gkeys, (B, T, D), "gkeys", "[B,T,D]")
    gq = _new((B, D), dev, B)
    if B > 0:
        _call("rec_sim_search_bwd_f32", *args, _ptr(scores), _ptr(gpooled), D, _ptr(chosen), _ptr(gsel), _ptr(gkeys),
              _ptr(gq))
    return gkeys, gq


_ESU_WEIGHTS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wo", "bo")


def _esu_attn_args(q, x, mask, weights):
    """``weights``: (Wq, bq, Wk, bk, Wv, bv, Wo, bo), Keras' kernels [D,H,dk] / [H,dk,D] and biases [H,dk] / [D]"""
    if _f32(x, "x").dim() != 3:
        raise ValueError("x must be [B,K,D], got %s" % (tuple(x.shape),))
    B, K, D = x.shape
    if len(weights) != 8 or _f32(weights[0], "Wq").dim() != 3 or weights[0].shape[0] != D:
        raise ValueError("the ESU attention takes (Wq, bq, Wk, bk, Wv, bv, Wo, bo) with Wq [D,H,dk]")
    H, dk = weights[0].shape[1:]
    _expect(q, (B, D), "q", "[B,D]")
    _expect(mask, (B, K), "mask", "[B,K]", dtype=torch.int32)
    shapes = ((D, H, dk), (H, dk), (D, H, dk), (H, dk), (D, H, dk), (H, dk), (H, dk, D), (D,))
    for t, shape, name in zip(weights, shapes, _ESU_WEIGHTS):
        _expect(t, shape, name)
    sim_check_shape(D, None, K, H, dk)
    return [_ptr(q), D, _ptr(x), _ptr(mask), B, K, D, H, dk], (B, K, D, H, dk)


def esu_attn_fwd(q, x, mask, weights, want_probs=False):
    """Keras MultiHeadAttention with one query: q [B,D], x [B,K,D] (keys and values), mask int32 [B,K] (non-zero =
    attend, applied additively as -1e9 in fp32) -> (out [B,D], probs [B,H,K] or None).  One launch."""
    args, (B, K, D, H, dk) = _esu_attn_args(q, x, mask, weights)
    dev = x.device
    out = _new((B, D), dev, B)
    probs = _new((B, H, K), dev, B) if want_probs else None
    if B > 0:
        _call_ws("rec_esu_attn_scratch_bytes", (B, K, D, H, dk), "rec_esu_attn_fwd_f32", dev, *args, *_ptrs(weights),
                 _ptr(out), _ptr(probs))
    return out, probs


def esu_attn_bwd(q, x, mask, weights, gout):
    """-> (gq [B,D], gx [B,K,D], dWq, dbq, dWk, dbk, dWv, dbv, dWo, dbo) from gout [B,D]; the forward's stages are
    computed again"""
    args, (B, K, D, H, dk) = _esu_attn_args(q, x, mask, weights)
    _expect_all(((gout, (B, D), "gout"),))
    dev = x.device
    gq, gx = _new((B, D), dev, B), _new((B, K, D), dev, B)
    grads = [_new_like(t, B) for t in weights]
    if B > 0:
        _call_ws("rec_esu_attn_scratch_bytes", (B, K, D, H, dk), "rec_esu_attn_bwd_f32", dev, *args,
                 *_ptrs(weights[:7]), _ptr(gout), D, _ptr(gq), _ptr(gx), *_ptrs(grads))
    return (gq, gx) + tuple(grads)


# ---------------------------------------------------------------------------------------------------
# ETA (7.SIM/CustomLayers.py:518-626; csrc/eta.hip): the SimHash search of the long series.  The limits are the
# header's and show through its size query.
# ---------------------------------------------------------------------------------------------------
ETA_MAX_M = LIMITS["REC_ETA_MAX_M"]


def eta_search_lds_bytes(T, D, m):
    """LDS of one example of the search (include/mi355rec.h): the projection in 16 or 32 columns, the ranks, the chosen"""
    return 4 * (D * (16 if m <= 16 else 32) + T + 16)


def eta_check_shape(D, T=None, K=None, m=None, C=None):
    """ValueError for sizes that describe no ETA search, NotImplementedError naming the limit for shapes the kernel does
    not cover (the ABI would return -2): the key width D = E C, the series length T, the K selected positions, the m
    hash bits and the C id columns of a step."""
    given = [v for v in (D, T, K, m, C) if v is not None]
    if min(given) < 1:
        raise ValueError("every size of an ETA search must be positive, got D=%r, T=%r, K=%r, m=%r, C=%r"
                         % (D, T, K, m, C))
    if C is not None and D % C:
        raise ValueError("the key width D = embedding_dims * series features; got D=%d with C=%d" % (D, C))
    if D > _SEARCH_MAX_D:
        raise NotImplementedError("the ETA search covers a key width embedding_dims * series features <= %d; got %d"
                                  % (_SEARCH_MAX_D, D))
    if K is not None and K > SIM_MAX_K:
        raise NotImplementedError("the ETA search covers lsh_topk <= %d selected positions; got %d" % (SIM_MAX_K, K))
    if m is not None and m > ETA_MAX_M:
        raise NotImplementedError("the ETA search covers lsh_dim <= %d hash bits; got %d" % (ETA_MAX_M, m))
    if T is not None and eta_search_lds_bytes(T, D, 1 if m is None else m) > _SEARCH_LDS_CAP:
        m = 1 if m is None else m
        raise NotImplementedError("the ETA search holds the projection and one example's ranks in LDS: 4 (D MC + T + 16) "
                                  "<= %d bytes with MC = 16 or 32 columns; got %d at T=%d, D=%d, lsh_dim=%d"
                                  % (_SEARCH_LDS_CAP, eta_search_lds_bytes(T, D, m), T, D, m))


def eta_search_fwd(embed, series, q, Hm, padding_index, K, oob=None, want_scores=True):
    """series [B,T,C] int64, q [B, C E], Hm [C E, m] -> (scores int32 [B,T] or None, chosen int32 [B,K], sel [B,K,D],
    sel_valid int32 [B,K], sel_ids int64 [B,K,C]): the Hamming similarity of the SimHash codes of every step and of q,
    the K best positions by it (padded steps rank as -inf, ties go to the lower index), their rows and their ids
    (7.SIM/CustomLayers.py:556-571).  One launch."""
    head, (V, E, B, T, Cn, D) = _search_head(embed, series, q, "the ETA search", K)
    if _f32(Hm, "Hm").dim() != 2 or Hm.shape[0] != D:
        raise ValueError("Hm must be [C E, m] = [%d, m], got %s" % (D, tuple(Hm.shape)))
    m = Hm.shape[1]
    eta_check_shape(D, T, K, m, Cn)
    dev = embed.device
    scores = _new((B, T), dev, B, torch.int32) if want_scores else None
    chosen, sel_valid = _new((B, K), dev, B, torch.int32), _new((B, K), dev, B, torch.int32)
    sel, sel_ids = _new((B, K, D), dev, B), _new((B, K, Cn), dev, B, torch.int64)
    if B > 0:
        _call("rec_eta_search_fwd_f32", *head, _ptr(Hm), m, int(padding_index), int(K), _ptr(scores),
              _ptr(chosen), _ptr(sel), _ptr(sel_valid), _ptr(sel_ids), _ptr(oob))
    return scores, chosen, sel, sel_valid, sel_ids


# ---------------------------------------------------------------------------------------------------
# SDIM (8.DMR/CustomLayers.py:816-841; csrc/sdim.hip): the hash-bucket interest of the long series.  The limits are the
# header's and show through its size query.
# ---------------------------------------------------------------------------------------------------
SDIM_MAX_BITS, SDIM_MAX_S, SDIM_MAX_D = LIMITS["REC_SDIM_MAX_BITS"], LIMITS["REC_SDIM_MAX_S"], _SEARCH_MAX_D
SDIM_MODES = {k: ENUMS["REC_SDIM_MODE_" + k.upper()] for k in ("reference", "valid")}


def sdim_lds_bytes(T, D, G, m):
    """LDS of one example of the forward (include/mi355rec.h): the projection in 16 or 32 columns, the steps' codes, the
    padding bit map, the candidates' codes and four waves' lists of matching steps (16-bit entries)"""
    return 4 * (D * (16 if G * m <= 16 else 32) + T + 2 * ((T + 63) // 64) + 16 + 2 * (T + T % 2))


def sdim_check_shape(D, T=None, S=None, G=None, m=None, C=None):
    """ValueError for sizes that describe no SDIM interest, NotImplementedError naming the limit for shapes the kernels
    do not cover (the ABI would return -2): the key width D = E C, the series length T, the S candidates, the G hash
    groups of m bits and the C id columns of a step."""
    given = [v for v in (D, T, S, G, m, C) if v is not None]
    if min(given) < 1:
        raise ValueError("every size of an SDIM interest must be positive, got D=%r, T=%r, S=%r, G=%r, m=%r, C=%r"
                         % (D, T, S, G, m, C))
    if C is not None and D % C:
        raise ValueError("the key width D = embedding_dims * series features; got D=%d with C=%d" % (D, C))
    if D > SDIM_MAX_D:
        raise NotImplementedError("the SDIM interest covers a key width embedding_dims * series features <= %d; got %d"
                                  % (SDIM_MAX_D, D))
    if S is not None and S > SDIM_MAX_S:
        raise NotImplementedError("the SDIM interest covers candidates <= %d per example; got %d" % (SDIM_MAX_S, S))
    bits = (1 if G is None else G) * (1 if m is None else m)
    if bits > SDIM_MAX_BITS:
        raise NotImplementedError("the SDIM interest covers lsh_group_num * lsh_group_length <= %d hash bits; got %d"
                                  % (SDIM_MAX_BITS, bits))
    if T is not None:
        G1 = 1 if G is None else G
        need = sdim_lds_bytes(T, D, G1, bits // G1)
        if need > _SEARCH_LDS_CAP:      # need > 4 T: this also keeps T inside the kernel's 16-bit list entries
            raise NotImplementedError("the SDIM interest holds the projection and one example's codes in LDS: 4 (D MC + T "
                                      "+ 2 ceil(T / 64) + 16 + 2 (T + T mod 2)) <= %d bytes with MC = 16 or 32 columns; got %d at "
                                      "T=%d, D=%d, hash bits=%d" % (_SEARCH_LDS_CAP, need, T, D, bits))


def _sdim_mode(mask_mode):
    if mask_mode not in SDIM_MODES:
        raise ValueError("mask_mode must be 'reference' or 'valid', got %r" % (mask_mode,))
    return SDIM_MODES[mask_mode]


def sdim_interest_fwd(embed, series, q, Hm, padding_index, mask_mode="reference", oob=None):
    """series [B,T,C] int64, q [B,S,C E] (the candidates' rows; a view with unit inner stride and any row stride), Hm
    [C E, G, m] -> (out [B,S,D], codes int32 [B,T], qcodes int32 [B,S], cnt int32 [B,S,G]): the mean, per hash group, of
    the steps whose group code equals the candidate's, averaged over the groups (8.DMR/CustomLayers.py:816-841), and
    what the backward needs.  One launch."""
    head, (V, E, B, T, Cn) = _series_head(embed, series, "the SDIM interest")
    D = Cn * E
    if not isinstance(q, torch.Tensor) or not q.is_cuda:
        raise RuntimeError("q must be a tensor on the MI355X: the HIP path has no CPU fallback")
    if q.dtype != torch.float32 or q.dim() != 3 or q.shape[0] != B or q.shape[2] != D:
        raise ValueError("q must be fp32 [B, S, C E] = [%d, S, %d], got %s %s" % (B, D, q.dtype, tuple(q.shape)))
    S = q.shape[1]
    # row (b, s) starts at (b S + s) ld_q: a size-1 axis has no stride of its own
    ld_q = q.stride(1) if S > 1 else (q.stride(0) if B > 1 else D)
    if q.numel() and (q.stride(2) != 1 or ld_q < D or (S > 1 and B > 1 and q.stride(0) != S * ld_q)):
        raise ValueError("q must have unit inner stride and one row stride >= C E over [B, S], got strides %s"
                         % (tuple(q.stride()),))
    if _f32(Hm, "Hm").dim() != 3 or Hm.shape[0] != D:
        raise ValueError("Hm must be [C E, G, m] = [%d, G, m], got %s" % (D, tuple(Hm.shape)))
    G, m = Hm.shape[1:]
    mode = _sdim_mode(mask_mode)
    sdim_check_shape(D, T, S, G, m, Cn)
    dev = embed.device
    out = _new((B, S, D), dev, B)
    codes, qcodes = _new((B, T), dev, B, torch.int32), _new((B, S), dev, B, torch.int32)
    cnt = _new((B, S, G), dev, B, torch.int32)
    if B > 0:
        _call("rec_sdim_interest_fwd_f32", *head, _ptr(q), ld_q, S, _ptr(Hm), G, m, int(padding_index), mode, _ptr(out),
              _ptr(codes), _ptr(qcodes), _ptr(cnt), _ptr(oob))
    return out, codes, qcodes, cnt


def sdim_interest_bwd(series, E, m, padding_index, codes, qcodes, cnt, gout, mask_mode="reference", gkeys=None):
    """-> gkeys [B,T,C E]: the IndexedSlices values of the series lookup, from gout [B,S,D] and the forward's codes,
    qcodes and cnt; ``E``: the table's width, ``m``: the bits of a hash group.  ``gkeys``: optional preallocated
    contiguous destination."""
    if _i64(series, "series").dim() != 3 or _req(cnt, torch.int32, "cnt").dim() != 3:
        raise ValueError("series must be [B,T,C] and cnt [B,S,G]")
    (B, T, Cn), (S, G) = series.shape, cnt.shape[1:]
    D = Cn * int(E)
    mode = _sdim_mode(mask_mode)
    sdim_check_shape(D, T, S, G, int(m), Cn)
    _expect(codes, (B, T), "codes", "[B,T]", dtype=torch.int32)
    _expect(qcodes, (B, S), "qcodes", "[B,S]", dtype=torch.int32)
    _expect(cnt, (B, S, G), "cnt", "[B,S,G]", dtype=torch.int32)
    _expect_all(((gout, (B, S, D), "gout"),))
    if gkeys is None:
        gkeys = _new((B, T, D), series.device, B)
    _expect(gkeys, (B, T, D), "gkeys", "[B,T,D]")
    if B > 0:
        _call("rec_sdim_interest_bwd_f32", _ptr(series), int(E), Cn, B, T, G, int(m), S, int(padding_index), mode,
              _ptr(codes), _ptr(qcodes), _ptr(cnt), _ptr(gout), D, _ptr(gkeys))
    return gkeys
