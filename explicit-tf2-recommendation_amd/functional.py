"""torch.autograd.Function wrappers: forward and backward of each op are HIP kernels called through the C ABI
(ops.py).  Embedding tables receive their gradient the way TF's GradientTape delivers it -- as an
IndexedSlices-like sparse gradient -- here already de-duplicated (sorted unique ids + summed rows) and wrapped
as an uncoalesced torch sparse COO tensor whose padded tail points at a valid id with zero rows, so no
host synchronisation is needed to learn the unique count.
"""
import math

import torch

from . import ops


class SparseRowGrad:
    """(uniq_ids [cap], rows [cap,E], n_uniq [1]) as produced by ops.DedupPlan; what the fused optimizers eat."""

    def __init__(self, uniq_ids, rows, n_uniq, shape):
        self.uniq_ids, self.rows, self.n_uniq, self.shape = uniq_ids, rows, n_uniq, shape

    def to_sparse(self):
        return torch.sparse_coo_tensor(self.uniq_ids[: self.rows.shape[0]].unsqueeze(0), self.rows, self.shape)


def _sparse_grad(plan, vals, E, shape, row_div=1, wide=False):
    rows = plan.segment_sum(vals, E, row_div, wide)
    return SparseRowGrad(plan.uniq_ids, rows, plan.n_uniq, shape).to_sparse()


class GradSink:
    """One de-duplication per table per step for a layer with several lookups into the SAME table (DIN, SIM GSU:
    profile / target-item rows through Gather, the behaviour series through the attention kernel).  The attention's
    backward -- which autograd runs first, its query comes out of the Gather -- leaves its ids and its IndexedSlices
    values here, written behind ``n_head`` free rows of one shared buffer; the Gather's backward then fills the head
    with its own values and builds ONE plan over both id lists.  Without it torch concatenates the two sparse gradients
    (a 157-MB copy at DIN config E) and each lookup sorts on its own."""

    def __init__(self, n_head, n_tail=0):
        self.n_head = int(n_head)
        self.n_tail = int(n_tail)                            # zero rows behind the series' values (sharded.ShardedEmbedding)
        self.ids = None
        self.buf = None

    def new_buf(self, n_series, E, device):
        buf = torch.empty((self.n_head + n_series + self.n_tail, E), dtype=torch.float32, device=device)
        if self.n_tail:
            buf[self.n_head + n_series:].zero_()
        return buf

    def take(self):
        ids, buf = self.ids, self.buf
        self.ids = self.buf = None
        return ids, buf


def _sink_dsts(sink, E, device, *id_tensors):
    """First half of a fused lookup's gradient hand-off: where its backward writes the IndexedSlices values of each id
    tensor ([B,n,C], or None for a lookup that is absent) -> (buf, a [B,n,C E] view of it per tensor), the views one
    after the other behind the sink's head rows; without a sink (None, Nones) and the kernel wrapper allocates."""
    if sink is None:
        return None, [None] * len(id_tensors)
    buf = sink.new_buf(sum(t.numel() for t in id_tensors if t is not None), E, device)
    dsts, at = [], sink.n_head
    for t in id_tensors:
        dsts.append(None if t is None else buf[at:at + t.numel()].view(t.shape[0], t.shape[1], t.shape[2] * E))
        at += 0 if t is None else t.numel()
    return buf, dsts


def _series_grad(ctx, ids, vals, V, E, sink=None, buf=None):
    """Second half: the table's gradient of a fused series / item lookup.  ``ids`` and ``vals`` are one tensor each or
    matching sequences (series first, then negatives; None entries are absent lookups), laid end to end in that order:
    it defines the de-duplication plan.  With a sink the ids and ``buf`` (which holds the values) are left there for the
    Gather's backward and None is returned; else sparse COO with de-duplicated rows, or None when the table needs no
    gradient."""
    if torch.is_tensor(ids):
        ids, vals = (ids,), (vals,)
    ids = [t for t in ids if t is not None]
    ids = ids[0] if len(ids) == 1 else torch.cat([t.reshape(-1) for t in ids])
    if sink is not None:
        sink.ids, sink.buf = ids, buf
        return None
    if not ctx.needs_input_grad[0]:
        return None
    vals = [v.reshape(-1, E) for v in vals if v is not None]
    return _sparse_grad(ops.DedupPlan(ids, V), vals[0] if len(vals) == 1 else torch.cat(vals), E, (V, E))


class Gather(torch.autograd.Function):
    """Embedding(V,E)(X): K2.  Backward: sparse row gradient (K4)."""

    @staticmethod
    def forward(ctx, table, X, oob, sink=None):
        out = ops.emb_gather(table, X, oob)
        ctx.save_for_backward(X)
        ctx.shape = tuple(table.shape)
        ctx.sink = sink
        return out

    @staticmethod
    def backward(ctx, g):
        (X,) = ctx.saved_tensors
        V, E = ctx.shape
        g = g.contiguous().reshape(-1, E)
        ids, buf = ctx.sink.take() if ctx.sink is not None else (None, None)
        if buf is not None:                                  # the series lookups of the same table ride along
            buf[: g.shape[0]].copy_(g)
            plan = ops.DedupPlan(torch.cat([X.reshape(-1), ids.reshape(-1)]), V)
            return _sparse_grad(plan, buf, E, (V, E)), None, None, None
        plan = ops.DedupPlan(X, V)
        return _sparse_grad(plan, g, E, (V, E)), None, None, None


class UsedRowsL2(torch.autograd.Function):
    """factor * tf.nn.l2_loss(tf.gather(table, tf.unique(ids).y))  (5.DIN/ModelManager.py:176-190): every row the
    batch touched is penalised ONCE, however often it was looked up.  Backward: sparse rows factor * table[u]."""

    @staticmethod
    def forward(ctx, table, ids, factor):
        V, E = table.shape
        plan = ops.DedupPlan(ids.reshape(-1).contiguous(), V)
        loss, rows = ops.l2_used_rows(table, plan, factor)
        ctx.save_for_backward(plan.uniq_ids, rows, plan.n_uniq)
        ctx.shape = (V, E)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        uniq_ids, rows, n_uniq = ctx.saved_tensors
        return SparseRowGrad(uniq_ids, rows * g, n_uniq, ctx.shape).to_sparse(), None, None


class EmbFM(torch.autograd.Function):
    """Fused w(X), embed(X), FM first + second order (K2+K3).  Returns z [B] and, for DeepFM, the gathered
    rows [B,F,E] that feed the DNN part.  Backward builds the IndexedSlices values (FM term + whatever came
    back through the rows) and de-duplicates once for both tables."""

    @staticmethod
    def forward(ctx, embed, w, bias, X, want_rows, oob):
        z, _, rows, S = ops.emb_fm_fwd(embed, w, bias, X, want_rows=want_rows, oob=oob)
        ctx.save_for_backward(embed, X, S, rows if want_rows else None)
        if not want_rows:
            rows = torch.empty(0, dtype=torch.float32, device=embed.device)
            ctx.mark_non_differentiable(rows)
        return z, rows

    @staticmethod
    def backward(ctx, gz, grows):
        embed, X, S, rows = ctx.saved_tensors
        V, E = embed.shape
        B, F = X.shape
        if gz is None:
            gz = torch.zeros(B, dtype=torch.float32, device=embed.device)
        gz = gz.contiguous()
        extra = grows.contiguous() if (grows is not None and rows is not None) else None
        vals = ops.emb_fm_bwd_vals(embed, X, gz, S, rows, extra)
        plan = ops.DedupPlan(X, V)
        g_embed = _sparse_grad(plan, vals, E, (V, E))
        g_w = _sparse_grad(plan, gz.reshape(B, 1), 1, (V, 1), row_div=F)
        g_bias = ops.colsum(gz.reshape(B, 1))
        return g_embed, g_w, g_bias, None, None, None


class LinearAct(torch.autograd.Function):
    """act(x @ K + b): MatMul + BiasAdd + activation of MLPLayer / Dense (K5) on the fp32 matrix cores."""

    @staticmethod
    def forward(ctx, x, K, b, act):
        x = x.contiguous()
        if b is not None:
            y = ops.gemm(x, K, epi=ops.EPI_OF_ACT[act], bias=b)
        else:
            y = ops.gemm(x, K)
            if act != ops.ACT_NONE:
                raise NotImplementedError("activation without bias")
        ctx.save_for_backward(x, K, y)
        ctx.act = act
        ctx.has_bias = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, K, y = ctx.saved_tensors
        gy = gy.contiguous()
        dpre = ops.act_bwd(ctx.act, y, gy) if ctx.act != ops.ACT_NONE else gy
        M, Kd = x.shape
        N = K.shape[1]
        gx = ops.gemm(dpre, K, transB=True) if ctx.needs_input_grad[0] else None
        gK = ops.gemm(x, dpre, transA=True, split_k=ops.split_k_for(M, Kd, N, True, False))
        gb = ops.colsum(dpre) if ctx.has_bias else None
        return gx, gK, gb, None


class CrossVec(torch.autograd.Function):
    """CrossLayer (3.DCN/CustomLayers.py:195-203).  w, b: [L, D]."""

    @staticmethod
    def forward(ctx, x0, w, b):
        x0 = x0.contiguous()
        y, xs = ops.crossnet_vec_fwd(x0, w.contiguous(), b.contiguous(), save=True)
        ctx.save_for_backward(x0, w, xs)
        return y

    @staticmethod
    def backward(ctx, gy):
        x0, w, xs = ctx.saved_tensors
        gx0, dw, db = ops.crossnet_vec_bwd(x0, w.contiguous(), xs, gy.contiguous())
        return gx0, dw, db


class CrossMat(torch.autograd.Function):
    """MatrixCrossLayer (3.DCN/CustomLayers.py:297-305): x_{l+1} = x0 * (x_l W_l^T + b_l) + x_l, one MFMA GEMM
    per layer with the elementwise part fused into its epilogue.  W: [L, D, D], b: [L, D]."""

    @staticmethod
    def forward(ctx, x0, W, b):
        x0 = x0.contiguous()
        L = W.shape[0]
        xs, us = [x0], []
        for l in range(L):
            u = torch.empty_like(x0)                     # U_l = x_l W_l^T + b_l, written by the GEMM epilogue
            xs.append(ops.gemm(xs[-1], W[l], transB=True, epi=ops.EPI_CROSS, bias=b[l], e0=x0, e1=xs[-1], aux=u))
            us.append(u)
        ctx.L = L
        ctx.save_for_backward(x0, W, b, *xs[:-1], *us)
        return xs[-1]

    @staticmethod
    def backward(ctx, gy):
        x0, W, b = ctx.saved_tensors[:3]
        L = ctx.L
        xs = ctx.saved_tensors[3:3 + L]
        us = ctx.saved_tensors[3 + L:]
        B, D = x0.shape
        g = gy.contiguous()
        gx0 = torch.empty_like(x0)
        dW = torch.empty_like(W)
        db = torch.empty_like(b)
        for l in range(L - 1, -1, -1):
            xl = xs[l]
            u = us[l]
            h = ops.crossnet_mat_bwd_elem(g, x0, u, gx0, accumulate=(l != L - 1))   # H = G(.)X0 ; dX0 += G(.)U
            ops.gemm(h, xl, transA=True, split_k=ops.split_k_for(B, D, D, True, False), out=dW[l])
            ops.colsum(h, out=db[l])
            g = ops.gemm(h, W[l], epi=ops.EPI_ADD, e1=g)                             # dX_l = G + H W
        if L == 0:
            return g, dW, db
        ops.axpby(1.0, g, 1.0, gx0)                                                  # x_0 is also layer 0's input
        return gx0, dW, db


class Cosine(torch.autograd.Function):
    """(1 + keras cosine_similarity(u, i))/2 = (1 - cos)/2  (2.FM/CustomLayers.py:233-234)."""

    @staticmethod
    def forward(ctx, u, i):
        u, i = u.contiguous(), i.contiguous()
        ctx.save_for_backward(u, i)
        return ops.cosine_fwd(u, i)

    @staticmethod
    def backward(ctx, g):
        u, i = ctx.saved_tensors
        return ops.cosine_bwd(u, i, g.contiguous())


class KerasBCE(torch.autograd.Function):
    """reduce_sum(BinaryCrossentropy()(y, p)) on probabilities (2.FM/ModelManager.py:100,175)."""

    @staticmethod
    def forward(ctx, p, y):
        loss, dp, _ = ops.bce_fwd_bwd(y, p.contiguous(), want_dp=True)
        ctx.save_for_backward(dp)
        ctx.shape = p.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return (dp * g).reshape(ctx.shape), None


class Sigmoid(torch.autograd.Function):
    """tf.nn.sigmoid head (2.FM/CustomLayers.py:155,305)."""

    @staticmethod
    def forward(ctx, z, z2=None):
        """sigmoid(z + z2): z2 is the optional second addend (fm_part + dnn_part)."""
        y = ops.act_fwd(ops.ACT_SIGMOID, z.contiguous(), z2.contiguous().reshape(z.shape) if z2 is not None else None)
        ctx.save_for_backward(y)
        ctx.shape2 = z2.shape if z2 is not None else None
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        gz = ops.act_bwd(ops.ACT_SIGMOID, y, g.contiguous())
        return gz, (gz.reshape(ctx.shape2) if ctx.shape2 is not None else None)


# ---------------------------------------------------------------------------------------------------
# DIN (5.DIN/CustomLayers.py:142-289)
# ---------------------------------------------------------------------------------------------------

class FeatAct(torch.autograd.Function):
    """Per-feature activation on [M,N]: Dice (inference-mode BN statistics), PReLU or a named activation."""

    @staticmethod
    def forward(ctx, x, kind, alpha, mean, var):
        x = x.contiguous()
        ctx.kind = kind
        ctx.save_for_backward(x, alpha, mean, var)
        return ops.feat_act_fwd(kind, x, alpha, mean, var)

    @staticmethod
    def backward(ctx, gy):
        x, alpha, mean, var = ctx.saved_tensors
        want_a = alpha is not None and ctx.needs_input_grad[2]
        gx, ga = ops.feat_act_bwd(ctx.kind, x, gy.contiguous(), alpha, mean, var, want_alpha=want_a)
        return gx, None, (ops.colsum(ga) if want_a else None), None, None


class LayerNorm(torch.autograd.Function):
    """tf.keras.layers.LayerNormalization(epsilon) over the last axis; ``epsilon`` None: Keras' default 1e-3."""

    @staticmethod
    def forward(ctx, x, gamma, beta, epsilon=None):
        y, xhat, rstd = ops.layernorm_fwd(x.contiguous(), gamma, beta, epsilon)
        ctx.save_for_backward(xhat, rstd, gamma)
        return y

    @staticmethod
    def backward(ctx, gy):
        xhat, rstd, gamma = ctx.saved_tensors
        gy = gy.contiguous()
        gx, gg = ops.layernorm_bwd(gy, xhat, rstd, gamma)
        return gx, ops.colsum(gg), ops.colsum(gy), None


class Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = ops.softmax_fwd(x.contiguous())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return ops.softmax_bwd(y, gy.contiguous())


class DinAttention(torch.autograd.Function):
    """DinActivationLayer over every time step + mask + weighted sum pooling (5.DIN/CustomLayers.py:173-180,
    256-282), bilinear-factorised.  Inputs: table, q = flattened candidate-item embedding [B,D], series ids
    [B,T,C], the Dense(H) kernel W1 [3D+D*D,H] / bias b1, the activation's parameters, the Dense(1) kernel W2 [H,1]
    / bias b2.  Returns pooled [B,D] and the raw scores [B,T]; the scores are differentiable only with ``score_grad``
    (the single-key path, whose result they are): DINLayer consumes pooled alone."""

    @staticmethod
    def forward(ctx, embed, q, series, W1, b1, kind, alpha, mean, var, W2, b2, padding_index, mask_valid, oob,
                sink=None, score_grad=False):
        q = q.contiguous()
        B, D = q.shape
        H = W1.shape[1]
        Wcat, Wkd, bext = ops.din_prepare(W1.contiguous(), b1.contiguous(), D, H)
        Mext = ops.gemm(q, Wcat, epi=ops.EPI_BIAS, bias=bext)                 # [B, D*H + H] on the matrix cores
        w2 = W2.contiguous().reshape(-1)
        scores, pooled = ops.din_attn_fwd(embed, series, Mext, Wkd, kind, alpha, mean, var, w2, b2.contiguous(),
                                          padding_index, mask_valid, oob)
        ctx.save_for_backward(embed, q, series, Wcat, Wkd, Mext, alpha, mean, var, w2, b2, scores)
        ctx.cfg = (kind, padding_index, mask_valid, D, H)
        ctx.sink = sink
        if score_grad:
            ctx.set_materialize_grads(False)                 # an output nobody used arrives as None, not as zeros
        else:
            ctx.mark_non_differentiable(scores)
        return pooled, scores

    @staticmethod
    def backward(ctx, gpooled, gscores):
        embed, q, series, Wcat, Wkd, Mext, alpha, mean, var, w2, b2, scores = ctx.saved_tensors
        kind, padding_index, mask_valid, D, H = ctx.cfg
        V, E = embed.shape
        B = q.shape[0]
        if gpooled is None:                                  # only the scores were used (score_grad)
            gpooled = torch.zeros((B, D), dtype=torch.float32, device=q.device)
        if gscores is not None:
            gscores = gscores.contiguous()
        buf, (dst,) = _sink_dsts(ctx.sink, E, embed.device, series)
        gkeys, gMext, gw2p, galphap, gb2p = ops.din_attn_bwd(embed, series, Mext, Wkd, kind, alpha, mean, var, w2, b2,
                                                             padding_index, mask_valid, scores, gpooled.contiguous(),
                                                             gkeys=dst, gscores=gscores)
        gq = ops.gemm(gMext, Wcat, transB=True)                                          # [B,D]
        gWcat = ops.gemm(q, gMext, transA=True, split_k=ops.split_k_for(B, D, D * H + H, True, False))  # [D, D*H+H]
        gbext = ops.colsum(gMext)
        gWkd = gbext[:D * H].reshape(D, H)                    # Eff_b = Wkd + M_b  =>  dWkd = sum_b dEff_b: the leading
                                                              # D*H column sums of gMext, already in gbext
        gW1 = ops.din_prepare_bwd(gWcat, gWkd, D, H)
        gb1 = gbext[D * H:].clone()
        gW2 = ops.colsum(gw2p).reshape(H, 1)
        galpha = ops.colsum(galphap) if alpha is not None else None
        gb2 = ops.colsum(gb2p)
        gembed = _series_grad(ctx, series, gkeys, V, E, ctx.sink, buf)
        return gembed, gq, None, gW1, gb1, None, galpha, None, None, gW2, gb2, None, None, None, None, None


class EmbIpn(torch.autograd.Function):
    """PNN inner-product front end, fused with the lookup: X [B,F] -> [Flatten(embed(X)) | <e_i,e_j>, i<j]
    (2.FM/CustomLayers.py:737-745 with IpnLayer :773-792).  Backward: IndexedSlices values from the saved output."""

    @staticmethod
    def forward(ctx, table, X, oob):
        out = ops.emb_ipn_fwd(table, X, oob)
        ctx.save_for_backward(X, out)
        ctx.shape = tuple(table.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        X, out = ctx.saved_tensors
        V, E = ctx.shape
        vals = ops.emb_ipn_bwd_vals(out, g.contiguous(), X.shape[1], E)
        plan = ops.DedupPlan(X, V)
        return _sparse_grad(plan, vals, E, (V, E)), None, None


class EmbBiInteraction(torch.autograd.Function):
    """NFM bi-interaction pooling fused with the lookup, written into the leading columns of
    [second_order | X_cont] (3.DCN/CustomLayers.py:493-503): returns that combined matrix."""

    @staticmethod
    def forward(ctx, table, X, cont, oob):
        V, E = table.shape
        B = X.shape[0]
        nc = 0 if cont is None else cont.shape[1]
        comb = torch.empty((B, E + nc), dtype=torch.float32, device=table.device)
        _, S = ops.emb_bi_fwd(table, X, comb, oob)
        if nc:
            comb[:, E:] = cont
        ctx.save_for_backward(table, X, S)
        ctx.nc = nc
        return comb

    @staticmethod
    def backward(ctx, g):
        table, X, S = ctx.saved_tensors
        V, E = table.shape
        g = g.contiguous()
        vals = ops.emb_bi_bwd_vals(table, X, g, S)
        plan = ops.DedupPlan(X, V)
        gcont = g[:, E:].contiguous() if ctx.nc and ctx.needs_input_grad[2] else None
        return _sparse_grad(plan, vals, E, (V, E)), None, gcont, None


class IpAttention(torch.autograd.Function):
    """GSU inner-product attention + sum pooling over the embedded behaviour series, fused with the series lookup
    (7.SIM/CustomLayers.py:88-96,107-118).  Returns pooled [B,D] and the masked scores [B,T]."""

    @staticmethod
    def forward(ctx, embed, q, series, padding_index, oob, sink=None):
        q = q.contiguous()
        scores, pooled = ops.ip_attn_fwd(embed, series, q, padding_index, oob)
        ctx.save_for_backward(embed, q, series, scores)
        ctx.padding_index = padding_index
        ctx.sink = sink
        ctx.mark_non_differentiable(scores)
        return pooled, scores

    @staticmethod
    def backward(ctx, gpooled, _gscores):
        embed, q, series, scores = ctx.saved_tensors
        V, E = embed.shape
        buf, (dst,) = _sink_dsts(ctx.sink, E, embed.device, series)
        gkeys, gq = ops.ip_attn_bwd(embed, series, q, ctx.padding_index, scores, gpooled.contiguous(), gkeys=dst)
        return _series_grad(ctx, series, gkeys, V, E, ctx.sink, buf), gq, None, None, None, None


class BatchNorm(torch.autograd.Function):
    """tf.keras.layers.BatchNormalization on [B,N] (training: batch statistics, moving averages updated in place)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, moving_mean, moving_var, training, eps, momentum):
        y, xhat, rstd = ops.batchnorm_fwd(x.contiguous(), gamma, beta, moving_mean, moving_var, training, eps, momentum)
        ctx.save_for_backward(xhat, rstd, gamma)
        ctx.training = training
        return y

    @staticmethod
    def backward(ctx, g):
        xhat, rstd, gamma = ctx.saved_tensors
        gx, ggamma, gbeta = ops.batchnorm_bwd(g.contiguous(), xhat, rstd, gamma, ctx.training)
        return gx, ggamma, gbeta, None, None, None, None, None


class FFM(torch.autograd.Function):
    """FFM logit: bias + first order + field-aware second order, fused with the lookups
    (2.FM/CustomLayers.py:398-425 / 428-462, 480-494).  v [V,F,E], w [V,1], bias [1], X [B,F] -> z [B]."""

    @staticmethod
    def forward(ctx, v, w, bias, X, oob):
        z, _ = ops.ffm_fwd(v, w, bias, X, oob=oob)
        ctx.save_for_backward(v, X)
        return z

    @staticmethod
    def backward(ctx, gz):
        v, X = ctx.saved_tensors
        V, F, E = v.shape
        B = X.shape[0]
        gz = gz.contiguous()
        plan = ops.DedupPlan(X, V)
        rows = ops.ffm_bwd_rows(v, X, gz, plan)
        g_v = SparseRowGrad(plan.uniq_ids, rows, plan.n_uniq, (V, F, E)).to_sparse()
        g_w = _sparse_grad(plan, gz.reshape(B, 1), 1, (V, 1), row_div=F)
        return g_v, g_w, ops.colsum(gz.reshape(B, 1)), None, None


class CIN(torch.autograd.Function):
    """CINLayer (3.DCN/CustomLayers.py:396-417): x0 [B,F,E], W_k (1, F*H_k, H_{k+1}) -> cin_part [B, sum H].  The
    states X^1..X^L [B, sum H, E] are saved for the backward, which writes dx0 and every dW_k (csrc/cin.hip)."""

    @staticmethod
    def forward(ctx, x0, *Ws):
        x0 = x0.contiguous()
        Ws = [w.contiguous() for w in Ws]
        cin_part, states = ops.cin_fwd(x0, Ws)
        ctx.save_for_backward(x0, states, *Ws)
        return cin_part

    @staticmethod
    def backward(ctx, g):
        x0, states, *Ws = ctx.saved_tensors
        dx0, dWs = ops.cin_bwd(x0, states, g.contiguous(), Ws)
        return (dx0, *dWs)


class FiBiNetInteraction(torch.autograd.Function):
    """SENet + bilinear interaction of FiBiNetLayer (3.DCN/CustomLayers.py:936-1011) as one kernel each way
    (csrc/fibinet.hip): x_emb [B,F,E], x_cont [B,C], S0 [F,mid], S1 [mid,F], W [nW,E,E] ->
    dnn_in [B, 2PE + C] = [raw pairs | SENet pairs | x_cont].  The continuous columns get no gradient (as in
    ConcatCols).  ``pack`` maps the trailing weight tensors to W and ``unpack`` maps dW back onto them."""

    @staticmethod
    def forward(ctx, x_emb, x_cont, S0, S1, type_code, pack, *Ws):
        x_emb, S0, S1 = x_emb.contiguous(), S0.contiguous(), S1.contiguous()
        W = pack(Ws)
        dnn_in, A, H1 = ops.fibinet_fwd(x_emb, x_cont.contiguous(), S0, S1, W, type_code)
        ctx.save_for_backward(x_emb, A, H1, S0, S1, W)
        ctx.type_code = type_code
        return dnn_in

    @staticmethod
    def backward(ctx, g):
        x_emb, A, H1, S0, S1, W = ctx.saved_tensors
        dx, dW, dS0, dS1 = ops.fibinet_bwd(x_emb, g.contiguous(), A, H1, S0, S1, W, ctx.type_code)
        return (dx, None, dS0, dS1, None, None, *dW.unbind(0))


class AutoIntAttention(torch.autograd.Function):
    """One TransformerAttentionLayer (3.DCN/CustomLayers.py:1012-1067) as one forward and one backward call of
    csrc/autoint.hip: x [B,Fc,E] -> y = relu(O (+ X | + X Wres)) [B,F,E], the softmax over the BATCH axis.  When
    x_cont [B,C] and cemb [C,E] are given, the C continuous fields cemb[c] * x_cont[:, c] are appended after the Fc
    categorical ones inside the kernels (AutoIntLayer's first layer); x_cont gets no gradient.  res: 0 / 1 / 2 =
    no residual / + X / + X Wres (Wres may be None unless res == 2)."""

    @staticmethod
    def forward(ctx, x, x_cont, cemb, Wq, Wk, Wv, Wres, num_heads, res, scaling):
        x = x.contiguous()
        if x_cont is not None:
            x_cont, cemb = x_cont.contiguous(), cemb.contiguous()
        Wq, Wk, Wv = Wq.contiguous(), Wk.contiguous(), Wv.contiguous()
        Wres = Wres.contiguous() if res == 2 else None
        y, stats, _ = ops.autoint_fwd(x, Wq, Wk, Wv, Wres, num_heads, res, scaling, x_cont, cemb)
        ctx.save_for_backward(x, x_cont, cemb, Wq, Wk, Wv, Wres, y, stats)
        ctx.cfg = (num_heads, res, scaling)
        return y

    @staticmethod
    def backward(ctx, g):
        x, x_cont, cemb, Wq, Wk, Wv, Wres, y, stats = ctx.saved_tensors
        num_heads, res, scaling = ctx.cfg
        dx, dWq, dWk, dWv, dWres, dcemb = ops.autoint_bwd(x, Wq, Wk, Wv, Wres, y, g.contiguous(), stats, num_heads, res,
                                                          scaling, x_cont, cemb)
        return dx, None, dcemb, dWq, dWk, dWv, dWres, None, None, None


class EmbAFM(torch.autograd.Function):
    """Attentional FM pooling fused with the lookup (3.DCN/CustomLayers.py:825-853, 870-881; csrc/afm.hip): table, X
    [B,F], attention_w (Wa [E,A], ba [A]), attention_h (hv [A,1], bh [1]) -> o [B,E] = sum_k softmax_k(s)_k e_i * e_j.
    Backward: the sparse row gradient of the table and the four dense ones, one launch plus the slot sum.
    ``SAVE_ROWS``: keep the gathered rows [B,F,E] for the backward instead of gathering them again (DESIGN.md 3.2 has
    the measurement behind the default)."""

    SAVE_ROWS = False

    @staticmethod
    def forward(ctx, table, X, Wa, ba, hv, bh, oob):
        Wa, ba, hv, bh = Wa.contiguous(), ba.contiguous(), hv.contiguous(), bh.contiguous()
        o, stats, rows = ops.emb_afm_fwd(table, X, Wa, ba, hv, bh, oob, want_rows=EmbAFM.SAVE_ROWS)
        ctx.save_for_backward(table, X, Wa, ba, hv, bh, o, stats, rows)
        return o

    @staticmethod
    def backward(ctx, g):
        table, X, Wa, ba, hv, bh, o, stats, rows = ctx.saved_tensors
        V, E = table.shape
        vals, dWa, dba, dhv, dbh = ops.emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, g.contiguous(), rows)
        plan = ops.DedupPlan(X, V)
        return _sparse_grad(plan, vals, E, (V, E)), None, dWa, dba, dhv, dbh, None


def _flatten_weights(weights):
    """[K_1, b_1, K_2, b_2, ...] -> (the flat params K_1 | b_1 | K_2 | b_2 | ..., their shapes)."""
    return torch.cat([w.reshape(-1) for w in weights]), [tuple(w.shape) for w in weights]


def _split_like(flat, shapes):
    """The inverse of _flatten_weights: views of ``flat`` in the weights' shapes."""
    out, at = [], 0
    for shp in shapes:
        n = math.prod(shp)
        out.append(flat[at:at + n].reshape(shp))
        at += n
    return out


class EmbCCPM(torch.autograd.Function):
    """CCPM's conv / k-max-pool stack fused with the lookup (3.DCN/CustomLayers.py:621-677; csrc/ccpm.hip): table, X
    [B,F], and per layer the Conv2D kernel [kw,1,Cin,Cout] and bias [Cout] -> Flatten of the last pooling,
    [B, 3 E C_L].  Backward: the sparse row gradient of the table and every kernel's and bias's gradient, one launch plus
    the slot sum.  ``SAVE_ROWS``: keep the gathered rows [B,F,E] for the backward instead of gathering them again
    (DESIGN.md 3.2 has the measurement behind the default)."""

    SAVE_ROWS = False

    @staticmethod
    def forward(ctx, table, X, filters, kernel_width, oob, *weights):
        params, shapes = _flatten_weights(weights)
        out, rows = ops.emb_ccpm_fwd(table, X, params, filters, kernel_width, oob, want_rows=EmbCCPM.SAVE_ROWS)
        ctx.save_for_backward(table, X, params, rows)
        ctx.cfg = (list(filters), list(kernel_width), shapes)
        return out

    @staticmethod
    def backward(ctx, g):
        table, X, params, rows = ctx.saved_tensors
        filters, kernel_width, shapes = ctx.cfg
        V, E = table.shape
        vals, dparams = ops.emb_ccpm_bwd(table, X, params, filters, kernel_width, g.contiguous(), rows)
        plan = ops.DedupPlan(X, V)
        return (_sparse_grad(plan, vals, E, (V, E)), None, None, None, None, *_split_like(dparams, shapes))


class EmbFGCNN(torch.autograd.Function):
    """FGCNN's conv / max-pool stack fused with the lookup (3.DCN/CustomLayers.py:757-767; csrc/fgcnn.hip): table, X
    [B,F], and per layer the Conv2D kernel [kw,1,Cin,Cout] and bias [Cout] -> (rows [B,F,E], p_1, ..., p_L) with p_j
    [B, H_j E C_j] the Flatten of the j-th pooled map.  Every output has consumers of its own (the rows go into the MLP
    input, each p_j into its recombination Dense), so the backward takes a gradient per output, None read as zeros:
    the sparse row gradient of the table and every kernel's and bias's gradient, one launch plus the slot sum."""

    @staticmethod
    def forward(ctx, table, X, filters, kernel_width, pooling_width, oob, *weights):
        params, shapes = _flatten_weights(weights)
        rows, pooled = ops.emb_fgcnn_fwd(table, X, params, filters, kernel_width, pooling_width, oob)
        ctx.save_for_backward(X, params, rows)
        ctx.cfg = (list(filters), list(kernel_width), list(pooling_width), shapes, tuple(table.shape),
                   [tuple(p.shape) for p in pooled])
        ctx.set_materialize_grads(False)
        return (rows, *pooled)

    @staticmethod
    def backward(ctx, grows, *gpooled):
        X, params, rows = ctx.saved_tensors
        filters, kernel_width, pooling_width, shapes, (V, E), pshapes = ctx.cfg
        dps = [g.contiguous() if g is not None else torch.zeros(shp, dtype=torch.float32, device=rows.device)
               for g, shp in zip(gpooled, pshapes)]
        vals, dparams = ops.emb_fgcnn_bwd(rows, params, filters, kernel_width, pooling_width, dps,
                                          grows.contiguous() if grows is not None else None)
        plan = ops.DedupPlan(X, V)
        return (_sparse_grad(plan, vals, E, (V, E)), None, None, None, None, None, *_split_like(dparams, shapes))


class EmbFieldLayerNorm(torch.autograd.Function):
    """MaskNet's input stage fused with the lookup (11.FiBiNet++/CustomLayers.py:260-311; csrc/masknet.hip): table, X
    [B,F] whose last Fk columns are the keys of the continuous features, values [B,Fk] (None when Fk == 0), gamma / beta
    [F,E] of the per-field LayerNormalizations -> (x_emb [B, F E], x_norm [B, F E]).  Both outputs have consumers (every
    mask block reads x_emb), so the backward takes a gradient per output, None read as zeros: the sparse row gradient of
    the table, dgamma and dbeta, one launch plus the slot sum.  ``values`` is an input and gets no gradient."""

    @staticmethod
    def forward(ctx, table, X, values, gamma, beta, oob):
        gamma, beta = gamma.contiguous(), beta.contiguous()
        x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X, values, gamma, beta, oob)
        ctx.save_for_backward(X, values, gamma, x_emb, stats)
        ctx.shape = tuple(table.shape)
        ctx.set_materialize_grads(False)
        return x_emb, x_norm

    @staticmethod
    def backward(ctx, g_emb, g_norm):
        X, values, gamma, x_emb, stats = ctx.saved_tensors
        V, E = ctx.shape
        g_norm = g_norm.contiguous() if g_norm is not None else torch.zeros_like(x_emb)
        vals, dgamma, dbeta = ops.emb_masknet_ln_bwd(x_emb, stats, values, gamma, g_norm,
                                                     g_emb.contiguous() if g_emb is not None else None)
        plan = ops.DedupPlan(X, V)
        return _sparse_grad(plan, vals, E, (V, E)), None, None, dgamma, dbeta, None


class MaskDxSink:
    """The one dLoss/dx_emb buffer of a MaskNet stack: every block's backward adds its share into it in the order
    autograd runs them (fixed: the reverse of the forward), and the block that arrives last hands the buffer on and
    re-arms the sink, so a second backward over a retained graph starts from a fresh buffer.  Every one of the n blocks
    must take part in a backward pass: a block whose output is cut out of the graph would leave the others' shares
    undelivered, so a pass that starts while an earlier one is incomplete raises instead."""

    def __init__(self, n_blocks):
        self.n = int(n_blocks)
        self.left = self.n
        self.buf = None
        self.seen = set()

    def add(self, key, run):
        """run(buf) -> the buffer with this block's share added (buf None: a new one); -> dx_emb or None"""
        if key in self.seen:
            raise RuntimeError("MaskDxSink: a mask block ran its backward twice before all %d blocks of the stack had "
                               "run once; every block of a stack must be part of the differentiated graph" % self.n)
        self.seen.add(key)
        self.buf = run(self.buf)
        self.left -= 1
        if self.left:
            return None
        out, self.buf, self.left = self.buf, None, self.n
        self.seen.clear()
        return out


class MaskBlock(torch.autograd.Function):
    """One mask block (11.FiBiNet++/CustomLayers.py:314-337; csrc/masknet.hip): y = relu(LayerNorm((v * (relu(x_emb W1 +
    b1) W2 + b2)) W3 + b3)), one launch each way plus the slot sum and the three weight-gradient GEMMs.  With a ``sink``
    shared by the n blocks of a stack, the gradient of x_emb is returned once, by the last of them to run."""

    @staticmethod
    def forward(ctx, x_emb, v, W1, b1, W2, b2, W3, b3, gamma, beta, sink):
        args = [t.contiguous() for t in (x_emb, v, W1, b1, W2, b2, W3, b3, gamma, beta)]
        train = any(ctx.needs_input_grad)
        y, saved = ops.mask_block_fwd(*args, save=train)
        if train:
            x_emb, v, W1, _, W2, _, W3, _, gamma, _ = args
            ctx.save_for_backward(x_emb, v, W1, W2, W3, gamma, y, *saved)
            ctx.sink = sink
        return y

    @staticmethod
    def backward(ctx, dy):
        x_emb, v, W1, W2, W3, gamma, y, *saved = ctx.saved_tensors
        sink, dy = ctx.sink, dy.contiguous()
        if sink is None:
            dv, dx, g = ops.mask_block_bwd(x_emb, v, W1, W2, W3, gamma, y, saved, dy)
        else:
            out = {}

            def run(buf):
                out["dv"], buf, out["g"] = ops.mask_block_bwd(x_emb, v, W1, W2, W3, gamma, y, saved, dy, dx_emb=buf,
                                                              accumulate=buf is not None)
                return buf

            dx = sink.add(id(ctx), run)
            dv, g = out["dv"], out["g"]
        dW1, db1, dW2, db2, dW3, db3, dgamma, dbeta = g
        return dx, dv, dW1, db1, dW2, db2, dW3, db3, dgamma, dbeta, None


class EmbScaledLookup(torch.autograd.Function):
    """ContextNet's input stage fused with the lookup (11.FiBiNet++/CustomLayers.py:492-523; csrc/contextnet.hip): table,
    X [B,F] whose last Fk columns are the keys of the continuous features, values [B,Fk] (None when Fk == 0) -> x
    [B, F E], the key rows multiplied by their value.  Backward: the sparse row gradient of the table, one launch plus
    the dedup + segment sum.  ``values`` is an input and gets no gradient."""

    @staticmethod
    def forward(ctx, table, X, values, oob):
        x = ops.emb_contextnet_in_fwd(table, X, values, oob)
        ctx.save_for_backward(X, values)
        ctx.shape = tuple(table.shape)
        return x

    @staticmethod
    def backward(ctx, g):
        X, values = ctx.saved_tensors
        V, E = ctx.shape
        vals = ops.emb_contextnet_in_bwd(g.contiguous(), values, X.shape[1])
        plan = ops.DedupPlan(X, V)
        return _sparse_grad(plan, vals, E, (V, E)), None, None, None


class ContextNetBlock(torch.autograd.Function):
    """One ContextNet block (11.FiBiNet++/CustomLayers.py:412-471; csrc/contextnet.hip): x [B, F E], the contextual
    embedding MLP Wa, ba, Wb, bb, the fields' W1 [F,E,E], W2 [F,E,E] (None: the single-matrix mode) and LayerNorm gamma,
    beta [F,E] -> y [B, F E], one launch each way plus the slot sums, the batched per-field weight gradients and the two
    weight-gradient GEMMs."""

    @staticmethod
    def forward(ctx, x, Wa, ba, Wb, bb, W1, W2, gamma, beta):
        args = [t.contiguous() if t is not None else None for t in (x, Wa, ba, Wb, bb, W1, W2, gamma, beta)]
        train = any(ctx.needs_input_grad)
        y, saved = ops.contextnet_block_fwd(*args, save=train)
        if train:
            x, Wa, _, Wb, _, W1, W2, gamma, _ = args
            ctx.save_for_backward(x, Wa, Wb, W1, W2, gamma, *saved)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, Wa, Wb, W1, W2, gamma, *saved = ctx.saved_tensors
        dx, (dWa, dba, dWb, dbb, dW1, dW2, dgamma, dbeta) = ops.contextnet_block_bwd(x, Wa, Wb, W1, W2, gamma, saved,
                                                                                     dy.contiguous())
        return dx, dWa, dba, dWb, dbb, dW1, dW2, dgamma, dbeta


class EmbNormLookup(torch.autograd.Function):
    """FiBiNet++'s input stage fused with the lookup (11.FiBiNet++/CustomLayers.py:78-145; csrc/fibinetplus.hip): table,
    X [B,F] whose last Fk columns are the keys of the continuous features, values [B,Fk] (None when Fk == 0), the ONE
    BatchNormalization of the categorical rows (gamma, beta, moving mean / variance [E]; ``training``: batch statistics,
    the moving averages updated in place) and the key fields' LayerNormalizations (gamma, beta [Fk,E]) -> x [B, F E].
    Backward: the sparse row gradient of the table and the four norm gradients.  ``values`` gets no gradient."""

    @staticmethod
    def forward(ctx, table, X, values, gamma_bn, beta_bn, gamma_ln, beta_ln, moving_mean, moving_var, training, oob):
        cg = lambda t: t.contiguous() if t is not None else None
        gamma_bn, beta_bn, gamma_ln, beta_ln = cg(gamma_bn), cg(beta_bn), cg(gamma_ln), cg(beta_ln)
        x, saved = ops.emb_fibinetplus_in_fwd(table, X, values, gamma_bn, beta_bn, gamma_ln, beta_ln, moving_mean,
                                              moving_var, training, oob)
        ctx.save_for_backward(X, values, gamma_bn, gamma_ln, *saved)
        ctx.shape = tuple(table.shape)
        ctx.training = bool(training)
        ctx.has = (gamma_bn is not None, gamma_ln is not None)
        return x

    @staticmethod
    def backward(ctx, g):
        X, values, gamma_bn, gamma_ln, *saved = ctx.saved_tensors
        V, E = ctx.shape
        vals, dg_bn, db_bn, dg_ln, db_ln = ops.emb_fibinetplus_in_bwd(g.contiguous(), values, saved, gamma_bn, gamma_ln,
                                                                      X.shape[1], ctx.training)
        plan = ops.DedupPlan(X, V)
        bn, ln = ctx.has
        return (_sparse_grad(plan, vals, E, (V, E)), None, None, dg_bn if bn else None, db_bn if bn else None,
                dg_ln if ln else None, db_ln if ln else None, None, None, None, None)


class FiBiNetPlusBlock(torch.autograd.Function):
    """The FiBiNet++ body (11.FiBiNet++/CustomLayers.py:170-242; csrc/fibinetplus.hip): x [B, F E], the bilinear+
    matrices W [nW,E,E] with their reducing Dense + LayerNorm (Wr, br, gamma_q, beta_q) and SENet+'s excitation (S0, b0,
    gamma0, beta0, S1, b1, gamma1, beta1) -> [q | x * A] [B, O + F E], one launch each way plus the slot sums, one launch
    for all bilinear weight gradients and three weight-gradient GEMMs.  ``packed`` maps the matrices' Parameters onto one
    [nW,E,E] array (BilinearInteractionPlusLayer.packed_weight)."""

    @staticmethod
    def forward(ctx, x, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1, G, type_code, packed, *ws):
        W = packed(ws).contiguous()
        args = [t.contiguous() for t in (x, W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1)]
        train = any(ctx.needs_input_grad)
        out, saved = ops.fibinetplus_block_fwd(*args, G, type_code, save=train)
        if train:
            x, W, Wr, _, gq, _, S0, _, g0, be0, S1, _, g1, be1 = args
            ctx.save_for_backward(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, *saved)
        ctx.G, ctx.type_code = G, type_code
        return out

    @staticmethod
    def backward(ctx, dout):
        x, W, Wr, gq, S0, g0, be0, S1, g1, be1, *saved = ctx.saved_tensors
        dx, g = ops.fibinetplus_block_bwd(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, ctx.G, ctx.type_code, saved,
                                          dout.contiguous())
        dW, dWr, dbr, dgq, dbq, dS0, db0, dg0, dbe0, dS1, db1, dg1, dbe1 = g
        return (dx, dWr, dbr, dgq, dbq, dS0, db0, dg0, dbe0, dS1, db1, dg1, dbe1, None, None, None) + tuple(dW.unbind(0))


class MMOEBody(torch.autograd.Function):
    """The MMOE / ESMM body (4.MMOE/CustomLayers.py:152-172, 221-244; csrc/mmoe.hip): x [B, D] and the packed weights W1,
    b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 (include/mi355rec.h) -> out [B, T], one launch each way plus the
    slot sums, one launch for all small weight gradients and one weight-gradient GEMM."""

    @staticmethod
    def forward(ctx, x, gate_softmax_passes, ctcvr, *weights):
        x = x.contiguous()
        weights = [t.contiguous() for t in weights]
        train = any(ctx.needs_input_grad)
        out, saved = ops.mmoe_fwd(x, weights, gate_softmax_passes, ctcvr, save=train)
        if train:
            ctx.save_for_backward(x, *weights, *saved)
        ctx.flags = (gate_softmax_passes, ctcvr)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, *rest = ctx.saved_tensors
        weights, saved = rest[:12], rest[12:]
        dx, grads = ops.mmoe_bwd(x, weights, saved, dout.contiguous(), *ctx.flags)
        return (dx, None, None) + tuple(grads)


class PLELevel(torch.autograd.Function):
    """One CGC level of PLE (4.MMOE/CustomLayers.py:315-358 and the towers :380-382; csrc/ple.hip): xin [B, Gin, Din]
    (Gin = 1 for the first level, tasks + 1 afterwards) and the packed weights W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h,
    Wtw, btw (include/mi355rec.h; None for the shared gate of the last level and for the towers of the others) ->
    y [B, Gout, O], and for the last level (y, out [B, T]).  One launch each way plus the slot sums, one launch for all
    small weight gradients and, for the first level, one weight-gradient GEMM.  Saves only under grad."""

    @staticmethod
    def forward(ctx, xin, T, S, Sh, last, *weights):
        xin = xin.contiguous()
        weights = [None if t is None else t.contiguous() for t in weights]
        train = any(ctx.needs_input_grad)
        y, out, saved = ops.ple_cgc_fwd(xin, weights, T, S, Sh, last, save=train)
        if train:
            ctx.save_for_backward(xin, *weights, *saved, y, out)
        ctx.cfg = (T, S, Sh, bool(last))
        return (y, out) if last else y

    @staticmethod
    def backward(ctx, dy, dout=None):
        xin, *rest = ctx.saved_tensors
        weights, saved, y, out = rest[:10], rest[10:14], rest[14], rest[15]
        last = ctx.cfg[3]
        dxin, grads = ops.ple_cgc_bwd(xin, weights, saved, y, out, None if dy is None else dy.contiguous(),
                                      dout.contiguous() if last else None, *ctx.cfg)
        return (dxin, None, None, None, None) + tuple(grads)


class CapsuleRouting(torch.autograd.Function):
    """MultiInterestExtractorLayer.call fused with the series lookup (6.MIND/CustomLayers.py:111-138, 204-212;
    csrc/mind.hip): table, series ids [B,T,C], S [C E, Dc], the non-trainable logits B0 [K,T] -> the capsules [B,K,Dc].
    One launch forward, which saves nothing but its inputs; the backward runs the rounds again and differentiates
    through all of them.  The table's gradient is a sparse COO tensor of de-duplicated rows; B0 gets none."""

    @staticmethod
    def forward(ctx, embed, series, S, B0, routing_rounds, padding_index, oob):
        S, B0 = S.contiguous(), B0.contiguous()
        out = ops.mind_routing_fwd(embed, series, S, B0, routing_rounds, padding_index, oob)
        ctx.save_for_backward(embed, series, S, B0)
        ctx.cfg = (routing_rounds, padding_index)
        return out

    @staticmethod
    def backward(ctx, gout):
        embed, series, S, B0 = ctx.saved_tensors
        V, E = embed.shape
        gkeys, dS = ops.mind_routing_bwd(embed, series, S, B0, gout.contiguous(), *ctx.cfg)
        return _series_grad(ctx, series, gkeys, V, E), None, dS, None, None, None, None


class LabelAwareAttention(torch.autograd.Function):
    """LabelAwareAttention, the inner products with the sampled items and the sampled-softmax loss, fused with the item
    lookup (6.MIND/CustomLayers.py:141-158, 252-285; csrc/mind.hip): table, item ids [B,Ns,C], capsules m [B,K,C E],
    valid capsule counts kv int32 [B] -> (out [B,Ns], loss [B]).  One launch each way; an output nobody used arrives as
    None in the backward, not as zeros."""

    @staticmethod
    def forward(ctx, embed, items, m, kv, oob):
        m = m.contiguous()
        out, loss = ops.mind_laa_fwd(embed, items, m, kv, oob)
        ctx.save_for_backward(embed, items, m, kv)
        ctx.set_materialize_grads(False)
        return out, loss

    @staticmethod
    def backward(ctx, gout, gloss):
        embed, items, m, kv = ctx.saved_tensors
        V, E = embed.shape
        gm, gitems = ops.mind_laa_bwd(embed, items, m, kv, None if gout is None else gout.contiguous(),
                                      None if gloss is None else gloss.contiguous())
        gembed = None
        if gout is not None or gloss is not None:
            gembed = _series_grad(ctx, items, gitems, V, E)
        return gembed, None, gm, None, None


class ComiRecRouting(torch.autograd.Function):
    """ComiRecDynamicRoutingLayer.call fused with the series lookup (6.MIND/CustomLayers.py:562-594, 714-724;
    csrc/comirec.hip): table, series ids [B,T,C], W [K,T,C E,Dc], the non-trainable logits B0 [K,T] -> the capsules
    [B,K,Dc].  The forward saves nothing but its inputs; the backward projects and routes again and differentiates
    through every round.  The table's gradient is a sparse COO tensor of de-duplicated rows; B0 gets none."""

    @staticmethod
    def forward(ctx, embed, series, W, B0, routing_rounds, padding_index, keep_padding, oob):
        W, B0 = W.contiguous(), B0.contiguous()
        out = ops.comirec_dr_fwd(embed, series, W, B0, routing_rounds, padding_index, keep_padding, oob)
        ctx.save_for_backward(embed, series, W, B0)
        ctx.cfg = (routing_rounds, padding_index, keep_padding)
        return out

    @staticmethod
    def backward(ctx, gout):
        embed, series, W, B0 = ctx.saved_tensors
        V, E = embed.shape
        gkeys, dW = ops.comirec_dr_bwd(embed, series, W, B0, gout.contiguous(), *ctx.cfg)
        return _series_grad(ctx, series, gkeys, V, E), None, dW, None, None, None, None, None


class ComiRecSelfAttention(torch.autograd.Function):
    """ComiRecSelfAttentiveLayer.call fused with the series lookup (6.MIND/CustomLayers.py:644-665; csrc/comirec.hip):
    table, series ids [B,T,C], W1 [C E,Dc], W2 [K,Dc], the constant positional table pos [T,C E] or None -> [B,K,Dc].
    One launch forward; the backward recomputes it."""

    @staticmethod
    def forward(ctx, embed, series, W1, W2, pos, padding_index, keep_padding, oob):
        W1, W2 = W1.contiguous(), W2.contiguous()
        out = ops.comirec_sa_fwd(embed, series, W1, W2, pos, padding_index, keep_padding, oob)
        ctx.save_for_backward(embed, series, W1, W2)
        ctx.pos, ctx.cfg = pos, (padding_index, keep_padding)
        return out

    @staticmethod
    def backward(ctx, gout):
        embed, series, W1, W2 = ctx.saved_tensors
        V, E = embed.shape
        gkeys, dW1, dW2 = ops.comirec_sa_bwd(embed, series, W1, W2, gout.contiguous(), ctx.pos, *ctx.cfg)
        return _series_grad(ctx, series, gkeys, V, E), None, dW1, dW2, None, None, None, None


class ComiRecSelect(torch.autograd.Function):
    """The hard attention of ComiRecLayer.manually_negative_sampled_call fused with the item lookup and the loss
    (6.MIND/CustomLayers.py:768-810; csrc/comirec.hip): table, item ids [B,Ns,C], capsules m [B,K,C E] -> (selected
    [B,Ns,C E], the capsule with the largest inner product per item, smallest index on a tie; inner [B,Ns]; loss [B];
    chosen int32 [B,Ns], not differentiable).  The backward uses the forward's ``chosen``; an output nobody used arrives
    as None, not as zeros."""

    @staticmethod
    def forward(ctx, embed, items, m, oob):
        m = m.contiguous()
        chosen, inner, loss = ops.comirec_select_fwd(embed, items, m, oob)
        selected = torch.gather(m, 1, chosen.long()[:, :, None].expand(-1, -1, m.shape[2]))
        ctx.save_for_backward(embed, items, m, chosen)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(chosen)
        return selected, inner, loss, chosen

    @staticmethod
    def backward(ctx, gsel, ginner, gloss, _gchosen):
        embed, items, m, chosen = ctx.saved_tensors
        V, E = embed.shape
        c = lambda g: None if g is None else g.contiguous()
        gm, gitems = ops.comirec_select_bwd(embed, items, m, chosen, c(ginner), c(gloss), c(gsel))
        gembed = None
        if gsel is not None or ginner is not None or gloss is not None:
            gembed = _series_grad(ctx, items, gitems, V, E)
        return gembed, None, gm, None


class SineInterest(torch.autograd.Function):
    """SINELayer.generate_user_interest fused with the series lookup (6.MIND/CustomLayers.py:1000-1130; csrc/sine.hip):
    table, series ids [B,T,C], the concept pool [L,C E], W1, W2, Wk1 [L,C E,C E], Wk2 [L,C E], W3, W4 -> (user_interest
    [B,C E], chosen int32 [B,K], every example's top-K concepts, not differentiable).  One launch forward, which saves
    nothing but its inputs and ``chosen``; the backward runs the forward again with that ``chosen`` and differentiates
    through all of it.  The table's gradient is a sparse COO tensor of de-duplicated rows."""

    @staticmethod
    def forward(ctx, embed, series, pool, W1, W2, Wk1, Wk2, W3, W4, K, tau, padding_index, oob):
        weights = tuple(w.contiguous() for w in (pool, W1, W2, Wk1, Wk2, W3, W4))
        out, chosen = ops.sine_interest_fwd(embed, series, *weights, K, tau, ops.SINE_LN_EPS, padding_index, oob)
        ctx.save_for_backward(embed, series, chosen, *weights)
        ctx.cfg = (tau, ops.SINE_LN_EPS, padding_index)
        ctx.mark_non_differentiable(chosen)
        return out, chosen

    @staticmethod
    def backward(ctx, gout, _gchosen):
        embed, series, chosen, *weights = ctx.saved_tensors
        V, E = embed.shape
        gkeys, *grads = ops.sine_interest_bwd(embed, series, *weights, chosen, gout.contiguous(), *ctx.cfg)
        return (_series_grad(ctx, series, gkeys, V, E), None, *grads, None, None, None, None)


class SineAux(torch.autograd.Function):
    """SINELayer.compute_auxiliary_loss (6.MIND/CustomLayers.py:1143-1157; csrc/sine.hip): the concept pool [L,D] -> the
    scalar 0.5 sum_{i != j} M_ij^2 of the centred pool's Gram matrix M.  Its gradient is zero where the off-diagonal is
    zero throughout (the reference's 0.5 square(norm) gives NaN there)."""

    @staticmethod
    def forward(ctx, pool):
        pool = pool.contiguous()
        ctx.save_for_backward(pool)
        return ops.sine_aux_fwd(pool)

    @staticmethod
    def backward(ctx, gloss):
        pool, = ctx.saved_tensors
        return ops.sine_aux_bwd(pool, gloss.reshape(1).contiguous())


class CoAction(torch.autograd.Function):
    """CoActionUnit.call fused with both lookups (7.SIM/CustomLayers.py:339-378; csrc/can.hip): the feed table [Vf,E],
    target ids iid [B], feed ids fid [B,T] and the induction tables [Vi,P] -- one per order, or ONE that every order reads
    -> out [order,B,T,Eo], or with ``pooled`` its sum over orders and positions [B,Eo].  Nothing but the inputs is saved;
    the backward runs the forward again.  Every table's gradient is a sparse COO tensor of de-duplicated rows: the feed
    table's over the B T feed ids, an induction table's over the B target ids (one plan serves all orders), and a shared
    table gets ONE gradient, the order * B value rows under one plan over the ids tiled ``order`` times."""

    @staticmethod
    def forward(ctx, feed, iid, fid, coefs, order, act, padding_index, pooled, oob, *inds):
        res = ops.can_fwd(feed, inds, iid, fid, coefs, order, act, padding_index, pooled, oob)
        ctx.save_for_backward(feed, iid, fid, *inds)
        ctx.cfg = (tuple(coefs), order, act)
        ctx.tail = (padding_index, pooled)
        return res

    @staticmethod
    def backward(ctx, g):
        feed, iid, fid, *inds = ctx.saved_tensors
        coefs, order, act = ctx.cfg
        gfeed, gind = ops.can_bwd(feed, inds, iid, fid, coefs, order, act, g.contiguous(), *ctx.tail)
        Vf, E = feed.shape
        Vi, P = inds[0].shape
        dfeed = _series_grad(ctx, fid, gfeed, Vf, E)
        dinds = [None] * len(inds)
        if len(inds) == 1 and ctx.needs_input_grad[9]:
            plan = ops.DedupPlan(iid.repeat(order), Vi)
            dinds[0] = _sparse_grad(plan, gind.reshape(-1, P), P, (Vi, P), wide=True)
        elif any(ctx.needs_input_grad[9:]):
            plan = ops.DedupPlan(iid, Vi)
            dinds = [_sparse_grad(plan, gind[o], P, (Vi, P), wide=True) if ctx.needs_input_grad[9 + o] else None
                     for o in range(order)]
        return (dfeed,) + (None,) * 8 + tuple(dinds)


class FinalMLPBody(torch.autograd.Function):
    """The FinalMLP body (8.DMR/CustomLayers.py:379-385, 406-442; csrc/finalmlp.hip): the shared rows xs [B, D], the rows
    x1 / x2 of the two gates and ONE packed parameter buffer (ops.finalmlp_param_shapes) -> out [B, o].  ``moving`` is the
    list of the 2 L moving means followed by the 2 L moving variances; in training they move in place on the device.
    Forward: 2 L + 1 launches in training, one in evaluation; the gradient of the packed buffer comes back as one tensor
    that autograd splits by the views the caller concatenated."""

    @staticmethod
    def forward(ctx, xs, x1, x2, params, moving, dims, training, eps, momentum):
        xs, x1, x2, params = (t.contiguous() for t in (xs, x1, x2, params))
        half = len(moving) // 2
        save = training or any(ctx.needs_input_grad)
        out, saved = ops.finalmlp_fwd(xs, x1, x2, params, moving[:half], moving[half:], dims, training, eps, momentum,
                                      save=save)
        if save:
            ctx.save_for_backward(xs, x1, x2, params, out, *saved)
        ctx.dims, ctx.training = dims, training
        return out

    @staticmethod
    def backward(ctx, dout):
        xs, x1, x2, params, out, *saved = ctx.saved_tensors
        dxs, dx1, dx2, dparams = ops.finalmlp_bwd(xs, x1, x2, params, saved, out, dout.contiguous(), ctx.dims,
                                                  ctx.training)
        return dxs, dx1, dx2, dparams, None, None, None, None, None


class DmrMatch(torch.autograd.Function):
    """DMRI2INetworkLayer, DMRU2INetworkLayer and compute_auxiliary_loss fused with the series and negative lookups
    (8.DMR/CustomLayers.py:203-316; csrc/dmr.hip): table, the candidate's rows xi [B,C E], series ids [B,T,C], negative
    ids [B,Nn,C], the positional table pos [T,C E], the i2i unit's Wc, Wp, We [C E,H] and z [H], the u2i unit's Wp, We
    and z -> (i2i [B,C E + 1], u2i [B,C E + 1], aux [B]).  P = pos [Wp_i2i | Wp_u2i] and q = xi Wc are GEMMs here; the
    rest is one launch each way, the backward recomputing from the ids.  An output nobody used arrives as None, not as
    zeros.  With ``sink`` (functional.GradSink) the values of both lookups ride along with the profile lookup's
    de-duplication and the table's gradient is returned there."""

    @staticmethod
    def forward(ctx, embed, xi, series, negatives, pos, Wc, Wp_i, We_i, z_i, Wp_u, We_u, z_u, padding_index, oob,
                sink=None):
        xi, pos, Wc = xi.contiguous(), pos.contiguous(), Wc.contiguous()
        Wp = torch.cat([Wp_i, Wp_u], dim=1)
        We = torch.cat([We_i, We_u], dim=1)
        z = torch.stack([z_i, z_u])
        P = ops.gemm(pos, Wp)
        q = ops.gemm(xi, Wc)
        i2i, u2i, aux = ops.dmr_fwd(embed, series, negatives, xi, q, P, We, z, padding_index, oob)
        ctx.save_for_backward(embed, xi, series, negatives, pos, Wc, Wp, We, z, P, q)
        ctx.padding_index, ctx.sink = padding_index, sink
        ctx.set_materialize_grads(False)
        return i2i, u2i, aux

    @staticmethod
    def backward(ctx, g_i2i, g_u2i, g_aux):
        embed, xi, series, negatives, pos, Wc, Wp, We, z, P, q = ctx.saved_tensors
        V, E = embed.shape
        B, D = xi.shape
        H = Wc.shape[1]
        c = lambda g: None if g is None else g.contiguous()
        buf, (dk, dn) = _sink_dsts(ctx.sink, E, embed.device, series, negatives)
        gkeys, gneg, gitem, gq, dP, dWe, dz = ops.dmr_bwd(embed, series, negatives, xi, q, P, We, z, c(g_i2i), c(g_u2i),
                                                          c(g_aux), ctx.padding_index, gkeys=dk, gneg=dn)
        gxi = ops.gemm(gq, Wc, transB=True, epi=ops.EPI_ADD, e1=gitem)       # through u . xi and through q = xi Wc
        dWc = ops.gemm(xi, gq, transA=True)
        dWp = ops.gemm(pos, dP, transA=True)
        dpos = ops.gemm(dP, Wp, transB=True)
        gembed = _series_grad(ctx, (series, negatives), (gkeys, gneg), V, E, ctx.sink, buf)
        return (gembed, gxi, None, None, dpos, dWc, dWp[:, :H], dWe[:, :H], dz[0], dWp[:, H:], dWe[:, H:], dz[1],
                None, None, None)


class EmbEPNetLookup(torch.autograd.Function):
    """PEPNet's embedding stage fused with the EPNet gates (10.POSO/CustomLayers.py:415-457; csrc/epnet.hip): table, ids
    [B, F + P] (F main ids, then the P personalisation ids) and the stacked GateNU weights A [F, P E, Hg], a [F, Hg], Bm
    [F, Hg, E], bm [F, E] -> u [B, (F + P) E]: the main rows times their gate, then the personalisation rows raw.
    Nothing but the ids is saved; the backward computes the gates again, returns the gate weights' gradients and hands
    the row gradients (the personalisation rows' from both of their uses) to the de-duplicated sparse path."""

    @staticmethod
    def forward(ctx, table, ids, F, oob, A, a, Bm, bm):
        weights = [t.contiguous() for t in (A, a, Bm, bm)]
        u = ops.epnet_lookup_fwd(table, ids, F, *weights, oob)
        ctx.save_for_backward(table, ids, *weights)
        ctx.F = F
        return u

    @staticmethod
    def backward(ctx, du):
        table, ids, *weights = ctx.saved_tensors
        V, E = table.shape
        vals, grads = ops.epnet_lookup_bwd(table, ids, ctx.F, *weights, du.contiguous())
        gtable = _sparse_grad(ops.DedupPlan(ids, V), vals, E, (V, E)) if ctx.needs_input_grad[0] else None
        return (gtable, None, None, None) + tuple(grads)


class PosoMLP(torch.autograd.Function):
    """T stacked POSO-MLPs of chained layers (10.POSO/CustomLayers.py:92-119; csrc/poso.hip): x [B, Dm], g [B, Dg] and
    the packed weights Wg1, bg1, Wg2, bg2, W, b, C (include/mi355rec.h) -> out [B, T, units[-1]]; one launch each way
    plus the slot sums, one launch for all small weight gradients and one weight-gradient GEMM.
    ``shared_cols`` > 0 is PEPNet's arrangement: ``x`` is None and the main input is the leading ``shared_cols`` columns
    of ``g`` (nothing is copied), which as part of the gate input stand behind a stop_gradient -- the gradient of ``g``
    is then dx in those columns and dg in the others."""

    @staticmethod
    def forward(ctx, x, g, units, acts, m, shared_cols, *weights):
        g = g.contiguous()
        x = g[:, :shared_cols] if shared_cols else x.contiguous()
        weights = [t.contiguous() for t in weights]
        train = any(ctx.needs_input_grad)
        out, saved = ops.poso_mlp_fwd(x, g, weights, units, acts, m, save=train)
        if train:
            ctx.save_for_backward(x, g, *weights, *saved)
        ctx.cfg = (list(units), list(acts), m)
        ctx.shared_cols = shared_cols
        return out

    @staticmethod
    def backward(ctx, dout):
        x, g, *rest = ctx.saved_tensors
        weights, saved = rest[:7], rest[7:]
        dx, dg, grads = ops.poso_mlp_bwd(x, g, weights, saved, dout.contiguous(), *ctx.cfg)
        if ctx.shared_cols:
            dg[:, :ctx.shared_cols].copy_(dx)             # stop_gradient: the gate path's share of these columns is dropped
            dx = None
        return (dx, dg, None, None, None, None) + tuple(grads)


class DienGru(torch.autograd.Function):
    """DIEN's interest extractor (5.DIN/CustomLayers.py:412, 434-453, 480-502; csrc/dien.hip): the masked
    tf.keras.layers.GRU (reset_after=True; ``kernel`` [H,3H], ``recurrent_kernel`` [H,3H], ``bias`` [2,3H], gate order
    z, r, h) fused with the series lookup and, with ``negatives``, the auxiliary loss -> (gru_output [B,T,H], h_final,
    aux).  Table mode: ``embed`` [V,E], ``series`` and ``negatives`` ids [B,T,C]; gru_output and aux (a scalar; None
    without negatives) are returned, h_final is None.  Dense mode (``embed`` None): ``x`` [B,T,H] with ``mask_ids``
    [B,T], DienGRU's AIGRU; only h_final is returned.  One recurrence launch each way; the backward recomputes the gates
    from the saved gru_output.  With ``sink`` (functional.GradSink) the values of both lookups ride along with the
    profile lookup's de-duplication and the table's gradient is returned there; ``after`` is then a tensor out of that
    lookup (the candidate's rows): it is not read and gets no gradient, the edge only makes autograd run this backward
    before the lookup's, which collects what the sink holds."""

    @staticmethod
    def forward(ctx, embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias, padding_index, oob=None,
                sink=None, after=None):
        kernel, recurrent_kernel, bias = kernel.contiguous(), recurrent_kernel.contiguous(), bias.contiguous()
        table = embed is not None
        if not table:
            x = x.contiguous()
        out, fin, aux = ops.dien_gru_fwd(kernel, recurrent_kernel, bias, embed, series, negatives, x, mask_ids,
                                         padding_index, oob, want_output=True, want_final=not table)
        ctx.save_for_backward(embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias, out)
        ctx.padding_index, ctx.sink = padding_index, sink
        ctx.set_materialize_grads(False)
        if table:
            return out, None, (aux.reshape(()) if aux is not None else None)
        ctx.mark_non_differentiable(out)
        return out, fin, None

    @staticmethod
    def backward(ctx, dout, dfin, gaux):
        embed, series, negatives, x, mask_ids, kernel, recurrent_kernel, bias, out = ctx.saved_tensors
        c = lambda g: None if g is None else g.contiguous()
        table = embed is not None
        buf, dk, dn = None, None, None
        if table:
            V, E = embed.shape
            buf, (dk, dn) = _sink_dsts(ctx.sink, E, embed.device, series, negatives)
        gaux = None if gaux is None else c(gaux).reshape(1)
        dx, dneg, dK, dU, db = ops.dien_gru_bwd(kernel, recurrent_kernel, bias, out, None if not table else c(dout),
                                                c(dfin), gaux, embed, series, negatives, x, mask_ids,
                                                ctx.padding_index, dx=dk, dneg=dn)
        gembed = _series_grad(ctx, (series, negatives), (dx, dneg), V, E, ctx.sink, buf) if table else None
        return gembed, None, None, (None if table else dx), None, dK, dU, db, None, None, None, None


class DienAugru(torch.autograd.Function):
    """DienActivationLayer and DienGRU's AGRU / AUGRU (5.DIN/CustomLayers.py:292-386; csrc/dien.hip): gru_output
    [B,T,H], the candidate's rows X_item [B,H], the bilinear W [H,H], the mask ids ([B,T] or the series ids [B,T,C]) and
    CustomGRUCell's weights -> (evolved interest [B,H], scores [B,T]).  q = X_item W^T is a GEMM here, the scores and
    the recurrence one launch each way; the backward recomputes the gates from the saved states.  The scores are
    returned for inspection and carry no gradient of their own."""

    @staticmethod
    def forward(ctx, gru_output, X_item, W, mask_ids, mode, padding_index, mask_valid, W_r, U_r, b_r, W_h, U_h, b_h,
                W_z=None, U_z=None, b_z=None):
        gru_output, X_item, W = gru_output.contiguous(), X_item.contiguous(), W.contiguous()
        if mode == ops.DIEN_AUGRU:
            Wx, Uh, bx = torch.cat([W_z, W_r, W_h], 1), torch.cat([U_z, U_r, U_h], 1), torch.cat([b_z, b_r, b_h])
        else:
            Wx, Uh, bx = torch.cat([W_r, W_h], 1), torch.cat([U_r, U_h], 1), torch.cat([b_r, b_h])
        q = ops.gemm(X_item, W, transB=True)
        train = any(ctx.needs_input_grad)
        scores, states, fin = ops.dien_augru_fwd(gru_output, q, mask_ids, mode, Wx, Uh, bx, padding_index, mask_valid,
                                                 save=train)
        if train:
            ctx.save_for_backward(gru_output, X_item, W, mask_ids, Wx, Uh, bx, q, scores, states)
        ctx.cfg = (mode, padding_index, mask_valid)
        ctx.mark_non_differentiable(scores)
        return fin, scores

    @staticmethod
    def backward(ctx, dfin, _dscores):
        gru_output, X_item, W, mask_ids, Wx, Uh, bx, q, scores, states = ctx.saved_tensors
        mode, padding_index, mask_valid = ctx.cfg
        H = X_item.shape[1]
        dg, dq, dWx, dUh, dbx = ops.dien_augru_bwd(gru_output, q, mask_ids, mode, Wx, Uh, bx, scores, states,
                                                   dfin.contiguous(), padding_index, mask_valid)
        dX_item = ops.gemm(dq, W)
        dW = ops.gemm(dq, X_item, transA=True)
        o = H if mode == ops.DIEN_AUGRU else 0               # the packed blocks: [z | r | h], AGRU [r | h]
        cell = (dWx[:, o:o + H], dUh[:, o:o + H], dbx[o:o + H], dWx[:, o + H:], dUh[:, o + H:], dbx[o + H:])
        if mode == ops.DIEN_AUGRU:
            cell = cell + (dWx[:, :H], dUh[:, :H], dbx[:H])
        else:
            cell = cell + (None, None, None)
        return (dg, dX_item, dW, None, None, None, None) + cell


class SimSearch(torch.autograd.Function):
    """SIM's soft search fused with the GSU pooling and the series lookup (7.SIM/CustomLayers.py:88-96, 236-260;
    csrc/sim.hip): ``embed`` [V,E], the candidate's rows ``q`` [B,D], ``series`` ids [B,T,C] -> (pooled [B,D], sel
    [B,K,D], sel_valid int32 [B,K], chosen int32 [B,K], scores [B,T]) with K = min(k, T); the last three carry no
    gradient.  One launch each way; the gradient that arrives through ``sel`` joins the pooling's in the one [B,T,D]
    buffer of IndexedSlices values, so ONE de-duplication plan serves the series.  ``sink``: as IpAttention's."""

    @staticmethod
    def forward(ctx, embed, q, series, padding_index, k, oob=None, sink=None):
        q = q.contiguous()
        K = min(int(k), series.shape[1])
        scores, pooled, chosen, sel, sel_valid = ops.sim_search_fwd(embed, series, q, padding_index, K, oob)
        ctx.save_for_backward(embed, q, series, scores, chosen)
        ctx.padding_index, ctx.sink = padding_index, sink
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(sel_valid, chosen, scores)
        return pooled, sel, sel_valid, chosen, scores

    @staticmethod
    def backward(ctx, gpooled, gsel, _gvalid, _gchosen, _gscores):
        embed, q, series, scores, chosen = ctx.saved_tensors
        V, E = embed.shape
        gpooled = torch.zeros_like(q) if gpooled is None else gpooled.contiguous()
        gsel = None if gsel is None else gsel.contiguous()
        buf, (dst,) = _sink_dsts(ctx.sink, E, embed.device, series)
        gkeys, gq = ops.sim_search_bwd(embed, series, q, ctx.padding_index, scores, gpooled, chosen, gsel, gkeys=dst)
        return _series_grad(ctx, series, gkeys, V, E, ctx.sink, buf), gq, None, None, None, None, None


class EsuAttention(torch.autograd.Function):
    """Keras MultiHeadAttention with one query over K dense keys (7.SIM/CustomLayers.py:159, 191-196; csrc/sim.hip):
    q [B,D], x [B,K,D] (keys and values), mask [B,K] (True / non-zero = attend; Keras' additive -1e9 in fp32), the
    kernels Wq, Wk, Wv [D,H,dk], Wo [H,dk,D] and their biases -> out [B,D].  One launch forward; the backward recomputes
    the forward's stages and sums the weight gradients over the batch in a fixed order."""

    @staticmethod
    def forward(ctx, q, x, mask, Wq, bq, Wk, bk, Wv, bv, Wo, bo):
        q, x = q.contiguous(), x.contiguous()
        mask = mask.to(torch.int32).contiguous()
        weights = tuple(w.contiguous() for w in (Wq, bq, Wk, bk, Wv, bv, Wo, bo))
        out, _ = ops.esu_attn_fwd(q, x, mask, weights)
        ctx.save_for_backward(q, x, mask, *weights)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, x, mask, *weights = ctx.saved_tensors
        grads = ops.esu_attn_bwd(q, x, mask, tuple(weights), gout.contiguous())
        return (grads[0], grads[1], None) + tuple(grads[2:])


class EtaSearch(torch.autograd.Function):
    """ETA's SimHash search fused with the series lookup (7.SIM/CustomLayers.py:556-571; csrc/eta.hip): ``embed`` [V,E],
    the candidate's rows ``q`` [B,D], ``series`` ids [B,T,C], the frozen projection ``Hm`` [D,m] -> (sel [B,K,D],
    sel_valid int32 [B,K], chosen int32 [B,K], scores int32 [B,T]) with K = min(k, T); the last three carry no gradient.
    One launch forward and none backward: ``sign`` has no gradient, so neither ``q`` nor ``Hm`` receives one, and the
    table's is the sparse row gradient of the B K C selected ids -- the [B,T,D] series is never written.  ``sink``: a
    GradSink of a Gather of the same table whose output feeds ``q``; the selected ids and their gradient rows are left
    there and ride that lookup's de-duplication plan.  With no gradient arriving through ``sel`` nothing is done."""

    @staticmethod
    def forward(ctx, embed, q, series, Hm, padding_index, k, oob=None, sink=None):
        q = q.contiguous()
        K = min(int(k), series.shape[1])
        scores, chosen, sel, sel_valid, sel_ids = ops.eta_search_fwd(embed, series, q, Hm.contiguous(), padding_index,
                                                                     K, oob)
        ctx.save_for_backward(sel_ids)
        ctx.shape, ctx.sink = tuple(embed.shape), sink
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(sel_valid, chosen, scores)
        return sel, sel_valid, chosen, scores

    @staticmethod
    def backward(ctx, gsel, _gvalid, _gchosen, _gscores):
        (sel_ids,) = ctx.saved_tensors
        V, E = ctx.shape
        none = (None,) * 8
        if gsel is None:
            return none
        gsel = gsel.contiguous()                             # row (b, j, c) of its [B K C, E] belongs to sel_ids[b, j, c]
        buf, (dst,) = _sink_dsts(ctx.sink, E, gsel.device, sel_ids)
        if dst is not None:
            dst.copy_(gsel)
        return (_series_grad(ctx, sel_ids, gsel, V, E, ctx.sink, buf),) + none[1:]


class SdimInterest(torch.autograd.Function):
    """SDIM's hash-bucket interest fused with the series lookup (8.DMR/CustomLayers.py:816-841; csrc/sdim.hip):
    ``embed`` [V,E], the candidates' rows ``q`` [B,S,D], ``series`` ids [B,T,C], the frozen projection ``Hm`` [D,G,m]
    -> (out [B,S,D], codes int32 [B,T], qcodes int32 [B,S], cnt int32 [B,S,G]); the last three carry no gradient.  One
    launch each way.  ``sign`` and ``one_hot`` have no gradient, so neither ``q`` nor ``Hm`` receives one; every step
    that collides with a candidate does, and the [B,T,D] IndexedSlices values are the only [B,T,D] tensor there ever is.
    ``mask_mode``: 'reference' sums the padded rows and counts every step, as the reference writes it; 'valid' sums and
    counts the valid ones.  ``sink``: a GradSink of a Gather of the same table whose output feeds ``q``; the series' ids
    and values are left there and ride that lookup's de-duplication plan.  With no gradient arriving nothing is done."""

    @staticmethod
    def forward(ctx, embed, q, series, Hm, padding_index, mask_mode="reference", oob=None, sink=None):
        if q.dim() == 3 and (q.stride(2) != 1 or (q.shape[1] > 1 and q.stride(0) != q.shape[1] * q.stride(1))):
            q = q.contiguous()                               # one candidate per example: a strided view is read in place
        out, codes, qcodes, cnt = ops.sdim_interest_fwd(embed, series, q, Hm.contiguous(), padding_index, mask_mode, oob)
        ctx.save_for_backward(series, codes, qcodes, cnt)
        ctx.shape, ctx.m, ctx.sink = tuple(embed.shape), Hm.shape[2], sink
        ctx.padding_index, ctx.mask_mode = padding_index, mask_mode
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(codes, qcodes, cnt)
        return out, codes, qcodes, cnt

    @staticmethod
    def backward(ctx, gout, _gcodes, _gqcodes, _gcnt):
        series, codes, qcodes, cnt = ctx.saved_tensors
        V, E = ctx.shape
        none = (None,) * 8
        if gout is None:
            return none
        buf, (dst,) = _sink_dsts(ctx.sink, E, series.device, series)
        gkeys = ops.sdim_interest_bwd(series, E, ctx.m, ctx.padding_index, codes, qcodes, cnt, gout.contiguous(),
                                      ctx.mask_mode, gkeys=dst)
        return (_series_grad(ctx, series, gkeys, V, E, ctx.sink, buf),) + none[1:]


def sim_loss(gsu_logits, esu_logits, label, alpha=0.2, beta=0.8):
    """The loss of SIM's train loop (7.SIM/ModelManager.py:173-180): tf.nn.softmax_cross_entropy_with_logits on the two
    heads' outputs -- which are softmax outputs already; the double softmax is the reference's and is kept -- weighted
    alpha, beta and summed over the batch.  ``label``: [B] 0/1 or one-hot [B,2].  Composed of torch ops."""
    if label.dim() == 1:
        label = torch.stack([1 - label, label], 1)
    label = label.to(gsu_logits.dtype)
    ce = lambda logits: -(label * torch.log_softmax(logits, -1)).sum(-1)
    return (alpha * ce(gsu_logits) + beta * ce(esu_logits)).sum()
