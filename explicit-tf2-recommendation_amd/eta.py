"""ETALayer (7.SIM/CustomLayers.py:518-626): end-to-end target attention over a SimHash search of the long behaviour
series (csrc/eta.hip).  The class lives in this module, not in layers.py: tests/test_sim_host.py pins that
``layers`` has no ``ETALayer`` attribute.  Use ``from explicit_tf2_recommendation_amd.eta import ETALayer``."""
import math

import torch

from . import functional as Fn
from . import ops
from .layers import (Activation, ConcatCols, Dense, Dice, Embedding, Layer, LayerNormalization, MultiHeadAttention, PReLU,
                     _initializer, _stack_ids, assemble_index, make_mlp_layer)


def _ids_in_torch(inputs, names, device):
    """the ids of ``names`` stacked on a last axis with torch alone, on any device: [B] or [B,1] features -> [B,F]"""
    cols = []
    for name in names:
        t = torch.as_tensor(inputs[name]).to(device=device, dtype=torch.int64)
        if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] != 1):
            raise ValueError("feature %r must have shape [B] or [B,1], got %s" % (name, tuple(t.shape)))
        cols.append(t.reshape(-1))
    return torch.stack(cols, -1)


def _mlp_in_torch(mlp, x):
    """a make_mlp_layer Sequential on torch ops alone (any device): Dense, LayerNormalization, PReLU, Dice on its moving
    statistics and the named activations"""
    acts = {ops.DACT_NONE: lambda v: v, ops.DACT_RELU: torch.relu, ops.DACT_SIGMOID: torch.sigmoid,
            ops.DACT_TANH: torch.tanh}
    dense_acts = {ops.ACT_NONE: ops.DACT_NONE, ops.ACT_RELU: ops.DACT_RELU, ops.ACT_SIGMOID: ops.DACT_SIGMOID,
                  ops.ACT_TANH: ops.DACT_TANH}
    for l in mlp.layers:
        if isinstance(l, Dense):
            x = acts[dense_acts[l._act]](x @ l.kernel + l.bias)
        elif isinstance(l, LayerNormalization):
            x = torch.nn.functional.layer_norm(x, x.shape[-1:], l.gamma, l.beta, 1e-3)
        elif isinstance(l, PReLU):
            x = torch.relu(x) + l.alpha * torch.clamp(x, max=0.0)
        elif isinstance(l, Dice):
            p = torch.sigmoid((x - l.moving_mean) / torch.sqrt(l.moving_variance + l.epsilon))
            x = l.alpha * (1.0 - p) * x + p * x
        elif isinstance(l, Activation) and l.inner is None and l.kind in acts:
            x = acts[l.kind](x)
        else:
            raise NotImplementedError("no torch composition of %s" % type(l).__name__)
    return x


class ETALayer(Layer):
    """7.SIM/CustomLayers.py:518-626, end-to-end target attention: the long behaviour series is searched by the Hamming
    similarity of SimHash codes -- sign(x H) of every step against the candidate's, H a frozen random projection -- for
    its ``lsh_topk`` best steps (a padded step ranks as -inf, ties go to the lower index: tf.argsort's order; the
    reference's ``scores + mask * (-inf)`` is NaN for every valid step and its intent is kept), then one-query
    multi-head attentions of the candidate over those steps and over the short-term series feed, beside the item and
    user rows, make_mlp_layer([200, 80], sigmoid_units=True).  ``forward`` returns ``{'output': [B,1]}`` and leaves
    ``inputs`` as it was.  ``H`` is the buffer ``projection_matrix`` [C E, lsh_dim] ~ N(0, 0.05): saved, never trained.
    The long-term attention mask, sequence_mask(number of valid selections), equals the validity of the selections,
    because the order puts every valid selection before every padded one.
    Extensions, after the reference's arguments: ``mask_mode`` -- 'reference' attends the first count(valid) short-term
    positions, as written (wrong for left-padded series), 'valid' the valid ones.  ``fused`` = True makes ONE Gather of
    the item, user and short-term ids, ONE search launch over the long series (csrc/eta.hip: the [B,T,D] series is
    neither written nor given a gradient; the selected rows' gradient rides the Gather's de-duplication plan) and the
    one-query attention kernels of csrc/sim.hip, which stop at 16 keys: a longer short-term series runs
    MultiHeadAttention.composed for that attention alone.  False composes the layer of a gather, an einsum with H,
    torch.sign, an equality count, torch.sort(stable=True, descending=True), a gather and the composed attention; on
    CPU tensors all of it is torch."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["label_goods_ids", "label_shop_ids", "label_cate_ids"],
                 longterm_series_features=["longterm_goods_ids", "longterm_shop_ids", "longterm_cate_ids"],
                 shortterm_series_features=["shortterm_goods_ids", "shortterm_shop_ids", "shortterm_cate_ids"],
                 feature_dims=160000, embedding_dims=16, padding_index=0, num_heads=8, key_dim=4, activation="ReLU",
                 lsh_dim=16, lsh_topk=3, mask_mode="reference", fused=True):
        super().__init__()
        assert len(item_categorical_features) == len(longterm_series_features) == len(shortterm_series_features)
        if mask_mode not in ("reference", "valid"):
            raise ValueError("mask_mode must be 'reference' or 'valid'")
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        self.longterm_series_features = longterm_series_features
        self.shortterm_series_features = shortterm_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.padding_index = padding_index
        self.lsh_dim, self.lsh_topk = lsh_dim, lsh_topk
        self.mask_mode, self.fused = mask_mode, fused
        C, U = len(item_categorical_features), len(user_and_context_categorical_features)
        D = C * embedding_dims
        if fused:
            ops.eta_check_shape(D, m=lsh_dim, C=C)
            ops.sim_check_shape(D, None, None, num_heads, key_dim)
        self.embed = Embedding(feature_dims, embedding_dims)
        self.register_buffer("projection_matrix", _initializer("random_normal")((D, lsh_dim)))
        self.shortterm_mha = MultiHeadAttention(num_heads=num_heads, key_dim=key_dim, input_dim=D)
        self.longterm_mha = MultiHeadAttention(num_heads=num_heads, key_dim=key_dim, input_dim=D)
        # Keras resolves the name 'ReLU' to relu
        self.final_mlp = make_mlp_layer([200, 80], activation="relu" if activation == "ReLU" else activation,
                                        sigmoid_units=True, input_dim=(C + U) * embedding_dims + 2 * D)

    @property
    def H(self):
        return self.projection_matrix

    def _short_attend(self, short_ids0):
        """bool [B,S]: the short-term positions the attention reads"""
        valid = short_ids0 != self.padding_index
        if self.mask_mode == "valid":
            return valid
        steps = torch.arange(valid.shape[1], device=valid.device)
        return steps[None, :] < valid.sum(1, keepdim=True)

    def _attend(self, mha, q, x, attend, fused):
        if fused and x.shape[1] <= ops.SIM_MAX_K:
            return mha(q.unsqueeze(1), x, attention_mask=attend.unsqueeze(1), fused=True).squeeze(1)
        return mha.composed(q.unsqueeze(1), x, attention_mask=attend.unsqueeze(1)).squeeze(1)

    def lsh_search(self, X_item, X_long, valid):
        """the composed search: X_item [B,D], X_long [B,T,D], valid bool [B,T] -> (rows [B,K,D], their validity [B,K],
        positions [B,K], scores [B,T])"""
        series_codes = torch.sign(torch.einsum("ble,em->blm", X_long, self.H))
        item_codes = torch.sign(torch.einsum("be,em->bm", X_item, self.H))
        scores = (series_codes == item_codes.unsqueeze(1)).to(X_long.dtype).sum(-1)
        ranked = torch.where(valid, scores, torch.full_like(scores, -math.inf))
        order = torch.sort(ranked, dim=-1, descending=True, stable=True).indices[:, :self.lsh_topk]
        rows = torch.gather(X_long, 1, order.unsqueeze(-1).expand(-1, -1, X_long.shape[2]))
        return rows, torch.gather(valid, 1, order), order, scores

    def _forward_composed(self, inputs):
        table = self.embed.embeddings
        dev = table.device
        X_item = _ids_in_torch(inputs, self.item_categorical_features, dev)
        X_user = _ids_in_torch(inputs, self.user_and_context_categorical_features, dev)
        stack = lambda cols: torch.stack(cols, -1)         # torch alone: this path runs on any device
        X_short = _stack_ids(inputs, self.shortterm_series_features, dev, stack)
        X_long = _stack_ids(inputs, self.longterm_series_features, dev, stack)
        B = X_item.shape[0]
        if table.is_cuda:
            flag = ops.new_flag(dev) if self.check_ids else None
            lookup = lambda X: self.embed(X.contiguous(), flag)
        else:
            flag = None
            lookup = lambda X: table[X]                    # torch raises IndexError for an id out of range
        q, user = lookup(X_item).reshape(B, -1), lookup(X_user).reshape(B, -1)
        x_short = lookup(X_short).reshape(B, X_short.shape[1], -1)
        x_long = lookup(X_long).reshape(B, X_long.shape[1], -1)
        self._raise_if_oob(flag)
        sel, sel_valid, _, _ = self.lsh_search(q, x_long, X_long[:, :, 0] != self.padding_index)
        short_interest = self._attend(self.shortterm_mha, q, x_short, self._short_attend(X_short[:, :, 0]), False)
        long_interest = self._attend(self.longterm_mha, q, sel, sel_valid, False)
        X_combined = torch.cat([q, user, short_interest, long_interest], 1)
        mlp = self.final_mlp if table.is_cuda else (lambda x: _mlp_in_torch(self.final_mlp, x))
        return {"output": mlp(X_combined)}

    def forward(self, inputs):
        if not self.fused:
            return self._forward_composed(inputs)
        table = self.embed.embeddings
        if not table.is_cuda:
            raise RuntimeError("ETALayer(fused=True) runs HIP kernels and has no CPU fallback; move the layer to the "
                               "MI355X or build it with fused=False")
        X_item = assemble_index(inputs, self.item_categorical_features)
        X_user = assemble_index(inputs, self.user_and_context_categorical_features)
        dev = X_item.device
        X_short = _stack_ids(inputs, self.shortterm_series_features, dev)
        X_long = _stack_ids(inputs, self.longterm_series_features, dev)
        (B, C), U, S, T = X_item.shape, X_user.shape[1], X_short.shape[1], X_long.shape[1]
        ops.eta_check_shape(C * self.embedding_dims, T, min(self.lsh_topk, T), self.lsh_dim, C)
        X_all = torch.cat([X_item, X_user, X_short.reshape(B, S * C)], 1)
        flag = ops.new_flag(dev) if self.check_ids else None
        sink = self.embed.grad_sink(X_all)                   # the selected long-term rows ride this lookup's plan
        rows = self.embed(X_all, flag, sink)                 # [B, C + U + S C, E]
        q = rows[:, :C].reshape(B, -1)
        x_short = rows[:, C + U:].reshape(B, S, -1)
        sel, sel_valid, _, _ = Fn.EtaSearch.apply(table, q, X_long, self.H, self.padding_index, self.lsh_topk, flag, sink)
        self._raise_if_oob(flag)
        short_interest = self._attend(self.shortterm_mha, q, x_short, self._short_attend(X_short[:, :, 0]), True)
        long_interest = self._attend(self.longterm_mha, q, sel, sel_valid != 0, True)
        X_combined = ConcatCols.apply(rows[:, :C + U].reshape(B, -1), short_interest, long_interest)
        return {"output": self.final_mlp(X_combined)}
