"""SDIMLayer (8.DMR/CustomLayers.py:772-955): target attention over the short-term series beside a hash-bucket interest
of the long one -- no search, no top-k (csrc/sdim.hip).  Like eta.ETALayer the class lives in a module of its
own.  Use ``from explicit_tf2_recommendation_amd.sdim import SDIMLayer``."""
import torch

from . import functional as Fn
from . import ops
from .eta import ETALayer, _ids_in_torch, _mlp_in_torch
from .layers import ConcatCols, Embedding, Layer, MultiHeadAttention, _initializer, _stack_ids, make_mlp_layer


def _candidate_ids(inputs, names, device):
    """the ids of the item features stacked on a last axis: [B], [B,1] or [B,S] each -> int64 [B,S,C] (torch alone)"""
    cols = []
    for name in names:
        t = torch.as_tensor(inputs[name]).to(device=device, dtype=torch.int64)
        if t.dim() not in (1, 2):
            raise ValueError("feature %r must have shape [B], [B,1] or [B,S], got %s" % (name, tuple(t.shape)))
        cols.append(t.reshape(t.shape[0], -1))
    if len({tuple(c.shape) for c in cols}) != 1:
        raise ValueError("the item features must agree in shape, got %s" % [tuple(c.shape) for c in cols])
    return torch.stack(cols, -1)


class SDIMLayer(Layer):
    """8.DMR/CustomLayers.py:772-955, sampling-based deep interest modelling: every step of the long behaviour series and
    every candidate gets G SimHash codes of m bits -- bit j is ``x H[:, j] > 0``, H a frozen random projection -- and a
    candidate's long-term interest is, per group, the mean of the steps whose code equals its own, averaged over the
    groups (``generate_longterm_interest`` with once=True; an empty bucket and a non-finite mean count as zero).  Beside
    it a multi-head attention of the candidate over the short-term series, the item rows and the tiled user rows feed
    make_mlp_layer([200, 80], sigmoid_units=True).  ``forward`` returns ``{'output': [B,S,1]}`` for S candidates per
    example (item features [B], [B,1] or [B,S]) and leaves ``inputs`` as it was.  ``H`` is the buffer
    ``projection_matrix`` [C E, lsh_group_num, lsh_group_length] ~ N(0, 0.05): saved, never trained.
    Not built: once=False, the reference's per-uid Python dict of bucket sums walked with ``.numpy()`` -- serving state
    (SURVEY 2).
    Extensions, after the reference's arguments: ``mask_mode`` -- 'reference' keeps the text as written: the long-term
    mask is ``ids == padding_index``, so the PADDED rows are summed and every step is counted, and the short-term
    attention reads the first count(valid) positions (wrong for left-padded series); 'valid' is the paper's intent: the
    valid steps are summed, counted and attended.  ``fused`` = True makes ONE Gather of the item, user and short-term ids
    and ONE interest launch over the long series (csrc/sdim.hip: the [B,T,D] series, the [B,T,G,m] projection, the
    one-hot and the bucket table are never written; the colliding steps' gradient rides the Gather's de-duplication
    plan); the one-query attention kernels of csrc/sim.hip run the short-term attention with one candidate and at most 16
    steps, MultiHeadAttention.composed otherwise.  False composes the layer of torch ops -- codes matched by equality, no
    2^m one-hot -- and on CPU tensors all of it is torch."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["label_goods_ids", "label_shop_ids", "label_cate_ids"],
                 longterm_series_features=["longterm_goods_ids", "longterm_shop_ids", "longterm_cate_ids"],
                 shortterm_series_features=["shortterm_goods_ids", "shortterm_shop_ids", "shortterm_cate_ids"],
                 feature_dims=160000, embedding_dims=16, padding_index=0, num_heads=8, key_dim=4, activation="ReLU",
                 lsh_group_num=4, lsh_group_length=3, mask_mode="reference", fused=True):
        super().__init__()
        assert len(item_categorical_features) == len(longterm_series_features) == len(shortterm_series_features)
        if mask_mode not in ops.SDIM_MODES:
            raise ValueError("mask_mode must be 'reference' or 'valid'")
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        self.longterm_series_features = longterm_series_features
        self.shortterm_series_features = shortterm_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.padding_index = padding_index
        self.lsh_group_num, self.lsh_group_length = lsh_group_num, lsh_group_length
        self.mask_mode, self.fused = mask_mode, fused
        C, U = len(item_categorical_features), len(user_and_context_categorical_features)
        D = C * embedding_dims
        if fused:
            ops.sdim_check_shape(D, G=lsh_group_num, m=lsh_group_length, C=C)
            ops.sim_check_shape(D, None, None, num_heads, key_dim)
        self.embed = Embedding(feature_dims, embedding_dims)
        self.register_buffer("projection_matrix", _initializer("random_normal")((D, lsh_group_num, lsh_group_length)))
        self.shortterm_mha = MultiHeadAttention(num_heads=num_heads, key_dim=key_dim, input_dim=D)
        # the reference also constructs a longterm_mha and never calls it: Keras builds no weights for it, so it is not here
        # Keras resolves the name 'ReLU' to relu
        self.final_mlp = make_mlp_layer([200, 80], activation="relu" if activation == "ReLU" else activation,
                                        sigmoid_units=True, input_dim=(C + U) * embedding_dims + 2 * D)

    @property
    def H(self):
        return self.projection_matrix

    _short_attend = ETALayer._short_attend
    _attend = ETALayer._attend

    def _shortterm_interest(self, q, x_short, attend, fused):
        """q [B,S,D] over x_short [B,n,D], attend bool [B,n] -> [B,S,D]"""
        if q.shape[1] == 1:
            return self._attend(self.shortterm_mha, q[:, 0], x_short, attend, fused).unsqueeze(1)
        return self.shortterm_mha.composed(q, x_short, attention_mask=attend.unsqueeze(1))

    def longterm_interest(self, X_item, X_long, pad):
        """the composed interest: X_item [B,S,D], X_long [B,T,D], pad bool [B,T] -> (interest [B,S,D], cnt [B,S,G])"""
        keys = torch.einsum("ble,egm->blgm", X_long, self.H) > 0
        cand = torch.einsum("bse,egm->bsgm", X_item, self.H) > 0
        match = (keys[:, None] == cand[:, :, None]).all(-1).to(X_long.dtype)               # [B,S,T,G]
        w = (pad if self.mask_mode == "reference" else ~pad).to(X_long.dtype)
        n = torch.ones_like(w) if self.mask_mode == "reference" else w
        total = torch.einsum("bslg,bld->bsgd", match * w[:, None, :, None], X_long)
        cnt = torch.einsum("bslg,bl->bsg", match, n)
        # a division by zero behind torch.where sends NaN back; the empty bucket is taken out before it
        mean = total / cnt.clamp(min=1).unsqueeze(-1)
        mean = torch.where(torch.isfinite(mean) & (cnt > 0).unsqueeze(-1), mean, torch.zeros_like(mean))
        return mean.mean(2), cnt

    def _forward_composed(self, inputs):
        table = self.embed.embeddings
        dev = table.device
        X_item = _candidate_ids(inputs, self.item_categorical_features, dev)
        X_user = _ids_in_torch(inputs, self.user_and_context_categorical_features, dev)
        stack = lambda cols: torch.stack(cols, -1)         # torch alone: this path runs on any device
        X_short = _stack_ids(inputs, self.shortterm_series_features, dev, stack)
        X_long = _stack_ids(inputs, self.longterm_series_features, dev, stack)
        B, S = X_item.shape[:2]
        if table.is_cuda:
            flag = ops.new_flag(dev) if self.check_ids else None
            lookup = lambda X: self.embed(X.contiguous(), flag)
        else:
            flag = None
            lookup = lambda X: table[X]                    # torch raises IndexError for an id out of range
        q, user = lookup(X_item).reshape(B, S, -1), lookup(X_user).reshape(B, 1, -1)
        x_short = lookup(X_short).reshape(B, X_short.shape[1], -1)
        x_long = lookup(X_long).reshape(B, X_long.shape[1], -1)
        self._raise_if_oob(flag)
        short_interest = self._shortterm_interest(q, x_short, self._short_attend(X_short[:, :, 0]), False)
        long_interest, _ = self.longterm_interest(q, x_long, X_long[:, :, 0] == self.padding_index)
        X_combined = torch.cat([q, user.expand(-1, S, -1), short_interest, long_interest], 2).reshape(B * S, -1)
        mlp = self.final_mlp if table.is_cuda else (lambda x: _mlp_in_torch(self.final_mlp, x))
        return {"output": mlp(X_combined).reshape(B, S, 1)}

    def forward(self, inputs):
        if not self.fused:
            return self._forward_composed(inputs)
        table = self.embed.embeddings
        if not table.is_cuda:
            raise RuntimeError("SDIMLayer(fused=True) runs HIP kernels and has no CPU fallback; move the layer to the "
                               "MI355X or build it with fused=False")
        dev = table.device
        X_item = _candidate_ids(inputs, self.item_categorical_features, dev)
        X_user = _ids_in_torch(inputs, self.user_and_context_categorical_features, dev)
        X_short = _stack_ids(inputs, self.shortterm_series_features, dev)
        X_long = _stack_ids(inputs, self.longterm_series_features, dev)
        (B, S, C), U, Ns, T = X_item.shape, X_user.shape[1], X_short.shape[1], X_long.shape[1]
        ops.sdim_check_shape(C * self.embedding_dims, T, S, self.lsh_group_num, self.lsh_group_length, C)
        X_all = torch.cat([X_item.reshape(B, S * C), X_user, X_short.reshape(B, Ns * C)], 1)
        flag = ops.new_flag(dev) if self.check_ids else None
        sink = self.embed.grad_sink(X_all)                   # the long series' rows ride this lookup's plan
        rows = self.embed(X_all, flag, sink)                 # [B, S C + U + Ns C, E]
        q = rows[:, :S * C].reshape(B, S, -1)
        x_short = rows[:, S * C + U:].reshape(B, Ns, -1)
        long_interest = Fn.SdimInterest.apply(table, q, X_long, self.H, self.padding_index, self.mask_mode, flag, sink)[0]
        self._raise_if_oob(flag)
        short_interest = self._shortterm_interest(q, x_short, self._short_attend(X_short[:, :, 0]), True)
        if S == 1:
            X_combined = ConcatCols.apply(rows[:, :C + U].reshape(B, -1), short_interest[:, 0], long_interest[:, 0])
        else:
            user = rows[:, S * C:S * C + U].reshape(B, 1, -1)
            X_combined = torch.cat([q, user.expand(-1, S, -1), short_interest, long_interest], 2).reshape(B * S, -1)
        return {"output": self.final_mlp(X_combined).reshape(B, S, 1)}
