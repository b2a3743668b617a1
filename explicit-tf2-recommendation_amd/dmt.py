"""DMT, Deep Multifaceted Transformers (8.DMR/CustomLayers.py:445-769): three behaviour series (click, cart, order) each
run a small Transformer -- an encoder stack over the series, a decoder whose one token is the candidate item -- and the
three interests feed an MMOE with two heads and two position-bias networks.  No kernel is new: on the GPU
the attentions run the one-query multi-head attention kernels of csrc/sim.hip -- a self-attention of T tokens is T
queries over the same T keys -- beside the LayerNorm, GEMM and lookup ops.  The classes live in a module of their own.
Use ``from explicit_tf2_recommendation_amd.dmt import DMTLayer``.

Parameters are named as Keras names them with '/' -> '.': ``mha._query_dense.kernel``, ``ffn.layers.0.kernel``,
``layernorm1.gamma``.

Two deviations from the reference, on purpose:
  dropout   random draws cannot be compared: ``dropout_rate`` / ``rate`` default to 0.0 here (reference 0.1), and a
            non-zero value raises NotImplementedError.
  heads     as written, ``ctr_output``, ``cvr_output`` and the bias MLP are make_mlp_layer([8, 1], ...): a
            LayerNormalization over a SINGLE feature follows the last Dense(1), and its output is ``beta`` whatever the
            input.  Both outputs are then constants (0.5 at initialisation) and no gradient reaches anything upstream.
            ``head='reference'`` (default) reproduces this: every upstream gradient is exactly zero or None.
            ``head='linear'`` (extension) ends each of the three heads with a plain Dense(1) after the hidden units, so the
            model can train.
"""
import torch

from . import functional as Fn
from . import ops
from .eta import _ids_in_torch
from .layers import (Activation, Dense, Embedding, Layer, LayerNormalization, MultiHeadAttention, PReLU, Sequential,
                     SoftmaxDense, _stack_ids, make_mlp_layer)

LN_EPSILON = 1e-6               # of every LayerNormalization inside the Transformer blocks
MAX_T = ops.SIM_MAX_K           # the series length the attention kernels cover: their keys are at most this many


def _check_series_length(T):
    if T > MAX_T:
        raise NotImplementedError("the fused DMT path covers a series length T <= %d (ops.SIM_MAX_K, the keys of the "
                                  "one-query attention kernel); got %d -- build the layer with fused=False" % (MAX_T, T))


def _no_dropout(rate, what):
    if rate != 0.0:
        raise NotImplementedError("%s: dropout is not built (random draws cannot be compared against the reference); "
                                  "pass 0.0, got %r" % (what, rate))


def _ln_torch(ln, x):
    """LayerNormalization composed of primitives: over a single feature autograd then sends exactly zero upstream, which
    torch's fused layer_norm backward (a polynomial in x) does not"""
    eps = 1e-3 if ln.epsilon is None else ln.epsilon
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + eps) * ln.gamma + ln.beta


def _mlp_torch(mlp, x):
    """a make_mlp_layer Sequential of this family on torch ops alone (any device)"""
    for l in mlp.layers:
        if isinstance(l, Dense):
            x = x @ l.kernel + l.bias
            if l._act == ops.ACT_RELU:
                x = torch.relu(x)
            elif l._act != ops.ACT_NONE:
                raise NotImplementedError("no torch composition of a Dense with activation code %d" % l._act)
        elif isinstance(l, LayerNormalization):
            x = _ln_torch(l, x)
        elif isinstance(l, PReLU):
            x = torch.relu(x) + l.alpha * torch.clamp(x, max=0.0)
        elif isinstance(l, Activation) and l.inner is None and l.kind == ops.DACT_RELU:
            x = torch.relu(x)
        elif isinstance(l, SoftmaxDense):
            x = torch.softmax(x @ l.dense.kernel + l.dense.bias, -1)
        else:
            raise NotImplementedError("no torch composition of %s" % type(l).__name__)
    return x


def _ffn(d_model, dff):
    return Sequential([Dense(dff, activation="relu", input_dim=d_model), Dense(d_model, input_dim=dff)])


class EncoderLayer(Layer):
    """8.DMR/CustomLayers.py:580-605: self-attention (Keras MultiHeadAttention(num_heads, key_dim=d_model)), residual +
    LayerNormalization(1e-6), Dense(dff, relu) -> Dense(d_model), residual + LayerNormalization(1e-6).
    ``forward(x [B,T,D], training, mask)``: ``mask`` [B,T] marks the valid tokens (True / non-zero); the attention mask
    is the pair mask m_t m_u the reference builds from it, applied additively as -1e9 in fp32, so a padded token attends
    uniformly over all T tokens and its row is real data.  ``fused`` and GPU tensors: every token is one query of
    functional.EsuAttention over the example's T rows (T <= MAX_T; a [B T, T, D] copy of the rows is made and given a
    gradient), then the LayerNorm and GEMM ops; otherwise ``composed``, torch ops alone.  Measured at B = 4096 with the
    reference's defaults: a stack of three takes 5.4 ms against 7.5 ms composed at T = 6 but 14.8 against
    10.4 ms at T = 16 -- an Encoder used alone near T = 16 is faster with fused=False; DeepInterestTransformer and
    DMTLayer as wholes are faster fused at both lengths."""

    def __init__(self, d_model, num_heads, dff, rate=0.0, fused=True):
        super().__init__()
        _no_dropout(rate, "EncoderLayer")
        self.d_model, self.num_heads, self.dff, self.fused = d_model, num_heads, dff, fused
        self.mha = MultiHeadAttention(num_heads, key_dim=d_model, input_dim=d_model)
        self.ffn = _ffn(d_model, dff)
        self.layernorm1 = LayerNormalization(d_model, epsilon=LN_EPSILON)
        self.layernorm2 = LayerNormalization(d_model, epsilon=LN_EPSILON)

    def composed(self, x, mask):
        m = (mask != 0).to(x.dtype)
        attn = self.mha.composed(x, x, attention_mask=m[:, :, None] * m[:, None, :])
        out1 = _ln_torch(self.layernorm1, x + attn)
        return _ln_torch(self.layernorm2, out1 + _mlp_torch(self.ffn, out1))

    def forward(self, x, training=False, mask=None):
        if x.dim() != 3:
            raise ValueError("EncoderLayer takes x [B,T,d_model], got %s" % (tuple(x.shape),))
        if mask is None:
            mask = torch.ones(x.shape[:2], dtype=torch.bool, device=x.device)
        if tuple(mask.shape) != tuple(x.shape[:2]):
            raise ValueError("mask must be [B,T] = %s (the valid tokens), got %s" % (tuple(x.shape[:2]), tuple(mask.shape)))
        if not (self.fused and x.is_cuda) or x.shape[0] == 0:   # an empty batch launches nothing either way
            return self.composed(x, mask)
        B, T, D = x.shape
        _check_series_length(T)
        ops.sim_check_shape(D, None, T, self.mha.num_heads, self.mha.key_dim)
        valid = mask != 0
        keys = x.unsqueeze(1).expand(B, T, T, D).reshape(B * T, T, D)
        pair = (valid[:, :, None] & valid[:, None, :]).reshape(B * T, T)
        x2 = x.reshape(B * T, D)
        attn = Fn.EsuAttention.apply(x2, keys, pair, *self.mha.weights())
        out1 = self.layernorm1(x2 + attn)
        return self.layernorm2(out1 + self.ffn(out1)).reshape(B, T, D)


class Encoder(Layer):
    """8.DMR/CustomLayers.py:608-620: ``num_layers`` EncoderLayers in a row (``enc_layers.{i}``)"""

    def __init__(self, num_layers, d_model, num_heads, dff, rate=0.0, fused=True):
        super().__init__()
        self.num_layers = num_layers
        self.enc_layers = torch.nn.ModuleList([EncoderLayer(d_model, num_heads, dff, rate, fused)
                                               for _ in range(num_layers)])

    def forward(self, x, training=False, mask=None):
        for layer in self.enc_layers:
            x = layer(x, training, mask)
        return x


class DecoderLayer(Layer):
    """8.DMR/CustomLayers.py:623-656 with ONE target token, the candidate item (the only way the reference calls it):
    ``mha1`` of the token over itself (one key: the output is (x Wv + bv) Wo + bo whatever the mask, and dWq = dWk = 0
    exactly), ``mha2`` of the result over the encoder's T rows, the feed-forward part, each behind a residual and a
    LayerNormalization(1e-6).  ``forward(x [B,1,D], enc_output [B,T,D], training, look_ahead_mask [B,1,1], padding_mask
    [B,1,T])``.  ``fused`` and GPU tensors: the one-query attention kernels of csrc/sim.hip (T <= 16) and the GEMM /
    LayerNorm ops; otherwise torch ops alone."""

    def __init__(self, d_model, num_heads, dff, rate=0.0, fused=True):
        super().__init__()
        _no_dropout(rate, "DecoderLayer")
        self.fused = fused
        self.mha1 = MultiHeadAttention(num_heads, key_dim=d_model, input_dim=d_model)
        self.mha2 = MultiHeadAttention(num_heads, key_dim=d_model, input_dim=d_model)
        self.ffn = _ffn(d_model, dff)
        self.layernorm1 = LayerNormalization(d_model, epsilon=LN_EPSILON)
        self.layernorm2 = LayerNormalization(d_model, epsilon=LN_EPSILON)
        self.layernorm3 = LayerNormalization(d_model, epsilon=LN_EPSILON)

    def forward(self, x, enc_output, training=False, look_ahead_mask=None, padding_mask=None):
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError("DecoderLayer takes one target token x [B,1,d_model], got %s" % (tuple(x.shape),))
        if not (self.fused and x.is_cuda) or x.shape[0] == 0:   # an empty batch launches nothing either way
            out1 = _ln_torch(self.layernorm1, self.mha1.composed(x, x, attention_mask=look_ahead_mask) + x)
            out2 = _ln_torch(self.layernorm2, self.mha2.composed(out1, enc_output, attention_mask=padding_mask) + out1)
            return _ln_torch(self.layernorm3, _mlp_torch(self.ffn, out2) + out2)
        out1 = self.layernorm1(self.mha1(x, x, attention_mask=look_ahead_mask)[:, 0] + x[:, 0])
        out2 = self.layernorm2(self.mha2(out1.unsqueeze(1), enc_output, attention_mask=padding_mask)[:, 0] + out1)
        return self.layernorm3(self.ffn(out2) + out2).unsqueeze(1)


class Decoder(Layer):
    """8.DMR/CustomLayers.py:659-671: ``num_layers`` DecoderLayers in a row (``dec_layers.{i}``)"""

    def __init__(self, num_layers, d_model, num_heads, dff, rate=0.0, fused=True):
        super().__init__()
        self.num_layers = num_layers
        self.dec_layers = torch.nn.ModuleList([DecoderLayer(d_model, num_heads, dff, rate, fused)
                                               for _ in range(num_layers)])

    def forward(self, x, enc_output, training=False, look_ahead_mask=None, padding_mask=None):
        for layer in self.dec_layers:
            x = layer(x, enc_output, training, look_ahead_mask, padding_mask)
        return x


class DeepInterestTransformer(Layer):
    """8.DMR/CustomLayers.py:674-726: the encoder over a behaviour series and the decoder whose one token is the candidate.
    ``forward(encoder_input [B,T] ids, decoder_input [B,1] ids, training, encoder_input_embedded [B,T,D],
    decoder_input_embedded [B,1,D])`` -> [B,1,D].  The masks are built as the reference builds them, from ``id != 0`` of
    the inputs (not from a padding_index): the encoder's pair mask m_t m_u, the decoder's look-ahead mask (1 x 1 band
    matrix times the candidate's validity) and its padding mask m_u m_candidate -- with a candidate id of 0 or a series
    padded throughout the decoder attends uniformly over all T encoder rows, padded ones included.
    ``shared_embedding_layer`` is used, never owned: its table is not a parameter of this module.
    ``fused`` (extension) = True runs the one-query attention kernels of csrc/sim.hip plus GEMM / LayerNorm ops for the
    encoder and the decoder; it covers T <= MAX_T (ops.SIM_MAX_K) and raises NotImplementedError naming the limit
    beyond.  False composes everything of torch ops, at any T and on any device."""

    def __init__(self, num_layers, d_model, num_heads, dff, input_vocab_size=None, rate=0.0, shared_embedding_layer=None,
                 fused=True):
        super().__init__()
        _no_dropout(rate, "DeepInterestTransformer")
        self.fused = fused
        if shared_embedding_layer is not None:
            self._shared = (shared_embedding_layer,)        # in a tuple: the owner registers it, not this module
        else:
            self._shared = None
            self.embedding = Embedding(input_vocab_size, d_model)
        if fused:
            ops.sim_check_shape(d_model, None, None, num_heads, d_model)
        self.encoder = Encoder(num_layers, d_model, num_heads, dff, rate, fused)
        self.decoder = Decoder(num_layers, d_model, num_heads, dff, rate, fused)

    def _lookup(self, ids):
        emb = self._shared[0] if self._shared is not None else self.embedding
        table = emb.embeddings
        ids = torch.as_tensor(ids).to(device=table.device, dtype=torch.int64)
        return emb(ids.contiguous()) if table.is_cuda else table[ids]

    @staticmethod
    def create_padding_mask(seq):
        return seq != 0

    def forward(self, encoder_input, decoder_input, training=False, encoder_input_embedded=None,
                decoder_input_embedded=None):
        x_enc = self._lookup(encoder_input) if encoder_input_embedded is None else encoder_input_embedded
        x_dec = self._lookup(decoder_input) if decoder_input_embedded is None else decoder_input_embedded
        dev = x_enc.device
        enc_valid = self.create_padding_mask(torch.as_tensor(encoder_input).to(dev))            # [B,T]
        dec_valid = self.create_padding_mask(torch.as_tensor(decoder_input).to(dev)).reshape(-1, 1)
        if self.fused and x_enc.is_cuda:
            _check_series_length(x_enc.shape[1])
        look_ahead = dec_valid[:, :, None]                                                      # [B,1,1]
        padding = enc_valid[:, None, :] & dec_valid[:, :, None]                                 # [B,1,T]
        enc_out = self.encoder(x_enc, training, enc_valid)
        return self.decoder(x_dec, enc_out, training, look_ahead, padding)


def _head(units, activation, input_dim, head):
    """make_mlp_layer(units, activation) as written ('reference'), or with a plain Dense in the place of the last unit's
    Dense, LayerNormalization and activation ('linear')"""
    if head == "reference":
        return make_mlp_layer(units, activation, input_dim=input_dim)
    hidden = make_mlp_layer(units[:-1], activation, input_dim=input_dim)
    last_in = units[-2] if len(units) > 1 else input_dim
    return Sequential(list(hidden.layers) + [Dense(units[-1], input_dim=last_in)])


def _keras_activation(name):
    return "relu" if name == "ReLU" else name              # Keras resolves the name 'ReLU' to relu


class BiasDeepNeuralNetworkLayer(Layer):
    """8.DMR/CustomLayers.py:729-769: the position, page and neighbourhood tables of its own; per neighbourhood feature
    the attention of the centre neighbour (index 3) over the ``neighbour_num`` neighbours, logits scaled by
    sqrt(embedding_dims); the attention weights, its outputs, the position row and the page row feed
    make_mlp_layer([8, 1], 'ReLU').  Composed of the lookup ops and torch: per example the attention is 2 x 7 rows of 16
    floats.  ``head`` as in DMTLayer."""

    def __init__(self, position_bias_features={"position_feature": "position", "page_feature": "page",
                                               "neighbourhood_features": ["near_expo_seq_cate2", "near_expo_seq_cate3"]},
                 feature_dims=160000, embedding_dims=16, max_position=400, max_page=100, neighbour_num=7,
                 head="reference"):
        super().__init__()
        if head not in ("reference", "linear"):
            raise ValueError("head must be 'reference' or 'linear', got %r" % (head,))
        if neighbour_num < 4:
            raise ValueError("the query is neighbour 3: neighbour_num must be at least 4, got %d" % neighbour_num)
        self.position_bias_features = position_bias_features
        self.neighbour_num, self.embedding_dims = neighbour_num, embedding_dims
        self.neighbourhood_embedding = Embedding(feature_dims, embedding_dims)
        self.position_embedding = Embedding(max_position, embedding_dims)
        self.page_embedding = Embedding(max_page, embedding_dims)
        F = len(position_bias_features["neighbourhood_features"])
        self.mlp = _head([8, 1], "relu", F * neighbour_num + F * embedding_dims + 2 * embedding_dims, head)

    def forward(self, inputs):
        f = self.position_bias_features
        dev = self.position_embedding.embeddings.device
        flag = ops.new_flag(dev) if (self.check_ids and dev.type == "cuda") else None

        def lookup(emb, ids):
            return emb(ids.contiguous(), flag) if dev.type == "cuda" else emb.embeddings[ids]

        B = torch.as_tensor(inputs[f["position_feature"]]).shape[0]
        X_position = lookup(self.position_embedding, _ids_in_torch(inputs, [f["position_feature"]], dev)).reshape(B, -1)
        X_page = lookup(self.page_embedding, _ids_in_torch(inputs, [f["page_feature"]], dev)).reshape(B, -1)
        nb = torch.stack([torch.as_tensor(inputs[n]).to(device=dev, dtype=torch.int64)
                          for n in f["neighbourhood_features"]], 1)                              # [B,F,N]
        if nb.dim() != 3 or nb.shape[2] != self.neighbour_num:
            raise ValueError("the neighbourhood features must be [B, %d], got %s" % (self.neighbour_num, tuple(nb.shape)))
        X_nb = lookup(self.neighbourhood_embedding, nb).reshape(B, nb.shape[1], self.neighbour_num, self.embedding_dims)
        self._raise_if_oob(flag)
        scores = torch.einsum("bhqe,bhke->bhqk", X_nb[:, :, 3:4, :], X_nb) / (self.embedding_dims ** 0.5)
        weights = torch.softmax(scores, -1)
        out = torch.einsum("bhqk,bhke->bhqe", weights, X_nb)
        result = torch.cat([weights.reshape(B, -1), out.reshape(B, -1), X_position, X_page], 1)
        return self.mlp(result) if dev.type == "cuda" else _mlp_torch(self.mlp, result)


class DMTLayer(Layer):
    """8.DMR/CustomLayers.py:445-577.  ``forward(inputs)`` takes the dict of features and returns ``{'ctr_logits',
    'cvr_logits'}`` ([B,1] each, after the sigmoid, as the reference names them) and leaves ``inputs`` as it was;
    ``set_stage(training)`` as in the reference (without dropout the stage changes nothing).
    ``tf_dim`` must equal ``len(item_categorical_features) * embedding_dims`` -- the reference fails at the residual add
    otherwise; here it is a ValueError at construction.
    Deviations (module docstring): ``dropout_rate`` defaults to 0.0 and a non-zero value raises NotImplementedError;
    ``head`` = 'reference' (default) keeps the degenerate [8, 1] heads as written -- constant outputs, exactly zero
    gradients upstream -- and 'linear' ends the three heads with a plain Dense(1).
    ``fused`` (extension) = True: every ``id_embed`` index of one forward -- the profile columns, the item columns and the
    three [B,T,C] series -- goes through ONE functional.Gather, so one de-duplication plan serves the table; the encoder
    stacks and the decoders run the one-query attention kernels (T <= MAX_T; NotImplementedError naming the limit
    beyond).  False composes the layer of torch ops, on any device.  The two bias networks
    keep their own tables."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 continuous_features=["continuous_feature1", "continuous_feature2", "continuous_feature3"],
                 click_series_features=["click_goods_ids", "click_shop_ids", "click_cate_ids"],
                 cart_series_features=["cart_goods_ids", "cart_shop_ids", "cart_cate_ids"],
                 order_series_features=["order_goods_ids", "order_shop_ids", "order_cate_ids"],
                 position_bias_features={"position_feature": "position", "page_feature": "page",
                                         "neighbourhood_features": ["near_expo_seq_cate2", "near_expo_seq_cate3"]},
                 feature_dims=160000, embedding_dims=16, training=True, tf_dim=48, tf_layers_num=3, tf_heads_num=4,
                 tf_dff=32, expert_units=[96, 32], expert_activation="PReLU", expert_num=6, gate_units=[64],
                 gate_activation="PReLU", output_units=[8, 1], output_activation="PReLU", dropout_rate=0.0,
                 max_position=400, max_page=100, neighbour_num=7, head="reference", fused=True):
        super().__init__()
        assert len(item_categorical_features) == len(click_series_features) == len(cart_series_features) \
            == len(order_series_features), "Features to be interacted should match in item and behavior series"
        _no_dropout(dropout_rate, "DMTLayer")
        if head not in ("reference", "linear"):
            raise ValueError("head must be 'reference' or 'linear', got %r" % (head,))
        C, U = len(item_categorical_features), len(user_and_context_categorical_features)
        if tf_dim != C * embedding_dims:
            raise ValueError("tf_dim must equal len(item_categorical_features) * embedding_dims = %d (the encoder adds "
                             "its input to its attention output), got %d" % (C * embedding_dims, tf_dim))
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        self.continuous_features = continuous_features
        self.click_series_features = click_series_features
        self.cart_series_features = cart_series_features
        self.order_series_features = order_series_features
        self.position_bias_features = position_bias_features
        self.feature_dims, self.embedding_dims = feature_dims, embedding_dims
        self.head, self.fused, self.training_stage = head, fused, training
        self.id_embed = Embedding(feature_dims, embedding_dims)
        make_tf = lambda: DeepInterestTransformer(num_layers=tf_layers_num, d_model=tf_dim, num_heads=tf_heads_num,
                                                  dff=tf_dff, rate=dropout_rate, shared_embedding_layer=self.id_embed,
                                                  fused=fused)
        self.click_transformer, self.cart_transformer, self.order_transformer = make_tf(), make_tf(), make_tf()
        self.expert_num = expert_num
        width = 3 * tf_dim + (U + C) * embedding_dims + len(continuous_features) + C * embedding_dims
        ea, ga, oa = (_keras_activation(a) for a in (expert_activation, gate_activation, output_activation))
        self.expert_model = torch.nn.ModuleList([make_mlp_layer(expert_units, ea, input_dim=width)
                                                 for _ in range(expert_num)])
        self.ctr_gate = make_mlp_layer(gate_units, ga, softmax_units=expert_num, input_dim=width)
        self.cvr_gate = make_mlp_layer(gate_units, ga, softmax_units=expert_num, input_dim=width)
        self.ctr_output = _head(output_units, oa, expert_num * expert_units[-1], head)
        self.cvr_output = _head(output_units, oa, expert_num * expert_units[-1], head)
        make_bias = lambda: BiasDeepNeuralNetworkLayer(position_bias_features=position_bias_features,
                                                       feature_dims=feature_dims, embedding_dims=embedding_dims,
                                                       max_position=max_position, max_page=max_page,
                                                       neighbour_num=neighbour_num, head=head)
        self.bias_network_ctr, self.bias_network_cvr = make_bias(), make_bias()

    def set_stage(self, training):
        self.training_stage = training

    def _series(self):
        return ((self.click_transformer, self.click_series_features), (self.cart_transformer, self.cart_series_features),
                (self.order_transformer, self.order_series_features))

    def forward(self, inputs):
        table = self.id_embed.embeddings
        dev = table.device
        on_gpu = table.is_cuda
        if self.fused and not on_gpu:
            raise RuntimeError("DMTLayer(fused=True) runs HIP kernels and has no CPU fallback; move the layer to the "
                               "MI355X or build it with fused=False")
        C, E = len(self.item_categorical_features), self.embedding_dims
        X_prof = _ids_in_torch(inputs, self.user_and_context_categorical_features + self.item_categorical_features, dev)
        B, UC = X_prof.shape
        stack = None if on_gpu else (lambda cols: torch.stack(cols, -1))
        X_ser = [_stack_ids(inputs, names, dev, stack) for _, names in self._series()]            # [B,T,C] each
        if self.fused:
            for X in X_ser:
                _check_series_length(X.shape[1])
        # one lookup of the table for everything: one de-duplication plan
        X_all = torch.cat([X_prof] + [X.reshape(B, -1) for X in X_ser], 1)
        flag = ops.new_flag(dev) if (self.check_ids and on_gpu) else None
        rows = self.id_embed(X_all.contiguous(), flag) if on_gpu else table[X_all]               # [B, n, E]
        self._raise_if_oob(flag)
        X_cate = rows[:, :UC].reshape(B, -1)
        X_item = rows[:, UC - C:UC].reshape(B, -1)
        X_cont = torch.stack([torch.as_tensor(inputs[n]).to(device=dev, dtype=torch.float32).reshape(B)
                              for n in self.continuous_features], 1)
        dec_ids = X_prof[:, UC - C].reshape(B, 1)                                                 # the first item feature
        interests, at = [], UC
        for (tf, _), X in zip(self._series(), X_ser):
            T = X.shape[1]
            x_enc = rows[:, at:at + T * C].reshape(B, T, C * E)
            at += T * C
            interests.append(tf(X[:, :, 0], dec_ids, self.training_stage, x_enc, X_item.unsqueeze(1))[:, 0])
        X = torch.cat(interests + [X_cate, X_cont, X_item], 1).contiguous()
        mlp = (lambda m, v: m(v)) if on_gpu else _mlp_torch
        experts = torch.stack([mlp(m, X) for m in self.expert_model], 1)                          # [B, experts, width]
        res = {}
        for task, gate, out, bias in (("ctr", self.ctr_gate, self.ctr_output, self.bias_network_ctr),
                                      ("cvr", self.cvr_gate, self.cvr_output, self.bias_network_cvr)):
            mixed = (experts * mlp(gate, X).unsqueeze(2)).reshape(B, -1).contiguous()
            res[task + "_logits"] = torch.sigmoid(mlp(out, mixed) + bias(inputs))
        return res
