"""Mirror of the reference's CustomLayers.py for the hot path -- same class names, constructor keywords,
dict-in / dict-out ``__call__`` and error behaviour -- with every op executed by the HIP kernels of
libmi355rec.so (through functional.py / ops.py).  Reference classes and the lines they follow:

  MLPLayer                      2.FM/CustomLayers.py:15-84   (default activation None; 'relu' in the 3.DCN/5.DIN copies)
  FMRankingLayer                2.FM/CustomLayers.py:87-157
  DSSMSingleTowerLayer          2.FM/CustomLayers.py:159-206
  DSSMTwoTowerRetrievalLayer    2.FM/CustomLayers.py:208-239
  DeepFMRankingLayer            2.FM/CustomLayers.py:241-308
  DenseLayer                    3.DCN/CustomLayers.py:153-167
  CrossLayer                    3.DCN/CustomLayers.py:170-203
  DeepCrossNetworkLayer         3.DCN/CustomLayers.py:206-269
  MatrixCrossLayer              3.DCN/CustomLayers.py:272-305
  XDeepFMRankingLayer           3.DCN/CustomLayers.py:308-374
  CINLayer                      3.DCN/CustomLayers.py:377-417
  FiBiNetLayer                  3.DCN/CustomLayers.py:888-956
  SENetLayer                    3.DCN/CustomLayers.py:959-981
  BilinearInteractionLayer      3.DCN/CustomLayers.py:984-1011
  TransformerAttentionLayer     3.DCN/CustomLayers.py:1012-1067
  AutoIntLayer                  3.DCN/CustomLayers.py:1070-1139
  InteractionLayer              3.DCN/CustomLayers.py:825-838
  AttentionLayer                3.DCN/CustomLayers.py:841-853
  AttentionalFactorizationMachine  3.DCN/CustomLayers.py:856-885
  KMaxPool                      3.DCN/CustomLayers.py:621-637
  CCPMBaseLayer                 3.DCN/CustomLayers.py:640-677
  CCPMLayer                     3.DCN/CustomLayers.py:680-725
  FGCNNBaseLayer                3.DCN/CustomLayers.py:728-772
  FGCNNLayer                    3.DCN/CustomLayers.py:775-822
  LayerNormInputFeaturesEmbeddingLayer  11.FiBiNet++/CustomLayers.py:245-311
  MaskBlockLayer                11.FiBiNet++/CustomLayers.py:314-337
  SerialMaskNetLayer            11.FiBiNet++/CustomLayers.py:340-364
  ParralledMaskNetLayer         11.FiBiNet++/CustomLayers.py:367-385
  MaskNetLayer                  11.FiBiNet++/CustomLayers.py:388-409
  ContextualEmbeddingLayer      11.FiBiNet++/CustomLayers.py:412-425
  NonLinearFeedforwardLayer     11.FiBiNet++/CustomLayers.py:428-446
  ContextNetBlockLayer          11.FiBiNet++/CustomLayers.py:449-471
  ContextNetLayer               11.FiBiNet++/CustomLayers.py:474-531
  NormInputFeaturesEmbeddingLayer  11.FiBiNet++/CustomLayers.py:78-145
  FiBiNetPlusLayer              11.FiBiNet++/CustomLayers.py:148-178
  SENetPlusLayer                11.FiBiNet++/CustomLayers.py:181-205
  BilinearInteractionPlusLayer  11.FiBiNet++/CustomLayers.py:208-242
  MMOELayer                     4.MMOE/CustomLayers.py:107-173
  ESMMLayer                     4.MMOE/CustomLayers.py:175-245
  PLELayer                      4.MMOE/CustomLayers.py:248-384
  GateNULayer                   10.POSO/CustomLayers.py:76-89
  PosoForMLPLayer               10.POSO/CustomLayers.py:92-119   (chain_layers=True: an extension, see the class)
  PEPNetLayer                   10.POSO/CustomLayers.py:371-462  (returns a tensor [B, tasks, units], as the reference)
  MultiInterestExtractorLayer   6.MIND/CustomLayers.py:62-138   (takes the table and the ids: the lookup is fused)
  LabelAwareAttention           6.MIND/CustomLayers.py:141-158  (with the inner products and the loss of :267-285)
  MINDLayer                     6.MIND/CustomLayers.py:161-285
  ComiRecDynamicRoutingLayer    6.MIND/CustomLayers.py:528-594  (takes the table and the ids, as the MIND extractor)
  ComiRecSelfAttentiveLayer     6.MIND/CustomLayers.py:597-665  (the same)
  ComiRecLayer                  6.MIND/CustomLayers.py:668-810  (negative_sample_type='manual')
  FinalMLPLayer                 8.DMR/CustomLayers.py:319-387
  FeatureSelectionLayer         8.DMR/CustomLayers.py:390-414
  DualPartsInteractionLayer     8.DMR/CustomLayers.py:416-442
  DienActivationLayer           5.DIN/CustomLayers.py:292-317
  CustomGRUCell                 5.DIN/CustomLayers.py:320-359
  DienGRU                       5.DIN/CustomLayers.py:362-386
  DIENLayer                     5.DIN/CustomLayers.py:389-517   (GRU: the Keras-named weights of tf.keras.layers.GRU)

Parameters are named after the TF checkpoint keys (``embed.embeddings``, ``w.embeddings``, ``bias``,
``MLP_layer1.kernel_0`` ...), so a TensorBundle checkpoint maps onto ``state_dict()`` by name.
Index tensors may be int64 ``[B,1]`` (ModelManager path) or ``[B]`` (direct layer call); out-of-range ids raise
IndexError when ``check_ids`` is on (the reference raises InvalidArgumentError on CPU).
"""
import math

import torch

from . import functional as Fn
from . import ops


# ---------------------------------------------------------------------------------------------------
# initialisers (Keras defaults)
# ---------------------------------------------------------------------------------------------------

_init_gen = torch.Generator(device="cpu")
_init_gen.manual_seed(1234)


def set_init_seed(seed):
    _init_gen.manual_seed(seed)


def _uniform(shape, lim):
    return (torch.rand(shape, generator=_init_gen) * 2 - 1) * lim


def glorot_uniform(shape):
    """TF2 glorot_uniform.  A convolution kernel [..., Cin, Cout] counts its receptive field: fan_in = rf Cin, fan_out =
    rf Cout with rf the product of the leading dims."""
    if len(shape) > 2:
        rf = math.prod(shape[:-2])
        fan_in, fan_out = rf * shape[-2], rf * shape[-1]
    else:
        fan_in, fan_out = (shape[0], shape[1]) if len(shape) == 2 else (shape[0], shape[0])
    return _uniform(shape, math.sqrt(6.0 / (fan_in + fan_out)))


def glorot_normal(shape):
    """TF2 glorot_normal: truncated normal at +-2 sigma, stddev sqrt(2 / (fan_in + fan_out)) / 0.87962566 (the stddev of
    a unit normal truncated at +-2), so that the draws have the untruncated variance."""
    fan_in, fan_out = (shape[-2], shape[-1]) if len(shape) >= 2 else (shape[0], shape[0])
    std = math.sqrt(2.0 / (fan_in + fan_out)) / 0.87962566103423978
    return torch.nn.init.trunc_normal_(torch.empty(shape), 0.0, std, -2.0 * std, 2.0 * std, generator=_init_gen)


def truncated_normal(shape, stddev=0.05):
    """TF2 tf.keras.initializers.TruncatedNormal() (mean 0, stddev 0.05): a normal of that stddev, values beyond 2
    stddev redrawn (no variance correction, unlike glorot_normal)."""
    return torch.nn.init.trunc_normal_(torch.empty(shape), 0.0, stddev, -2.0 * stddev, 2.0 * stddev, generator=_init_gen)


def _initializer(name):
    if callable(name):
        return name
    table = {"glorot_uniform": glorot_uniform, "glorot_normal": glorot_normal, "truncated_normal": truncated_normal,
             "zeros": lambda s: torch.zeros(s),
             "random_normal": lambda s: torch.randn(s, generator=_init_gen) * 0.05,
             "uniform": lambda s: _uniform(s, 0.05)}
    if name not in table:
        raise ValueError("Unknown initializer: %r" % (name,))
    return table[name]


def _activation_code(activation):
    if activation not in ops.ACT_CODE:
        raise ValueError("Unknown activation function: %r" % (activation,))
    return ops.ACT_CODE[activation]


class Layer(torch.nn.Module):
    """Keras-Layer conveniences on top of torch.nn.Module."""

    check_ids = True            # debug-mode bounds check: one 4-byte device->host read per call

    @property
    def trainable_variables(self):
        return [p for p in self.parameters() if p.requires_grad]

    def _device(self):
        for p in self.parameters():
            return p.device
        return torch.device("cuda")

    def _raise_if_oob(self, flag):
        if flag is not None and int(flag.item()) != 0:
            raise IndexError("embedding id out of range [0, feature_dims)")

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        post = getattr(self, "_post_apply", None)
        if post is not None:
            post()                  # e.g. re-establish the fused table layout after .cuda()/.to()
        return out


class _FMTables:
    """Mixin of the FM-family layers: keep ``embed.embeddings`` [V,E] and ``w.embeddings`` [V,1] as two strided
    views of ONE device array [V, ld] (row = [embed | w | pad], ld = next_pow2(E+1) >= 16) so that both values
    of an id arrive in the same 128-byte line.  The two Parameters keep their reference names and shapes
    (``state_dict``, ``copy_``, sparse gradients all work); only their strides change."""

    def fuse_tables(self):
        e, w = self.embed.embeddings, self.w.embeddings
        V, E = e.shape
        if not e.is_cuda or E % 4 != 0:
            return False
        ld = ops.fused_row_stride(E)
        if e.stride(0) == ld and w.stride(0) == ld and w.data_ptr() == e.data_ptr() + 4 * E:
            return True
        storage = torch.zeros((V, ld), dtype=torch.float32, device=e.device)
        storage[:, :E].copy_(e.data)
        storage[:, E:E + 1].copy_(w.data)
        self.embed.embeddings = torch.nn.Parameter(storage[:, :E], requires_grad=e.requires_grad)
        self.w.embeddings = torch.nn.Parameter(storage[:, E:E + 1], requires_grad=w.requires_grad)
        self._fused_storage = storage
        return True

    def _post_apply(self):
        self.fuse_tables()


def assemble_index(inputs, feature_names):
    """expand_dims(rank-1) + concat(axis=1)  (2.FM/CustomLayers.py:138-144) -> X [B,F] int64, on the GPU."""
    cols = []
    for name in feature_names:
        t = inputs[name]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        if t.dtype != torch.int64:
            t = t.to(torch.int64)
        if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] != 1):
            raise ValueError("feature %r must have shape [B] or [B,1], got %s" % (name, tuple(t.shape)))
        if not t.is_cuda:
            t = t.cuda()
        cols.append(t.contiguous())
    return ops.index_pack(cols)


class Embedding(Layer):
    """tf.keras.layers.Embedding(V, E): table ``embeddings`` ~ U(-0.05, 0.05)."""

    def __init__(self, input_dim, output_dim, embeddings_regularizer=None):
        super().__init__()
        # the "l2" regulariser of the reference lands in layer.losses, which its train loop never adds
        # (2.FM/ModelManager.py:175): kept for signature compatibility, no effect on gradients.
        self.embeddings_regularizer = embeddings_regularizer
        self.embeddings = torch.nn.Parameter(_uniform((input_dim, output_dim), 0.05))

    def forward(self, X, oob=None, sink=None):
        return Fn.Gather.apply(self.embeddings, X, oob, sink)

    def grad_sink(self, X):
        """A functional.GradSink for a second lookup of this table in the same step (None when no gradient is
        recorded)."""
        if torch.is_grad_enabled() and self.embeddings.requires_grad:
            return Fn.GradSink(X.numel())
        return None


def make_embedding(feature_dims, embedding_dims, sharded=False, group=None, comm=None, capacity=None,
                   embeddings_regularizer=None, device=None):
    """The table of a layer: layers.Embedding, or -- ``sharded=True`` -- sharded.ShardedEmbedding, its rows
    block-partitioned over the ranks of ``group`` (where the reference builds tf.keras.layers.Embedding,
    2.FM/CustomLayers.py:176-178, 3.DCN/CustomLayers.py:231, 5.DIN/CustomLayers.py:216-217).  Same call signature;
    the parameter is ``embeddings_shard`` [ceil(V/P), E] instead of ``embeddings`` [V, E]."""
    if not sharded:
        return Embedding(feature_dims, embedding_dims, embeddings_regularizer=embeddings_regularizer)
    from . import sharded as _sh
    return _sh.ShardedEmbedding(feature_dims, embedding_dims, group=group, comm=comm, capacity=capacity, device=device)


def _is_sharded(embed):
    return hasattr(embed, "embeddings_shard")


class MLPLayer(Layer):
    """MatMul + BiasAdd + activation on EVERY layer (2.FM/CustomLayers.py:72-84)."""

    def __init__(self, units, activation=None, use_bias=True, is_batch_norm=False, is_dropput=0,
                 kernel_initializer="glorot_uniform", bias_initializer="zeros", input_dim=None, **kwargs):
        super().__init__()
        self.units = [units] if not isinstance(units, list) else units
        if len(self.units) <= 0:
            raise ValueError("Received an invalid value for `units`, expected a positive integer, got %r." % (units,))
        self.is_batch_norm = bool(is_batch_norm)
        self.use_bias = use_bias
        self.is_dropout = is_dropput          # can never fire in the reference (is_train is never passed)
        self.activation = activation
        self._act = _activation_code(activation)
        self._kinit = _initializer(kernel_initializer)
        self._binit = _initializer(bias_initializer)
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, last_dim):
        dims = [int(last_dim)] + list(self.units)
        for i in range(len(dims) - 1):
            self.register_parameter("kernel_%d" % i, torch.nn.Parameter(self._kinit((dims[i], dims[i + 1]))))
            if self.use_bias:
                self.register_parameter("bias_%d" % i, torch.nn.Parameter(self._binit((dims[i + 1],))))
            if self.is_batch_norm:
                self.add_module("bn_%d" % i, BatchNormalization(input_dim=dims[i + 1]))
        self.built = True

    def forward(self, inputs, is_train=False):
        if not self.built:
            if inputs.shape[-1] is None:
                raise ValueError("The last dimension of the inputs to `Dense` should be defined. Found `None`.")
            self.build(inputs.shape[-1])
            self.to(inputs.device)
        x = inputs
        for i in range(len(self.units)):
            b = getattr(self, "bias_%d" % i) if self.use_bias else None
            if self.is_batch_norm:      # MatMul, BiasAdd, BatchNormalization, activation (2.FM/CustomLayers.py:74-81)
                x = Fn.LinearAct.apply(x, getattr(self, "kernel_%d" % i), b, ops.ACT_CODE[None])
                x = getattr(self, "bn_%d" % i)(x)
                if self.activation is not None:
                    x = Activation(self.activation)(x)
            else:
                x = Fn.LinearAct.apply(x, getattr(self, "kernel_%d" % i), b, self._act)
        return x


class FMRankingLayer(_FMTables, Layer):
    def __init__(self, feature_names=["item_tag1", "item_tag2", "item_tag3"], feature_dims=20, embedding_dims=16,
                 **kwargs):
        super().__init__()
        self.feature_names = feature_names
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.bias = torch.nn.Parameter(glorot_uniform((1,)))          # Keras default for a float weight
        self.embed = Embedding(feature_dims, embedding_dims, embeddings_regularizer="l2")
        self.w = Embedding(feature_dims, 1, embeddings_regularizer="l2")

    def forward(self, inputs):
        X = assemble_index(inputs, self.feature_names)
        flag = ops.new_flag(X.device) if self.check_ids else None
        z, _ = Fn.EmbFM.apply(self.embed.embeddings, self.w.embeddings, self.bias, X, False, flag)
        self._raise_if_oob(flag)
        output = Fn.Sigmoid.apply(z).reshape(-1, 1)
        return {"output": output}


class DeepFMRankingLayer(_FMTables, Layer):
    def __init__(self, feature_names=["user_tag0", "user_tag1", "item_tag1", "item_tag2", "item_tag3"],
                 feature_dims=20, embedding_dims=16, mlp_dims=[32, 8], **kwargs):
        super().__init__()
        self.feature_names = feature_names
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.mlp_dims = mlp_dims
        self.bias = torch.nn.Parameter(glorot_uniform((1,)))
        self.embed = Embedding(feature_dims, embedding_dims, embeddings_regularizer="l2")
        self.w = Embedding(feature_dims, 1, embeddings_regularizer="l2")
        self.MLP_layer1 = MLPLayer(units=list(mlp_dims), activation="relu",
                                   input_dim=len(feature_names) * embedding_dims)
        self.MLP_layer2 = MLPLayer(units=[1], input_dim=list(mlp_dims)[-1])

    def forward(self, inputs):
        X = assemble_index(inputs, self.feature_names)
        flag = ops.new_flag(X.device) if self.check_ids else None
        fm_part, rows = Fn.EmbFM.apply(self.embed.embeddings, self.w.embeddings, self.bias, X, True, flag)
        self._raise_if_oob(flag)
        dense_embedding = rows.reshape(rows.shape[0], -1)             # Flatten(): field-major, dim-minor
        dnn_part = self.MLP_layer2(self.MLP_layer1(dense_embedding))  # [B,1]
        return {"output": Fn.Sigmoid.apply(dnn_part, fm_part)}         # sigmoid(fm_part + dnn_part), [B,1]


class DSSMSingleTowerLayer(Layer):
    def __init__(self, feature_names=["item_tag1", "item_tag2", "item_tag3"], feature_dims=20, embedding_dims=8,
                 mlp_dims=[64, 32], final_dim=8, sharded=False, group=None, comm=None, capacity=None, **kwargs):
        super().__init__()
        self.feature_names = feature_names
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.mlp_dims = mlp_dims
        self.final_dim = final_dim
        # sharded=True: the table is row-sharded over the process group (BASELINE config D: 100M x 64d over 8 GPUs)
        self.embed = make_embedding(feature_dims, embedding_dims, sharded, group, comm, capacity, "l2")
        self.mlp = MLPLayer(units=list(mlp_dims), activation="relu", input_dim=len(feature_names) * embedding_dims)
        self.final = MLPLayer(units=[final_dim], activation=None, input_dim=list(mlp_dims)[-1])

    def forward(self, inputs):
        # the reference accepts [B,1] (model path) and, through an exception-driven reshape, [B] (direct call,
        # 2.FM/CustomLayers.py:188-194): both are handled explicitly here
        X = assemble_index(inputs, self.feature_names)
        flag = ops.new_flag(X.device) if self.check_ids else None
        e = self.embed(X, flag)
        self._raise_if_oob(flag)
        x = e.reshape(e.shape[0], -1)
        x = self.final(self.mlp(x))
        return {"user_id": inputs.get("user_id", None), "item_id": inputs.get("item_id", None), "output": x}


class DSSMTwoTowerRetrievalLayer(Layer):
    def __init__(self, u_feature_names=["user_tag1", "user_tag2"],
                 i_feature_names=["item_tag1", "item_tag2", "item_tag3"], u_feature_dims=20, i_feature_dims=20,
                 u_embedding_dims=8, i_embedding_dims=8, u_mlp_dims=[64, 32], i_mlp_dims=[64, 32], final_dim=8,
                 sharded=False, group=None, comm=None, u_capacity=None, i_capacity=None, **kwargs):
        super().__init__()
        # sharded: True (both towers' tables), or "u" / "i" / ("u", "i")
        which = ("u", "i") if sharded is True else ((sharded,) if isinstance(sharded, str) else tuple(sharded or ()))
        self.u_tower = DSSMSingleTowerLayer(feature_names=u_feature_names, feature_dims=u_feature_dims,
                                            embedding_dims=u_embedding_dims, mlp_dims=u_mlp_dims, final_dim=final_dim,
                                            sharded="u" in which, group=group, comm=comm, capacity=u_capacity)
        self.i_tower = DSSMSingleTowerLayer(feature_names=i_feature_names, feature_dims=i_feature_dims,
                                            embedding_dims=i_embedding_dims, mlp_dims=i_mlp_dims, final_dim=final_dim,
                                            sharded="i" in which, group=group, comm=comm, capacity=i_capacity)

    def forward(self, inputs):
        u_embedding = self.u_tower(inputs)["output"]
        i_embedding = self.i_tower(inputs)["output"]
        similarity = Fn.Cosine.apply(u_embedding, i_embedding)        # (1 - cos)/2, shape [B]
        return {"user_embedding": u_embedding, "item_embedding": i_embedding, "output": similarity}


# ---------------------------------------------------------------------------------------------------
# 3.DCN
# ---------------------------------------------------------------------------------------------------

class Dense(Layer):
    """tf.keras.layers.Dense(units, activation): ``kernel`` glorot-uniform, ``bias`` zeros."""

    def __init__(self, units, activation=None, input_dim=None):
        super().__init__()
        self.units = units
        self._act = _activation_code(activation)
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, last_dim):
        self.kernel = torch.nn.Parameter(glorot_uniform((int(last_dim), self.units)))
        self.bias = torch.nn.Parameter(torch.zeros(self.units))
        self.built = True

    def forward(self, x):
        if not self.built:
            self.build(x.shape[-1])
            self.to(x.device)
        return Fn.LinearAct.apply(x, self.kernel, self.bias, self._act)


class DenseLayer(Layer):
    def __init__(self, units, activation, input_dim=None):
        super().__init__()
        dims = [input_dim] + list(units)
        self.hidden_layer = torch.nn.ModuleList(
            [Dense(u, activation=activation, input_dim=dims[i]) for i, u in enumerate(units)])

    def forward(self, inputs, **kwargs):
        x = inputs
        for layer in self.hidden_layer:
            x = layer(x)
        return x


class _CrossBase(Layer):
    def __init__(self, layer_num, reg_w=1e-4, reg_b=1e-4, input_dim=None):
        super().__init__()
        self.layer_num = layer_num
        self.reg_w = reg_w          # l2 regularisers never reach the loss in the reference's loop
        self.reg_b = reg_b
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def _maybe_build(self, x):
        if not self.built:
            self.build(x.shape[1])
            self.to(x.device)


class CrossLayer(_CrossBase):
    """x_{l+1} = x0 * (x_l^T w_l) + b_l + x_l; w_l, b_l: [D,1] (w ~ N(0,0.05), b = 0)."""

    def build(self, D):
        for i in range(self.layer_num):
            self.register_parameter("w%d" % i, torch.nn.Parameter(torch.randn((D, 1), generator=_init_gen) * 0.05))
            self.register_parameter("b%d" % i, torch.nn.Parameter(torch.zeros((D, 1))))
        self.built = True

    def forward(self, inputs, **kwargs):
        self._maybe_build(inputs)
        w = torch.cat([getattr(self, "w%d" % i).reshape(1, -1) for i in range(self.layer_num)], dim=0)
        b = torch.cat([getattr(self, "b%d" % i).reshape(1, -1) for i in range(self.layer_num)], dim=0)
        return Fn.CrossVec.apply(inputs, w, b)


class MatrixCrossLayer(_CrossBase):
    """x_{l+1} = x0 (.) (W_l x_l + b_l) + x_l; W_l: [D,D] ~ N(0,0.05), b_l: [D,1] = 0."""

    def build(self, D):
        for i in range(self.layer_num):
            self.register_parameter("w%d" % i, torch.nn.Parameter(torch.randn((D, D), generator=_init_gen) * 0.05))
            self.register_parameter("b%d" % i, torch.nn.Parameter(torch.zeros((D, 1))))
        self.built = True

    def forward(self, inputs, **kwargs):
        self._maybe_build(inputs)
        W = torch.stack([getattr(self, "w%d" % i) for i in range(self.layer_num)], dim=0)
        b = torch.cat([getattr(self, "b%d" % i).reshape(1, -1) for i in range(self.layer_num)], dim=0)
        return Fn.CrossMat.apply(inputs, W, b)


class ConcatCols(torch.autograd.Function):
    """tf.concat(axis=1) of 2-D fp32 blocks, by column-block copies."""

    @staticmethod
    def forward(ctx, *blocks):
        widths = [b.shape[1] for b in blocks]
        out = torch.empty((blocks[0].shape[0], sum(widths)), dtype=torch.float32, device=blocks[0].device)
        c = 0
        for b, w in zip(blocks, widths):
            ops.copy_cols(b.contiguous(), out[:, c:c + w])
            c += w
        ctx.widths = widths
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        outs = []
        c = 0
        for i, w in enumerate(ctx.widths):
            if ctx.needs_input_grad[i]:                  # input features (the continuous columns) need no gradient
                blk = torch.empty((g.shape[0], w), dtype=torch.float32, device=g.device)
                ops.copy_cols(g[:, c:c + w], blk)
                outs.append(blk)
            else:
                outs.append(None)
            c += w
        return tuple(outs)


def _cont_block(inputs, names, device):
    cols = []
    for n in names:
        t = inputs[n]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        t = t.to(device=device, dtype=torch.float32)
        if t.dim() == 1:
            t = t.unsqueeze(1)
        cols.append(t.contiguous())
    if len(cols) > 1:                                     # one [B, n_cont] block: one copy into the concatenation
        return [torch.cat(cols, dim=1)]
    return cols


class DeepCrossNetworkLayer(Layer):
    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=16, units=[64, 8], activation="relu", layer_num=3, reg_w=1e-4, reg_b=1e-4,
                 type="vec", sharded=False, group=None, comm=None, capacity=None):
        super().__init__()
        D = len(continuous_features) + len(categorical_features) * embedding_dims
        if type == "vec":
            self.cross_layer = CrossLayer(layer_num, reg_w, reg_b, input_dim=D)
        else:
            self.cross_layer = MatrixCrossLayer(layer_num, reg_w, reg_b, input_dim=D)
        self.dense_layer = DenseLayer(units, activation, input_dim=D)
        self.embedding_layer = make_embedding(feature_dims, embedding_dims, sharded, group, comm, capacity)
        self.categorical_features = categorical_features
        self.continuous_features = continuous_features
        self.output_layer = Dense(1, activation="sigmoid", input_dim=D + list(units)[-1])

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        X_emb = self.embedding_layer(X, flag)
        self._raise_if_oob(flag)
        X_flatten = X_emb.reshape(X_emb.shape[0], -1)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        _input = ConcatCols.apply(*cont, X_flatten)                   # continuous FIRST (:259)
        cross_output = self.cross_layer(_input)
        dnn_output = self.dense_layer(_input)
        combine_output = ConcatCols.apply(cross_output, dnn_output)
        return {"output": self.output_layer(combine_output)}


class CINLayer(Layer):
    """Compressed Interaction Network (3.DCN/CustomLayers.py:377-417): weights ``w0..w{L-1}`` of the reference's shape
    (1, F*H_k, H_{k+1}) (H_0 = F), glorot-uniform, no bias, no activation.  Built from the first input's field count
    (or ``input_dim=F``); forward and backward are the fp32-MFMA kernels of csrc/cin.hip.  The l1_l2 regulariser of the
    reference never reaches its loss and is not applied."""

    def __init__(self, cin_size=[8, 16], input_dim=None):
        super().__init__()
        self.cin_size = [int(h) for h in cin_size]
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, F):
        F = int(F)
        self.field_num = [F] + self.cin_size
        for i in range(len(self.cin_size)):
            a, b = self.field_num[0] * self.field_num[i], self.field_num[i + 1]
            self.register_parameter("w%d" % i, torch.nn.Parameter(_uniform((1, a, b), math.sqrt(6.0 / (a + b)))))
        self.built = True

    def forward(self, inputs, **kwargs):
        if not self.built:
            self.build(inputs.shape[1])
            self.to(inputs.device)
        ops.cin_check_shape(inputs.shape[1], inputs.shape[2], self.cin_size)
        return Fn.CIN.apply(inputs, *[getattr(self, "w%d" % i) for i in range(len(self.cin_size))])


class XDeepFMRankingLayer(Layer):
    """3.DCN/CustomLayers.py:308-374: output = Dense(1, sigmoid)(concat[linear_part, dense_part, cin_part]) with
    linear_part = sum_f w[X_f], dense_part = DenseLayer(units, activation)(concat[X_cont, Flatten(X0)]) and
    cin_part = CINLayer(cin_size)(X0), X0 = embedding_layer(X_cate).  The "l2" / l1_l2 regularisers are kept for the
    signature and never reach the loss (3.DCN/ModelManager.py trains on the BCE alone)."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=16, units=[64, 8], activation="relu", cin_size=[16, 32, 64]):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        F = len(self.categorical_features)
        ops.cin_check_shape(F, embedding_dims, cin_size)
        self.w = Embedding(feature_dims, 1, embeddings_regularizer="l2")
        self.dense_layer = DenseLayer(units, activation, input_dim=len(self.continuous_features) + F * embedding_dims)
        self.embedding_layer = Embedding(feature_dims, embedding_dims)
        self.cin_layer = CINLayer(cin_size, input_dim=F)
        self.output_layer = Dense(1, activation="sigmoid", input_dim=1 + list(units)[-1] + sum(cin_size))
        # linear_part = w_rows [B,F] . ones [F,1] on the GEMM kernel (reduce_sum over the fields)
        self.register_buffer("_field_ones", torch.ones((F, 1)), persistent=False)

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        B, F = X.shape
        flag = ops.new_flag(X.device) if self.check_ids else None
        w_rows = self.w(X, flag)                                        # [B,F,1]
        X_emb = self.embedding_layer(X, flag)                           # [B,F,E]
        self._raise_if_oob(flag)
        linear_part = Fn.LinearAct.apply(w_rows.reshape(B, F), self._field_ones, None, ops.ACT_NONE)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        dense_input = ConcatCols.apply(*cont, X_emb.reshape(B, -1))     # continuous FIRST (:357)
        dense_part = self.dense_layer(dense_input)
        cin_part = self.cin_layer(X_emb)
        output = self.output_layer(ConcatCols.apply(linear_part, dense_part, cin_part))
        return {"output": output}


class SENetLayer(Layer):
    """3.DCN/CustomLayers.py:959-981: A = excitation(mean_e inputs), excitation = MLPLayer([mid, F], 'relu',
    use_bias=False) with mid = max(1, F // reduction_ratio) (``excitation.kernel_0`` [F,mid], ``excitation.kernel_1``
    [mid,F], glorot-uniform).  Its forward runs fused with the bilinear interaction inside FiBiNetLayer
    (csrc/fibinet.hip); there is no separate kernel for it."""

    def __init__(self, reduction_ratio=3, input_dim=None):
        super().__init__()
        self.reduction_ratio = reduction_ratio
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, field_num):
        self.field_num = int(field_num)
        self.mid_unit_num = max(1, self.field_num // self.reduction_ratio)
        self.excitation = MLPLayer([self.mid_unit_num, self.field_num], activation="relu", use_bias=False,
                                   input_dim=self.field_num)
        self.built = True

    def forward(self, inputs):
        raise NotImplementedError("SENetLayer runs fused inside FiBiNetLayer (csrc/fibinet.hip)")


class BilinearInteractionLayer(Layer):
    """3.DCN/CustomLayers.py:984-1011: p_ij = (v_i W_ij) * v_j over the pairs i < j (itertools.combinations order),
    W_ij = ``bilinear_weight`` ('all'), ``bilinear_weight{i}`` ('each'), ``bilinear_weight{i}_{j}`` ('interaction'),
    each [E,E], TF2 glorot_normal.  The Parameters are views of one packed [nW,E,E] array, so that the kernel takes a
    single pointer (re-packed after .to() / .cuda(); if outside code replaces one, ``packed_weight`` stacks them).
    Its forward runs fused with SENet inside FiBiNetLayer (csrc/fibinet.hip)."""

    def __init__(self, bilinear_type="interaction", input_shape=None):
        super().__init__()
        self.bilinear_type = bilinear_type
        self.built = False
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        F, E = int(input_shape[-2]), int(input_shape[-1])
        self.field_num, self.embedding_size = F, E
        pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
        if self.bilinear_type == "all":
            self._w_names = ["bilinear_weight"]
        elif self.bilinear_type == "each":
            self._w_names = ["bilinear_weight%d" % i for i in range(F - 1)]
        elif self.bilinear_type == "interaction":
            self._w_names = ["bilinear_weight%d_%d" % p for p in pairs]
        else:
            raise NotImplementedError
        self.type_code = ops.FIBINET_TYPES[self.bilinear_type]
        packed = torch.stack([glorot_normal((E, E)) for _ in self._w_names])
        self._pack_into(packed)
        self.built = True

    def _pack_into(self, packed):
        self._packed = packed
        for k, n in enumerate(self._w_names):
            old = getattr(self, n, None)
            self.register_parameter(n, torch.nn.Parameter(packed[k], requires_grad=True if old is None
                                                          else old.requires_grad))

    def weights(self):
        return [getattr(self, n) for n in self._w_names]

    def _is_packed(self):
        ws = self.weights()
        E = self.embedding_size
        st, off = ws[0].untyped_storage().data_ptr(), ws[0].storage_offset()
        return all(w.is_contiguous() and w.device == ws[0].device and w.untyped_storage().data_ptr() == st
                   and w.storage_offset() == off + E * E * k for k, w in enumerate(ws))

    def packed_weight(self, ws):
        """W [nW,E,E] for the kernel: a view of the packed array, or one torch.stack if the packing was broken."""
        if len(ws) and self._is_packed():
            return torch.as_strided(ws[0], (len(ws),) + tuple(ws[0].shape), (ws[0].numel(),) + tuple(ws[0].stride()))
        return torch.stack(list(ws))

    def _post_apply(self):
        if not self.built or self._is_packed():
            return
        ws = self.weights()
        packed = torch.stack([w.data for w in ws])
        self._pack_into(packed)

    def forward(self, inputs):
        raise NotImplementedError("BilinearInteractionLayer runs fused inside FiBiNetLayer (csrc/fibinet.hip)")


class FiBiNetLayer(Layer):
    """3.DCN/CustomLayers.py:888-956: output = Dense(1, sigmoid)(dnn_layer(concat[Flatten(concat[Bilinear(X_emb),
    Bilinear(SENet(X_emb))]), X_cont])), X_emb = embedding_layer(X_cate), dnn_layer = MLPLayer(units, activation).
    The SENet, both bilinear passes and the concatenation are one kernel each way (functional.FiBiNetInteraction);
    the MLP runs on the GEMM kernels."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=16, units=[128, 16], activation="relu", bilinear_type="interaction", reduction_ratio=3):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        self.bilinear_type = bilinear_type
        F, C, E = len(self.categorical_features), len(self.continuous_features), int(embedding_dims)
        ops.fibinet_check_shape(F, E, C, max(1, F // reduction_ratio))
        P = F * (F - 1) // 2
        self.embedding_layer = Embedding(feature_dims, E)
        self.dnn_layer = MLPLayer(list(units), activation=activation, input_dim=2 * P * E + C)
        self.output_layer = Dense(1, activation="sigmoid", input_dim=list(units)[-1])
        self.SENet = SENetLayer(reduction_ratio=reduction_ratio, input_dim=F)
        self.Bilinear = BilinearInteractionLayer(bilinear_type=bilinear_type, input_shape=(F, E))

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        X_emb = self.embedding_layer(X, flag)                           # [B,F,E]
        self._raise_if_oob(flag)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        x_cont = cont[0] if cont else torch.empty((X.shape[0], 0), dtype=torch.float32, device=X.device)
        ex = self.SENet.excitation
        dnn_input = Fn.FiBiNetInteraction.apply(X_emb, x_cont, ex.kernel_0, ex.kernel_1, self.Bilinear.type_code,
                                                self.Bilinear.packed_weight, *self.Bilinear.weights())
        return {"output": self.output_layer(self.dnn_layer(dnn_input))}


class TransformerAttentionLayer(Layer):
    """3.DCN/CustomLayers.py:1012-1067: multi-head self-attention over the fields, ``query``, ``key``, ``value`` (and
    ``res`` when use_res and res_learnable) [E,E], TF2 TruncatedNormal().  Head h owns the columns [h d, (h+1) d),
    d = E / num_heads.  The reference's softmax runs over axis 1 of (H, B, F, F), the BATCH axis, so every example's
    output depends on the whole batch; this port keeps that.  One kernel pair per layer (functional.AutoIntAttention,
    csrc/autoint.hip)."""

    def __init__(self, num_heads=2, use_res=True, res_learnable=False, scaling=False, input_dim=None):
        super().__init__()
        self.num_heads = num_heads
        self.use_res = use_res
        self.scaling = scaling
        self.res_learnable = res_learnable
        self.res_code = ops.AUTOINT_RES[(bool(use_res), bool(res_learnable))]
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, input_shape):
        E = int(input_shape[-1]) if isinstance(input_shape, (tuple, list, torch.Size)) else int(input_shape)
        self.embedding_dim = E
        self.att_embedding_size = E // self.num_heads
        if E % self.num_heads != 0:
            raise ValueError("embedding_dim %d is not divisible by num_heads %d" % (E, self.num_heads))
        self.query = torch.nn.Parameter(truncated_normal((E, E)))
        self.key = torch.nn.Parameter(truncated_normal((E, E)))
        self.value = torch.nn.Parameter(truncated_normal((E, E)))
        if self.use_res and self.res_learnable:
            self.res = torch.nn.Parameter(truncated_normal((E, E)))
        self.built = True

    def attend(self, x, x_cont=None, cemb=None):
        """x [B,Fc,E] (+ continuous fields cemb[c] * x_cont[:, c] appended last) -> [B,F,E]."""
        if not self.built:
            self.build(x.shape[-1])
            self.to(x.device)
        return Fn.AutoIntAttention.apply(x, x_cont, cemb, self.query, self.key, self.value,
                                         getattr(self, "res", None), self.num_heads, self.res_code, bool(self.scaling))

    def forward(self, inputs):
        return self.attend(inputs)


class AutoIntLayer(Layer):
    """3.DCN/CustomLayers.py:1070-1139: X_emb = concat[embedding_layer(X_cate), continuous_embedding.embeddings *
    x_cont[..., None]] (continuous fields last), attention_layer_num TransformerAttentionLayers, Flatten, dnn_layer =
    MLPLayer(units, activation), output_layer = Dense(1, sigmoid).  The continuous fields are assembled inside the first
    attention layer's kernels; the MLP runs on the GEMM kernels."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=8, units=[128, 16], activation="relu", attention_layer_num=2, num_heads=2):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        Fc, C, E = len(self.categorical_features), len(self.continuous_features), int(embedding_dims)
        ops.autoint_check_shape(Fc + C, E, int(num_heads), C)
        if Fc < 1 or (C > 0 and attention_layer_num < 1):
            raise NotImplementedError("AutoIntLayer needs a categorical feature, and an attention layer to assemble "
                                      "the continuous fields in")
        self.embedding_dims = E
        self.embedding_layer = Embedding(feature_dims, E)
        self.continuous_embedding = Embedding(C, E)
        self.attention_layers = torch.nn.ModuleList(
            [TransformerAttentionLayer(num_heads=num_heads, input_dim=E) for _ in range(attention_layer_num)])
        self.dnn_layer = MLPLayer(list(units), activation=activation, input_dim=(Fc + C) * E)
        self.output_layer = Dense(1, activation="sigmoid", input_dim=list(units)[-1])

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        att = self.embedding_layer(X, flag)                              # [B,Fc,E]
        self._raise_if_oob(flag)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        x_cont = cont[0] if cont else None
        cemb = self.continuous_embedding.embeddings if cont else None
        for k, layer in enumerate(self.attention_layers):
            att = layer.attend(att, x_cont, cemb) if k == 0 else layer.attend(att)
        dnn_input = att.reshape(att.shape[0], -1)                        # Flatten: field-major [B, F*E] (a view)
        return {"output": self.output_layer(self.dnn_layer(dnn_input))}


class InteractionLayer(Layer):
    """3.DCN/CustomLayers.py:825-838: the F(F-1)/2 products e_i * e_j, i < j, i outer and j inner.  It has no weights;
    its forward runs fused with the lookup and the attention inside AttentionalFactorizationMachine (csrc/afm.hip)."""

    def forward(self, inputs):
        raise NotImplementedError("InteractionLayer runs fused inside AttentionalFactorizationMachine (csrc/afm.hip)")


class AttentionLayer(Layer):
    """3.DCN/CustomLayers.py:841-853: ``attention_w`` = Dense(attn_size, relu), ``attention_h`` = Dense(1), a softmax
    over the pair axis and the weighted sum of the pairs.  Its forward runs fused inside
    AttentionalFactorizationMachine (csrc/afm.hip); there is no separate kernel for it."""

    def __init__(self, attn_size, input_dim=None):
        super().__init__()
        self.attn_size = int(attn_size)
        self.attention_w = Dense(self.attn_size, activation="relu")
        self.attention_h = Dense(1, activation=None, input_dim=self.attn_size)
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, embedding_dims):
        self.attention_w.build(int(embedding_dims))
        self.built = True

    def forward(self, inputs):
        raise NotImplementedError("AttentionLayer runs fused inside AttentionalFactorizationMachine (csrc/afm.hip)")


class AttentionalFactorizationMachine(Layer):
    """3.DCN/CustomLayers.py:856-885: output = MLPLayer([1], sigmoid)(attention_layer(interaction_layer(
    embedding_layer(X)))).  Categorical features only.  The lookup, the pairwise products, the attention and the pooling
    are one kernel each way (functional.EmbAFM); the [E,1] head runs on the GEMM kernels."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 feature_dims=150000, embedding_dims=16, attn_size=3):
        super().__init__()
        self.categorical_features = list(categorical_features)
        F, E = len(self.categorical_features), int(embedding_dims)
        ops.afm_check_shape(F, E, int(attn_size))
        self.embedding_dims = E
        self.interaction_layer = InteractionLayer()
        self.attention_layer = AttentionLayer(attn_size=attn_size, input_dim=E)
        self.embedding_layer = Embedding(feature_dims, E, embeddings_regularizer="l2")
        self.output_layer = MLPLayer(units=[1], activation="sigmoid", input_dim=E)

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        att = self.attention_layer
        attention_output = Fn.EmbAFM.apply(self.embedding_layer.embeddings, X, att.attention_w.kernel,
                                           att.attention_w.bias, att.attention_h.kernel, att.attention_h.bias, flag)
        self._raise_if_oob(flag)
        return {"output": self.output_layer(attention_output)}


class KMaxPool(Layer):
    """3.DCN/CustomLayers.py:621-637: per (embedding dim, channel) the k largest values over the field axis, in
    DESCENDING order of value (tf.nn.top_k(sorted=True), not the field order of the paper), the lower field first on
    equal values.  It has no weights; its forward runs fused inside CCPMLayer (csrc/ccpm.hip)."""

    def __init__(self, k):
        super().__init__()
        self.k = int(k)

    def forward(self, inputs):
        raise NotImplementedError("KMaxPool runs fused inside CCPMLayer (csrc/ccpm.hip)")


class _FieldConv(Layer):
    """The parameters of Conv2D(filters, (kernel_width, 1), padding='same', activation='tanh'): ``kernel``
    [kw,1,Cin,Cout] glorot-uniform, ``bias`` [Cout] zeros."""

    def __init__(self, kernel_width, cin, cout):
        super().__init__()
        self.kernel = torch.nn.Parameter(glorot_uniform((int(kernel_width), 1, int(cin), int(cout))))
        self.bias = torch.nn.Parameter(torch.zeros(int(cout)))

    def forward(self, inputs):
        raise NotImplementedError("the field convolution runs fused inside CCPMLayer (csrc/ccpm.hip) and FGCNNLayer "
                                  "(csrc/fgcnn.hip)")


def _field_convs(filters, kernel_width):
    """The ``conv_layers`` of CCPMBaseLayer and FGCNNBaseLayer: layer i reads the channels of layer i - 1, the first one
    a single channel."""
    cins = [1] + list(filters[:-1])
    return torch.nn.ModuleList([_FieldConv(kw, cin, c) for kw, cin, c in zip(kernel_width, cins, filters)])


def _field_conv_weights(conv_layers):
    """K_1, b_1, K_2, b_2, ...: the order of the kernels' flat params."""
    return [w for c in conv_layers for w in (c.kernel, c.bias)]


class CCPMBaseLayer(Layer):
    """3.DCN/CustomLayers.py:640-677: L x (Conv2D along the field axis, tanh, KMaxPool) and Flatten.  ``build`` takes
    the input shape (fields, embedding_dims); the k of every pooling comes from ``input_shape[-1]``, the embedding
    width, as in the reference (ops.ccpm_k).  Holds ``conv_layers.{i}.kernel`` / ``.bias``; its forward runs fused with
    the lookup inside CCPMLayer (csrc/ccpm.hip)."""

    def __init__(self, filters=[4, 6], kernel_width=[4, 2], input_shape=None):
        super().__init__()
        self.filters = [int(c) for c in filters]
        self.kernel_width = [int(k) for k in kernel_width]
        self.layers_num = len(self.filters)
        self.built = False
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        F, E = int(input_shape[-2]), int(input_shape[-1])
        self.pool_k = ops.ccpm_check_shape(F, E, self.filters, self.kernel_width)
        self.conv_layers = _field_convs(self.filters, self.kernel_width)
        self.kmax_layers = torch.nn.ModuleList([KMaxPool(k) for k in self.pool_k])
        self.output_dim = self.pool_k[-1] * E * self.filters[-1]
        self.built = True

    def weights(self):
        return _field_conv_weights(self.conv_layers)

    def forward(self, inputs):
        raise NotImplementedError("CCPMBaseLayer runs fused with the lookup inside CCPMLayer (csrc/ccpm.hip)")


class CCPMLayer(Layer):
    """3.DCN/CustomLayers.py:680-725: output = MLP_layer2([1], sigmoid)(MLP_layer1(units, activation, batch norm)(
    concat[ccpm_layer(embedding_layer(X_cate)), X_cont])), the continuous columns LAST.  The lookup, the convolutions,
    the poolings and the Flatten are one kernel each way (functional.EmbCCPM); the MLPs run on the GEMM kernels."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=150000,
                 embedding_dims=16, units=[64, 32, 8], activation="relu", is_batch_norm=True, filters=[4, 6],
                 kernel_width=[4, 2]):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        self.units = list(units)
        self.activation = activation
        F, C, E = len(self.categorical_features), len(self.continuous_features), int(embedding_dims)
        self.ccpm_layer = CCPMBaseLayer(filters, kernel_width, input_shape=(F, E))
        self.MLP_layer1 = MLPLayer(units=self.units, activation=activation, is_batch_norm=is_batch_norm,
                                   input_dim=self.ccpm_layer.output_dim + C)
        self.MLP_layer2 = MLPLayer(units=[1], activation="sigmoid", input_dim=self.units[-1])
        self.embedding_layer = Embedding(feature_dims, E, embeddings_regularizer="l2")

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        base = self.ccpm_layer
        ccpm_output = Fn.EmbCCPM.apply(self.embedding_layer.embeddings, X, base.filters, base.kernel_width, flag,
                                       *base.weights())
        self._raise_if_oob(flag)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        _input = ConcatCols.apply(ccpm_output, *cont) if cont else ccpm_output       # continuous LAST (:720)
        return {"output": self.MLP_layer2(self.MLP_layer1(_input))}


class FGCNNBaseLayer(Layer):
    """3.DCN/CustomLayers.py:728-772: L x (Conv2D along the field axis, tanh, MaxPool2D((pooling_width, 1))), and after
    every pooling a Dense "recombination" of its Flatten, reshaped to [N_j, E]; the output is their concat along the
    field axis, [B, sum N_j, E].  ``build`` takes the input shape (fields, embedding_dims).  As in the reference every
    Dense has dnn_maps x fields x embedding_dims // pooling_width units, from the ORIGINAL field count and not from the
    height its layer pools (ops.fgcnn_dense_units).  Holds ``conv_layers.{i}.kernel`` / ``.bias`` and
    ``dense_layers.{i}.kernel`` / ``.bias``.  The convolutions and poolings run fused with the lookup inside FGCNNLayer
    (csrc/fgcnn.hip); ``recombine`` is the part after them, on the GEMM kernels."""

    def __init__(self, filters=[14, 16], kernel_width=[7, 7], dnn_maps=[3, 3], pooling_width=[2, 2], input_shape=None):
        super().__init__()
        self.filters = [int(c) for c in filters]
        self.kernel_width = [int(k) for k in kernel_width]
        self.dnn_maps = [int(m) for m in dnn_maps]
        self.pooling_width = [int(w) for w in pooling_width]
        self.built = False
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        F, E = int(input_shape[-2]), int(input_shape[-1])
        self.heights = ops.fgcnn_check_shape(F, E, self.filters, self.kernel_width, self.pooling_width, self.dnn_maps)
        self.dense_units = ops.fgcnn_dense_units(F, E, self.dnn_maps, self.pooling_width)
        self.new_fields = [u // E for u in self.dense_units]
        self.conv_layers = _field_convs(self.filters, self.kernel_width)
        self.dense_layers = torch.nn.ModuleList(
            [Dense(u, input_dim=h * E * c) for u, h, c in zip(self.dense_units, self.heights, self.filters)])
        self.output_dim = sum(self.dense_units)
        self.built = True

    def weights(self):
        return _field_conv_weights(self.conv_layers)

    def recombine(self, pooled):
        """[p_1 .. p_L] -> [d_1 .. d_L], d_j = Dense_j(p_j) [B, N_j E]: row-major, the reshape to [N_j, E] and the
        Flatten that follows the concat leave the bytes where they are."""
        return [dense(p) for dense, p in zip(self.dense_layers, pooled)]

    def forward(self, inputs):
        raise NotImplementedError("FGCNNBaseLayer's convolutions run fused with the lookup inside FGCNNLayer "
                                  "(csrc/fgcnn.hip)")


class FGCNNLayer(Layer):
    """3.DCN/CustomLayers.py:775-822: output = MLP_layer2([1], sigmoid)(MLP_layer1(units, activation, batch norm)(
    concat[Flatten(concat[X_emb, fgcnn_layer(X_emb)], axis=1), X_cont])): the embeddings first, then every layer's
    recombined maps in order, the continuous columns LAST.  The lookup, the convolutions and the poolings are one kernel
    each way (functional.EmbFGCNN); the recombinations and the MLPs run on the GEMM kernels."""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=150000,
                 embedding_dims=16, units=[64, 8], activation="relu", is_batch_norm=True, filters=[14, 16],
                 kernel_width=[7, 7], dnn_maps=[3, 3], pooling_width=[2, 2]):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        self.units = list(units)
        self.activation = activation
        F, C, E = len(self.categorical_features), len(self.continuous_features), int(embedding_dims)
        self.fgcnn_layer = FGCNNBaseLayer(filters, kernel_width, dnn_maps, pooling_width, input_shape=(F, E))
        self.MLP_layer1 = MLPLayer(units=self.units, activation=activation, is_batch_norm=is_batch_norm,
                                   input_dim=F * E + self.fgcnn_layer.output_dim + C)
        self.MLP_layer2 = MLPLayer(units=[1], activation="sigmoid", input_dim=self.units[-1])
        self.embedding_layer = Embedding(feature_dims, E, embeddings_regularizer="l2")

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        base = self.fgcnn_layer
        rows, *pooled = Fn.EmbFGCNN.apply(self.embedding_layer.embeddings, X, base.filters, base.kernel_width,
                                          base.pooling_width, flag, *base.weights())
        self._raise_if_oob(flag)
        cont = _cont_block(inputs, self.continuous_features, X.device)
        _input = ConcatCols.apply(rows.reshape(rows.shape[0], -1), *base.recombine(pooled), *cont)   # :815-817
        return {"output": self.MLP_layer2(self.MLP_layer1(_input))}


# ---------------------------------------------------------------------------------------------------
# 11.FiBiNet++: MaskNet
# ---------------------------------------------------------------------------------------------------

_MASKNET_CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
_MASKNET_CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


class LayerNormInputFeaturesEmbeddingLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:245-311.  Categorical ids and the ``<c>_key`` ids of the continuous features index
    ONE table; the row of a continuous feature is scaled by its ``<c>_value``; every field then passes its own
    LayerNormalization (``emb_layernorm_list.{f}.gamma`` / ``.beta``).  Returns (X_emb_normed, X_emb), both [B, F, E],
    from one kernel each way (functional.EmbFieldLayerNorm)."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features_keys = [name + "_key" for name in continuous_features]
        self.continuous_features_values = [name + "_value" for name in continuous_features]
        self.fields_num = len(self.categorical_features) + len(self.continuous_features_keys)
        self.embedding_dims = int(embedding_dims)
        ops.masknet_ln_check_shape(self.fields_num, self.embedding_dims, len(self.continuous_features_keys))
        self.embedding_layer = Embedding(feature_dims, self.embedding_dims)
        self.emb_layernorm_list = torch.nn.ModuleList(
            [LayerNormalization(self.embedding_dims) for _ in range(self.fields_num)])

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features + self.continuous_features_keys)
        values = None
        if self.continuous_features_values:
            values = _cont_block(inputs, self.continuous_features_values, X.device)[0]
        flag = ops.new_flag(X.device) if self.check_ids else None
        gamma = torch.stack([ln.gamma for ln in self.emb_layernorm_list])
        beta = torch.stack([ln.beta for ln in self.emb_layernorm_list])
        x_emb, x_norm = Fn.EmbFieldLayerNorm.apply(self.embedding_layer.embeddings, X, values, gamma, beta, flag)
        self._raise_if_oob(flag)
        shape = (X.shape[0], self.fields_num, self.embedding_dims)
        return x_norm.reshape(shape), x_emb.reshape(shape)


def make_instance_guided_mask(output_dim, reduction_rate=3, input_dim=None):
    """11.FiBiNet++/CustomLayers.py:314-319: Dense(output_dim * reduction_rate), ReLU, Dense(output_dim).  ``input_dim``
    (extension) is needed because layers are built eagerly."""
    if input_dim is None:
        raise ValueError("make_instance_guided_mask needs input_dim")
    hidden = int(output_dim) * int(reduction_rate)
    return Sequential([Dense(hidden, input_dim=input_dim), Activation("relu"), Dense(int(output_dim), input_dim=hidden)])


class MaskBlockLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:322-337: output = ln_hid(v * instance_guided_mask(X_emb)) for inputs (v, X_emb), both
    2-D; ln_hid is Dense(block_output_dim), LayerNormalization, ReLU.  v is the normalised embeddings
    (``input_type='feature'``, width fields_num * embedding_dims) or the previous block's output (``'block'``, width
    block_output_dim).  The sub-layers hold the parameters (``instance_guided_mask.layers.{0,2}.kernel`` / ``.bias``,
    ``ln_hid.layers.0.kernel`` / ``.bias``, ``ln_hid.layers.1.gamma`` / ``.beta``); the call runs them as one kernel
    each way (functional.MaskBlock)."""

    def __init__(self, fields_num=13, input_type="feature", embedding_dims=16, block_output_dim=32):
        super().__init__()
        self.input_type = input_type
        D, O = int(fields_num) * int(embedding_dims), int(block_output_dim)
        P = D if input_type == "feature" else O
        ops.mask_block_check_shape(D, P, O, 3)
        self.instance_guided_mask = make_instance_guided_mask(P, input_dim=D)
        self.ln_hid = make_mlp_layer([O], activation="relu", normalization="layernorm", input_dim=P)

    def forward(self, inputs, sink=None):
        v, x_emb = inputs
        d1, _, d2 = self.instance_guided_mask.layers
        d3, ln, _ = self.ln_hid.layers
        return Fn.MaskBlock.apply(x_emb, v, d1.kernel, d1.bias, d2.kernel, d2.bias, d3.kernel, d3.bias, ln.gamma, ln.beta,
                                  sink)


class _MaskNetBase(Layer):
    def __init__(self, categorical_features, continuous_features, feature_dims, embedding_dims, block_output_dim,
                 block_num):
        super().__init__()
        if int(block_num) < 1:
            raise ValueError("block_num must be at least 1, got %r" % (block_num,))
        self.norm_embedding_layer = LayerNormInputFeaturesEmbeddingLayer(categorical_features, continuous_features,
                                                                         feature_dims, embedding_dims)
        self.embedding_dims = int(embedding_dims)
        self.fields_num = self.norm_embedding_layer.fields_num
        self.block_output_dim, self.block_num = int(block_output_dim), int(block_num)

    def _block(self, input_type):
        return MaskBlockLayer(fields_num=self.fields_num, input_type=input_type, embedding_dims=self.embedding_dims,
                              block_output_dim=self.block_output_dim)

    def _flat_inputs(self, inputs):
        x_norm, x_emb = self.norm_embedding_layer(inputs)
        D = self.embedding_dims * self.fields_num
        sink = Fn.MaskDxSink(self.block_num) if torch.is_grad_enabled() else None
        return x_norm.reshape(-1, D), x_emb.reshape(-1, D), sink


class SerialMaskNetLayer(_MaskNetBase):
    """11.FiBiNet++/CustomLayers.py:340-364: one 'feature' block on the flattened (X_emb_normed, X_emb), then
    block_num - 1 'block' blocks, each fed the previous output and guided by the same X_emb -> [B, block_output_dim]."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16, block_output_dim=32, block_num=6):
        super().__init__(categorical_features, continuous_features, feature_dims, embedding_dims, block_output_dim,
                         block_num)
        self.mask_block_on_feature = self._block("feature")
        self.mask_block_on_block_list = torch.nn.ModuleList([self._block("block") for _ in range(self.block_num - 1)])
        self.output_dim = self.block_output_dim

    def forward(self, inputs):
        x_norm, x_emb, sink = self._flat_inputs(inputs)
        x = self.mask_block_on_feature((x_norm, x_emb), sink)
        for block in self.mask_block_on_block_list:
            x = block((x, x_emb), sink)
        return x


class ParralledMaskNetLayer(_MaskNetBase):
    """11.FiBiNet++/CustomLayers.py:367-385 (the reference's spelling): block_num 'feature' blocks on the same inputs,
    concatenated -> [B, block_num * block_output_dim].  As written the reference passes the [B, F, E] tensors on without
    the flatten its serial sibling applies, and [B, F, E] * [B, F, F E] raises for F > 1; this class applies that
    flatten.  That is a reading of the intent, NOT reference behaviour."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16, block_output_dim=32, block_num=6):
        super().__init__(categorical_features, continuous_features, feature_dims, embedding_dims, block_output_dim,
                         block_num)
        self.mask_block_on_feature_list = torch.nn.ModuleList([self._block("feature") for _ in range(self.block_num)])
        self.output_dim = self.block_num * self.block_output_dim

    def forward(self, inputs):
        x_norm, x_emb, sink = self._flat_inputs(inputs)
        return ConcatCols.apply(*[block((x_norm, x_emb), sink) for block in self.mask_block_on_feature_list])


class MaskNetLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:388-409: output = final_mlp(mask_net(inputs)) with final_mlp = Dense, PReLU per unit
    of final_mlp_units, then Dense(1, sigmoid) -> {'output': [B, 1]}.  ``inputs`` carries the categorical ids, and per
    continuous feature c the id ``c + '_key'`` and the float ``c + '_value'``."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16, block_output_dim=32, block_num=6, stacking_mode="serial", final_mlp_units=[32]):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features_keys = [name + "_key" for name in continuous_features]
        self.continuous_features_values = [name + "_value" for name in continuous_features]
        self.stacking_mode = stacking_mode
        net = SerialMaskNetLayer if stacking_mode == "serial" else ParralledMaskNetLayer
        self.mask_net = net(categorical_features, continuous_features, feature_dims, embedding_dims, block_output_dim,
                            block_num)
        self.final_mlp = make_mlp_layer(list(final_mlp_units), sigmoid_units=True, normalization="None",
                                        input_dim=self.mask_net.output_dim)

    def forward(self, inputs):
        return {"output": self.final_mlp(self.mask_net(inputs))}


# ---------------------------------------------------------------------------------------------------
# 11.FiBiNet++: ContextNet
# ---------------------------------------------------------------------------------------------------

class ContextualEmbeddingLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:412-425: mask = reshape(contextual_embedding_transform(flatten(inputs))) with the
    transform make_instance_guided_mask(fields_num * embedding_dims).  It holds the parameters
    (``contextual_embedding_transform.layers.{0,2}.kernel`` / ``.bias``); ContextNetBlockLayer runs them inside its one
    kernel, and a direct call composes the same Dense layers."""

    def __init__(self, fields_num=13, embedding_dims=16):
        super().__init__()
        D = int(fields_num) * int(embedding_dims)
        self.contextual_embedding_transform = make_instance_guided_mask(D, input_dim=D)

    def forward(self, inputs):
        return self.contextual_embedding_transform(inputs.reshape(inputs.shape[0], -1)).reshape(inputs.shape)


class NonLinearFeedforwardLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:428-446: ln(relu(x W1) W2 + x) in 'pointwise' mode, ln(x W1) in any other; W1, W2
    [E,E] TF2 glorot_normal, W2 only in pointwise mode; ``ln.gamma`` / ``ln.beta``.  It holds one field's parameters;
    ContextNetBlockLayer runs all fields inside its one kernel; a direct call composes the same arithmetic from the GEMM,
    activation and LayerNorm kernels."""

    def __init__(self, embedding_dims=16, mode="pointwise"):
        super().__init__()
        E = int(embedding_dims)
        self.W1 = torch.nn.Parameter(glorot_normal((E, E)))
        self.ln = LayerNormalization(E)
        self.mode = mode
        if mode == "pointwise":
            self.W2 = torch.nn.Parameter(glorot_normal((E, E)))

    def forward(self, inputs):
        out = Fn.LinearAct.apply(inputs, self.W1, None, ops.ACT_NONE)
        if self.mode == "pointwise":
            out = Fn.LinearAct.apply(Fn.FeatAct.apply(out, ops.DACT_RELU, None, None, None), self.W2, None,
                                     ops.ACT_NONE) + inputs
        return self.ln(out)


class ContextNetBlockLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:449-471: mask = ce_layer(x); per field f, nonlinear_layer_list[f](x_f * mask_f);
    stacked -> [B, F, E].  The reference builds ``ce_layer`` and ``nonlinear_layer_list`` from the first input's shape;
    layers are built eagerly here, so ``fields_num`` and ``embedding_dims`` are extension keywords.  The sub-layers hold
    the parameters under the reference's names; the call stacks the per-field weights and runs the block as one kernel
    each way (functional.ContextNetBlock)."""

    def __init__(self, nonlinear_type="pointwise", fields_num=13, embedding_dims=16):
        super().__init__()
        self.nonlinear_type = nonlinear_type
        self.fields_num, self.embedding_dims = int(fields_num), int(embedding_dims)
        ops.contextnet_check_shape(self.fields_num, self.embedding_dims, 3)
        self.nonlinear_layer_list = torch.nn.ModuleList(
            [NonLinearFeedforwardLayer(embedding_dims=self.embedding_dims, mode=nonlinear_type)
             for _ in range(self.fields_num)])
        self.ce_layer = ContextualEmbeddingLayer(fields_num=self.fields_num, embedding_dims=self.embedding_dims)

    def forward(self, inputs):
        F, E = self.fields_num, self.embedding_dims
        d1, _, d2 = self.ce_layer.contextual_embedding_transform.layers
        nl = self.nonlinear_layer_list
        W1 = torch.stack([l.W1 for l in nl])
        W2 = torch.stack([l.W2 for l in nl]) if self.nonlinear_type == "pointwise" else None
        gamma, beta = torch.stack([l.ln.gamma for l in nl]), torch.stack([l.ln.beta for l in nl])
        y = Fn.ContextNetBlock.apply(inputs.reshape(-1, F * E), d1.kernel, d1.bias, d2.kernel, d2.bias, W1, W2, gamma, beta)
        return y.reshape(-1, F, E)


class ContextNetLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:474-531: X = rows of the categorical ids and of the ``<c>_key`` ids out of ONE table,
    the key rows scaled by their ``<c>_value`` (no LayerNorm, unlike MaskNet); block_num ContextNet blocks; output =
    final_mlp(flatten(X)) with final_mlp = Dense, PReLU per unit of final_mlp_units, then Dense(1, sigmoid) ->
    {'output': [B, 1]}."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16, block_num=6, final_mlp_units=[32], nonlinear_type="pointwise"):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features_keys = [name + "_key" for name in continuous_features]
        self.continuous_features_values = [name + "_value" for name in continuous_features]
        self.fields_num = len(self.categorical_features) + len(self.continuous_features_keys)
        self.embedding_dims = int(embedding_dims)
        if int(block_num) < 1:
            raise ValueError("block_num must be at least 1, got %r" % (block_num,))
        ops.contextnet_check_shape(self.fields_num, self.embedding_dims, 3, len(self.continuous_features_keys))
        self.embedding_layer = Embedding(feature_dims, self.embedding_dims)
        self.context_block_list = torch.nn.ModuleList(
            [ContextNetBlockLayer(nonlinear_type=nonlinear_type, fields_num=self.fields_num,
                                  embedding_dims=self.embedding_dims) for _ in range(int(block_num))])
        self.final_mlp = make_mlp_layer(list(final_mlp_units), sigmoid_units=True, normalization="None",
                                        input_dim=self.fields_num * self.embedding_dims)

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features + self.continuous_features_keys)
        values = None
        if self.continuous_features_values:
            values = _cont_block(inputs, self.continuous_features_values, X.device)[0]
        flag = ops.new_flag(X.device) if self.check_ids else None
        x = Fn.EmbScaledLookup.apply(self.embedding_layer.embeddings, X, values, flag)
        self._raise_if_oob(flag)
        x = x.reshape(X.shape[0], self.fields_num, self.embedding_dims)
        for block in self.context_block_list:
            x = block(x)
        return {"output": self.final_mlp(x.reshape(X.shape[0], -1))}


# ---------------------------------------------------------------------------------------------------
# 11.FiBiNet++: FiBiNet++
# ---------------------------------------------------------------------------------------------------

class NormInputFeaturesEmbeddingLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:78-145.  Categorical ids and the ``<c>_key`` ids of the continuous features index ONE
    table.  The categorical rows pass ONE BatchNormalization over the last axis of [B, Fc, E] (``emb_batchnorm.gamma`` /
    ``.beta`` / ``.moving_mean`` / ``.moving_variance`` [E]; batch statistics and the moving-average update in training
    mode, the moving statistics in eval mode); the row of a continuous feature is scaled by its ``<c>_value`` and passes
    its own LayerNormalization (``emb_layernorm_list.{j}.gamma`` / ``.beta``).  Returns [B, F, E], categorical fields
    first, from one fused call each way (functional.EmbNormLookup)."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features_keys = [name + "_key" for name in continuous_features]
        self.continuous_features_values = [name + "_value" for name in continuous_features]
        self.fields_num = len(self.categorical_features) + len(self.continuous_features_keys)
        self.embedding_dims = int(embedding_dims)
        ops.fibinetplus_check_shape(self.fields_num, self.embedding_dims, Fk=len(self.continuous_features_keys),
                                    min_fields=1)
        self.embedding_layer = Embedding(feature_dims, self.embedding_dims)
        self.emb_batchnorm = BatchNormalization(input_dim=self.embedding_dims)
        self.emb_layernorm_list = torch.nn.ModuleList(
            [LayerNormalization(self.embedding_dims) for _ in self.continuous_features_keys])

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features + self.continuous_features_keys)
        values = gamma_ln = beta_ln = None
        if self.continuous_features_values:
            values = _cont_block(inputs, self.continuous_features_values, X.device)[0]
            gamma_ln = torch.stack([ln.gamma for ln in self.emb_layernorm_list])
            beta_ln = torch.stack([ln.beta for ln in self.emb_layernorm_list])
        flag = ops.new_flag(X.device) if self.check_ids else None
        bn = self.emb_batchnorm
        x = Fn.EmbNormLookup.apply(self.embedding_layer.embeddings, X, values, bn.gamma, bn.beta, gamma_ln, beta_ln,
                                   bn.moving_mean, bn.moving_variance, self.training, flag)
        self._raise_if_oob(flag)
        return x.reshape(X.shape[0], self.fields_num, self.embedding_dims)


class SENetPlusLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:181-205: the embedding axis is split into group_num groups; per field the group
    means then the group maxima (width 2 G F) feed excitation = make_mlp_layer([mid, F E], 'relu') with mid = max(1,
    2 G F // reduction_ratio) (``excitation.layers.{0,3}.kernel`` / ``.bias``, ``.{1,4}.gamma`` / ``.beta``); V = inputs
    * A, no residual and no final LayerNorm.  The reference builds the excitation from the first input's shape; layers
    are built eagerly here, so ``input_shape`` (F, E) is an extension keyword.  FiBiNetPlusLayer runs the parameters
    inside its one kernel; a direct call composes the same arithmetic from the GEMM, LayerNorm and activation kernels
    plus torch for the grouping."""

    def __init__(self, reduction_ratio=3, group_num=4, input_shape=None):
        super().__init__()
        self.reduction_ratio = reduction_ratio
        self.group_num = group_num
        self.built = False
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        F, E, G = int(input_shape[-2]), int(input_shape[-1]), int(self.group_num)
        self.field_num, self.embedding_size = F, E
        if G < 1 or E % G:
            raise ValueError("group_num must divide embedding_dims, got group_num=%r, embedding_dims=%d" % (G, E))
        self.mid_unit_num = ops.fibinetplus_mid(F, G, self.reduction_ratio)
        self.excitation = make_mlp_layer([self.mid_unit_num, F * E], activation="relu", input_dim=2 * G * F)
        self.built = True

    def forward(self, inputs):
        if not self.built:
            self.build(inputs.shape)
            self.to(inputs.device)
        B, F, E = inputs.shape
        G = int(self.group_num)
        grouped = inputs.reshape(B, F, G, E // G)
        info = torch.cat([grouped.mean(dim=-1), grouped.max(dim=-1).values], dim=-1).reshape(B, 2 * G * F)
        return inputs * self.excitation(info.contiguous()).reshape(B, F, E)


class BilinearInteractionPlusLayer(BilinearInteractionLayer):
    """11.FiBiNet++/CustomLayers.py:208-242: ONE scalar per pair, p_ij = sum((v_i W_ij) * v_j) over the pairs i < j
    (itertools.combinations order), then reducing_layer = make_mlp_layer([output_dim], 'None'): Dense + LayerNormalization
    and no activation (``reducing_layer.layers.0.kernel`` / ``.bias``, ``.1.gamma`` / ``.beta``).  The matrices are named
    and packed as BilinearInteractionLayer's.  ``input_shape`` (F, E) is an extension keyword (eager build).
    FiBiNetPlusLayer runs the parameters inside its one kernel; a direct call composes the same arithmetic from the GEMM
    and LayerNorm kernels plus torch elementwise operations."""

    def __init__(self, bilinear_type="interaction", output_dim=16, input_shape=None):
        super().__init__(bilinear_type=bilinear_type, input_shape=None)
        self.output_dim = int(output_dim)
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        super().build(input_shape)
        F = self.field_num
        self.reducing_layer = make_mlp_layer([self.output_dim], activation="None", input_dim=F * (F - 1) // 2)

    def forward(self, inputs):
        if not self.built:
            self.build(inputs.shape)
            self.to(inputs.device)
        F = self.field_num
        ws = self.weights()
        p = []
        for t, (i, j) in enumerate((i, j) for i in range(F) for j in range(i + 1, F)):
            w = ws[{"all": 0, "each": i, "interaction": t}[self.bilinear_type]]
            vi = Fn.LinearAct.apply(inputs[:, i].contiguous(), w, None, ops.ACT_NONE)
            p.append((vi * inputs[:, j]).sum(dim=1))
        return self.reducing_layer(torch.stack(p, dim=1).contiguous())


class FiBiNetPlusLayer(Layer):
    """11.FiBiNet++/CustomLayers.py:148-178: X = norm_embedding_layer(inputs); output = final_mlp(concat[bilinear+(X),
    flatten(SENet+(X))]) with final_mlp = Dense, LayerNormalization, activation per unit of final_mlp_units, then
    Dense(1, sigmoid) -> {'output': [B, 1]}.  The input stage is one fused call each way (functional.EmbNormLookup), the
    two sub-layers and the concatenation one kernel each way (functional.FiBiNetPlusBlock); the head runs on the GEMM,
    LayerNorm and activation kernels."""

    def __init__(self, categorical_features=_MASKNET_CAT, continuous_features=_MASKNET_CONT, feature_dims=160000,
                 embedding_dims=16, bilinear_type="interaction", bilinear_output_dim=16, senet_reduction_ratio=3,
                 senet_group_num=2, final_mlp_units=[32], final_mlp_activation="ReLU"):
        super().__init__()
        F = len(categorical_features) + len(continuous_features)
        E, G, O = int(embedding_dims), int(senet_group_num), int(bilinear_output_dim)
        if bilinear_type not in ops.FIBINET_TYPES:
            raise NotImplementedError
        ops.fibinetplus_check_shape(F, E, G, ops.fibinetplus_mid(F, max(G, 1), senet_reduction_ratio) if G >= 1 else 1,
                                    O, len(continuous_features))
        self.norm_embedding_layer = NormInputFeaturesEmbeddingLayer(categorical_features, continuous_features,
                                                                    feature_dims, E)
        self.bilinear_interaction_plus_layer = BilinearInteractionPlusLayer(bilinear_type, O, input_shape=(F, E))
        self.senet_plus_layer = SENetPlusLayer(senet_reduction_ratio, G, input_shape=(F, E))
        # Keras spells the layer class 'ReLU'; the activation kernels know it as 'relu'
        act = "relu" if final_mlp_activation == "ReLU" else final_mlp_activation
        self.final_mlp = make_mlp_layer(list(final_mlp_units), activation=act, sigmoid_units=True, input_dim=O + F * E)

    def forward(self, inputs):
        x = self.norm_embedding_layer(inputs)
        bil, se = self.bilinear_interaction_plus_layer, self.senet_plus_layer
        red, ex = bil.reducing_layer.layers, se.excitation.layers
        out = Fn.FiBiNetPlusBlock.apply(x.reshape(x.shape[0], -1), red[0].kernel, red[0].bias, red[1].gamma, red[1].beta,
                                        ex[0].kernel, ex[0].bias, ex[1].gamma, ex[1].beta, ex[3].kernel, ex[3].bias,
                                        ex[4].gamma, ex[4].beta, int(se.group_num), bil.type_code, bil.packed_weight,
                                        *bil.weights())
        return {"output": self.final_mlp(out)}


# ---------------------------------------------------------------------------------------------------
# 5.DIN
# ---------------------------------------------------------------------------------------------------

class Dice(Layer):
    """Dice (5.DIN/CustomLayers.py:183-196): p = sigmoid(BN(x)) with BatchNormalization(center=False, scale=False),
    out = alpha*(1-p)*x + p*x, alpha init 0.  The BN runs on its moving statistics (inference mode: mean 0,
    variance 1 at init) -- the oracle is pinned to that mode; batch statistics inside
    tf.vectorized_map are not reproduced."""

    def __init__(self, axis=-1, epsilon=1e-9, input_dim=None):
        super().__init__()
        self.axis, self.epsilon = axis, epsilon
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, n):
        self.alpha = torch.nn.Parameter(torch.zeros(int(n)))
        self.register_buffer("moving_mean", torch.zeros(int(n)))
        self.register_buffer("moving_variance", torch.ones(int(n)))
        self.built = True

    def forward(self, x):
        if not self.built:
            self.build(x.shape[-1])
            self.to(x.device)
        return Fn.FeatAct.apply(x, ops.DACT_DICE, self.alpha, self.moving_mean, self.moving_variance)


class PReLU(Layer):
    """tf.keras.layers.PReLU(): max(0,x) + alpha*min(0,x), alpha per feature, init 0."""

    def __init__(self, input_dim=None):
        super().__init__()
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, n):
        self.alpha = torch.nn.Parameter(torch.zeros(int(n)))
        self.built = True

    def forward(self, x):
        if not self.built:
            self.build(x.shape[-1])
            self.to(x.device)
        return Fn.FeatAct.apply(x, ops.DACT_PRELU, self.alpha, None, None)


class Activation(Layer):
    """tf.keras.layers.Activation(name or callable layer)."""

    def __init__(self, activation):
        super().__init__()
        if isinstance(activation, torch.nn.Module):
            self.inner, self.kind = activation, None
        else:
            if activation not in ops.DACT_CODE:
                raise ValueError("Unknown activation function: %r" % (activation,))
            self.inner, self.kind = None, ops.DACT_CODE[activation]

    def forward(self, x):
        if self.inner is not None:
            return self.inner(x)
        return Fn.FeatAct.apply(x, self.kind, None, None, None)


class LayerNormalization(Layer):
    """tf.keras.layers.LayerNormalization(epsilon): last axis, gamma 1, beta 0; ``epsilon`` None is Keras' default 1e-3."""

    def __init__(self, input_dim, epsilon=None):
        super().__init__()
        self.epsilon = epsilon
        self.gamma = torch.nn.Parameter(torch.ones(int(input_dim)))
        self.beta = torch.nn.Parameter(torch.zeros(int(input_dim)))

    def forward(self, x):
        if self.epsilon is None:
            return Fn.LayerNorm.apply(x, self.gamma, self.beta)
        return Fn.LayerNorm.apply(x, self.gamma, self.beta, self.epsilon)


class SoftmaxDense(Layer):
    """Dense(units, activation='softmax')."""

    def __init__(self, units, input_dim):
        super().__init__()
        self.dense = Dense(units, activation=None, input_dim=input_dim)

    def forward(self, x):
        return Fn.Softmax.apply(self.dense(x))


class Sequential(Layer):
    def __init__(self, layers_):
        super().__init__()
        self.layers = torch.nn.ModuleList(layers_)

    def forward(self, x):
        for l in self.layers:
            x = l(x)
        return x


def make_mlp_layer(units, activation="PReLU", normalization="layernorm", softmax_units=-1, sigmoid_units=False,
                   input_dim=None):
    """5.DIN/CustomLayers.py:142-160.  ``input_dim`` (extension) is needed because layers are built eagerly."""
    if input_dim is None:
        raise ValueError("make_mlp_layer needs input_dim")
    seq = []
    d = input_dim
    for unit in units:
        seq.append(Dense(unit, input_dim=d))
        d = unit
        if normalization == "batchnorm":
            seq.append(BatchNormalization(input_dim=d))
        elif normalization == "layernorm":
            seq.append(LayerNormalization(d))
        if activation == "PReLU":
            seq.append(PReLU(d))
        elif activation == "Dice":
            seq.append(Dice(input_dim=d))
        elif isinstance(activation, torch.nn.Module):
            # the reference wraps a Dice() *instance* in Activation(...) (5.DIN/CustomLayers.py:154-155,219)
            if isinstance(activation, (Dice, PReLU)) and not activation.built:
                activation.build(d)
            seq.append(Activation(activation))
        elif activation != "None":                       # the reference's spelling of "no activation layer"
            seq.append(Activation(activation))
    if softmax_units > 0:
        seq.append(SoftmaxDense(softmax_units, d))
    elif sigmoid_units:
        seq.append(Dense(1, activation="sigmoid", input_dim=d))
    return Sequential(seq)


class DinActivationLayer(Layer):
    """5.DIN/CustomLayers.py:163-180: Dense(36) -> activation -> Dense(1) over [q, q-k, k, vec(k q^T)].
    ``call((vec1, vec2))`` scores ONE key per example like the reference; DINLayer uses the batched, fused
    attention kernel with the same parameters."""

    def __init__(self, activation="PReLU", input_dim=None, **kwargs):
        super().__init__()
        self._activation_spec = (activation,)     # in a tuple: a Dice() instance must register under mlp_layer only
        self.hidden = 36
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, D):
        D = int(D)
        self.D = D
        self.mlp_layer = make_mlp_layer([self.hidden], activation=self._activation_spec[0], normalization="none",
                                        input_dim=3 * D + D * D)
        self.output_layer = Dense(1, input_dim=self.hidden)
        self.built = True

    def act_params(self):
        act = self.mlp_layer.layers[1]
        inner = act.inner if isinstance(act, Activation) and act.inner is not None else act
        if isinstance(inner, Dice):
            return ops.DACT_DICE, inner.alpha, inner.moving_mean, inner.moving_variance
        if isinstance(inner, PReLU):
            return ops.DACT_PRELU, inner.alpha, None, None
        return inner.kind, None, None, None

    def attend(self, embed, q, series, padding_index, mask_valid, oob=None, sink=None):
        """All T keys of every example at once: pooled [B,D], raw scores [B,T]."""
        dense = self.mlp_layer.layers[0]
        kind, alpha, mean, var = self.act_params()
        return Fn.DinAttention.apply(embed, q, series, dense.kernel, dense.bias, kind, alpha, mean, var,
                                     self.output_layer.kernel, self.output_layer.bias, padding_index, mask_valid, oob,
                                     sink)

    def forward(self, inputs):
        vec1, vec2 = inputs                       # q [B,D], k [B,D]
        if not self.built:
            self.build(vec1.shape[1])
            self.to(vec1.device)
        # a single key per example = a length-1 "series" of already-gathered rows: gather from an identity table
        B, D = vec2.shape
        ids = torch.arange(B, device=vec2.device, dtype=torch.int64).reshape(B, 1, 1)
        pooled, scores = self.attend_rows(vec1, vec2, ids)
        return scores.reshape(B, 1)

    def attend_rows(self, q, keys2d, ids):
        dense = self.mlp_layer.layers[0]
        kind, alpha, mean, var = self.act_params()
        # mask_valid=1 with padding_index=-1: no position is masked; the scores are this path's result, so they carry
        # a gradient (to q, to the keys as the rows of the identity table, and to the unit's parameters)
        return Fn.DinAttention.apply(keys2d.contiguous(), q, ids, dense.kernel, dense.bias, kind, alpha, mean, var,
                                     self.output_layer.kernel, self.output_layer.bias, -1, 1, None, None, True)


class DINLayer(Layer):
    """5.DIN/CustomLayers.py:199-289.  ``mask_mode='reference'`` reproduces the reference's mask (only PADDED
    positions contribute, :256,277-278); ``'valid'`` is the intended convention."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=16, activation="Dice", padding_index=0, mask_mode="reference", sharded=False, group=None,
                 comm=None, capacity=None):
        super().__init__()
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.behavior_series_features = behavior_series_features
        self.continuous_features = continuous_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        if mask_mode not in ("reference", "valid"):
            raise ValueError("mask_mode must be 'reference' or 'valid'")
        self.mask_mode = mask_mode
        if sharded and padding_index != 0:
            raise NotImplementedError("sharded DINLayer: padding_index must be 0 (the smallest id: its row then sits in "
                                      "slot 0 of the exchanged rows, which is what the attention kernel's mask compares)")
        # sharded=True: the table is row-sharded over the process group (BASELINE config E: 50M x 32d over 8 GPUs)
        self.embed = make_embedding(feature_dims, embedding_dims, sharded, group, comm, capacity)
        D = len(item_categorical_features) * embedding_dims
        self.din_activation_layer = DinActivationLayer(
            activation=Dice() if activation == "Dice" else activation, input_dim=D)
        n_profile = len(user_and_context_categorical_features) + len(item_categorical_features)
        self.mlp = make_mlp_layer([200, 80], activation=activation, softmax_units=2,
                                  input_dim=n_profile * embedding_dims + D)
        self.padding_index = padding_index

    def forward(self, inputs):
        prof_names = self.user_and_context_categorical_features + self.item_categorical_features
        X_cate = assemble_index(inputs, prof_names)
        flag = ops.new_flag(X_cate.device) if self.check_ids else None
        n_item = len(self.item_categorical_features)
        mask_valid = 1 if self.mask_mode == "valid" else 0
        if _is_sharded(self.embed):
            # row-sharded table: ONE de-duplicated exchange for the profile ids, the behaviour series and the padding id
            # (always part of the lookup: as the smallest id it is unique 0 of owner 0 = slot 0 of the rows that come
            # back, so the attention kernel's mask `first series id == padding_index` becomes `slot == 0`); every
            # consumer then works on the local [P*cap, E] rows buffer with slots in place of ids
            series = _stack_ids(inputs, self.behavior_series_features, X_cate.device)
            pad = torch.full((1,), self.padding_index, dtype=torch.int64, device=X_cate.device)
            n1, n2 = X_cate.numel(), series.numel()
            rows, slot = self.embed.exchange(torch.cat([X_cate.reshape(-1), series.reshape(-1), pad]), flag)
            s_cate = slot[:n1].reshape(X_cate.shape).contiguous()
            s_series = slot[n1:n1 + n2].reshape(series.shape).contiguous()
            # (the consumers' gradients -- profile rows, series values, a zero row for the padding lookup -- line up with
            # the exchange's id list, whose de-duplication plan the backward reuses)
            sink = self.embed.grad_sink(X_cate, n_tail=1)
            profile = self.embed.take(rows, s_cate, sink)
            profile_output = profile.reshape(profile.shape[0], -1)
            q = profile[:, profile.shape[1] - n_item:, :].reshape(profile.shape[0], -1)
            pooled, _ = self.din_activation_layer.attend(rows, q, s_series, 0, mask_valid, None, sink)
            self._raise_if_oob(flag)
            X_combined = ConcatCols.apply(profile_output, pooled)
            return {"output": self.mlp(X_combined)}
        # one lookup serves both: the candidate item's rows are the tail of the profile rows (the reference looks the
        # item ids up a second time, 5.DIN/CustomLayers.py:244-247 -- same values), and the series lookups of the
        # attention share the profile lookup's de-duplication (functional.GradSink)
        sink = self.embed.grad_sink(X_cate)
        profile = self.embed(X_cate, flag, sink)
        profile_output = profile.reshape(profile.shape[0], -1)
        q = profile[:, profile.shape[1] - n_item:, :].reshape(profile.shape[0], -1)
        series = _stack_ids(inputs, self.behavior_series_features, X_cate.device)
        pooled, _ = self.din_activation_layer.attend(self.embed.embeddings, q, series, self.padding_index,
                                                     mask_valid, flag, sink)
        self._raise_if_oob(flag)
        X_combined = ConcatCols.apply(profile_output, pooled)
        return {"output": self.mlp(X_combined)}


# ---------------------------------------------------------------------------------------------------
# sibling layers on the same gather
# ---------------------------------------------------------------------------------------------------

class BatchNormalization(Layer):
    """tf.keras.layers.BatchNormalization() on [B,N]: axis=-1, momentum=0.99, epsilon=1e-3, gamma ones, beta zeros,
    moving mean 0 / variance 1.  Like Keras it normalises with BATCH statistics (and updates the moving averages)
    when the module is in training mode -- the reference's train loops call ``model(inputs, training=True)``
    (3.DCN/ModelManager.py:192) -- and with the moving statistics in eval mode."""

    def __init__(self, momentum=0.99, epsilon=1e-3, center=True, scale=True, input_dim=None):
        super().__init__()
        self.momentum, self.epsilon, self.center, self.scale = momentum, epsilon, center, scale
        self.built = False
        if input_dim is not None:
            self.build(input_dim)

    def build(self, n):
        n = int(n)
        self.gamma = torch.nn.Parameter(torch.ones(n)) if self.scale else None
        self.beta = torch.nn.Parameter(torch.zeros(n)) if self.center else None
        self.register_buffer("moving_mean", torch.zeros(n))
        self.register_buffer("moving_variance", torch.ones(n))
        self.built = True

    def forward(self, x):
        if not self.built:
            self.build(x.shape[-1])
            self.to(x.device)
        return Fn.BatchNorm.apply(x, self.gamma, self.beta, self.moving_mean, self.moving_variance, self.training,
                                  self.epsilon, self.momentum)


class PNNLayer(Layer):
    """2.FM/CustomLayers.py:696-745 with method='inner' (IpnLayer, :773-792): embed -> [Flatten | pairwise inner
    products] -> MLP(relu) -> MLP([1], sigmoid).  The lookup, the flatten and the F(F-1)/2 inner products are one
    kernel; its output IS ``combined_vector``.  method='outer' (OpnLayer) is not on the hot path."""

    def __init__(self, feature_names=["user_tag0", "user_tag1", "item_tag1", "item_tag2", "item_tag3"], feature_dims=20,
                 embedding_dims=16, mlp_dims=[32, 8], dropout=0, method="inner", kernel_type=None, **kwargs):
        super().__init__()
        assert method in ("inner", "outer")
        if method == "outer":
            raise NotImplementedError("PNNLayer(method='outer') is outside the accelerated path")
        self.feature_names = feature_names
        self.feature_dims = feature_dims
        self.fields_cnt = len(feature_names)
        self.embedding_dims = embedding_dims
        self.mlp_dims = mlp_dims
        self.method, self.dropout, self.kernel_type = method, dropout, kernel_type
        F = self.fields_cnt
        self.embed = Embedding(feature_dims, embedding_dims, embeddings_regularizer="l2")
        self.MLP_layer1 = MLPLayer(units=mlp_dims, activation="relu", is_dropput=dropout,
                                   input_dim=F * embedding_dims + F * (F - 1) // 2)
        self.MLP_layer2 = MLPLayer(units=[1], activation="sigmoid", input_dim=list(mlp_dims)[-1])

    def forward(self, inputs):
        X = assemble_index(inputs, self.feature_names)
        flag = ops.new_flag(X.device) if self.check_ids else None
        combined_vector = Fn.EmbIpn.apply(self.embed.embeddings, X, flag)
        self._raise_if_oob(flag)
        output = self.MLP_layer2(self.MLP_layer1(combined_vector))
        return {"output": output}


class NeuralFactorizationMachineLayer(Layer):
    """3.DCN/CustomLayers.py:451-509: bi-interaction pooling of the categorical embeddings ++ continuous features ->
    BatchNormalization -> MLP(units, activation) -> MLP([1], sigmoid).  (The first-order table ``w`` is created by
    the reference but never used, :491-495; it is not allocated here.)"""

    def __init__(self, categorical_features=["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2",
                                             "itag3", "itag4"],
                 continuous_features=["itag4_origin", "itag4_square", "itag4_cube"], feature_dims=160000,
                 embedding_dims=16, units=[64, 8], activation="relu"):
        super().__init__()
        self.categorical_features = categorical_features
        self.continuous_features = continuous_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        n = embedding_dims + len(continuous_features)
        self.embed = Embedding(feature_dims, embedding_dims, embeddings_regularizer="l2")
        self.bn_layer = BatchNormalization(input_dim=n)
        self.MLP_layer1 = MLPLayer(units=units, activation=activation, input_dim=n)
        self.MLP_layer2 = MLPLayer(units=[1], activation="sigmoid", input_dim=list(units)[-1])

    def forward(self, inputs):
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        cont = _cont_block(inputs, self.continuous_features, X.device)
        X_cont = torch.cat(cont, dim=1) if cont else None
        combined_vector = Fn.EmbBiInteraction.apply(self.embed.embeddings, X, X_cont, flag)
        self._raise_if_oob(flag)
        combined_vector = self.bn_layer(combined_vector)
        output = self.MLP_layer2(self.MLP_layer1(combined_vector))
        return {"output": output}


class GSULayer(Layer):
    """7.SIM/CustomLayers.py:62-127 (general search unit): target item embedding, inner-product attention over the
    embedded behaviour series with the valid mask, sum pooling, MLP [200,80] + softmax(2).  The series lookup,
    scores and pooling are one kernel, so ``X_series`` (the [B,T,D] embedded series the reference also returns) is
    only materialised when ``return_series=True``."""

    def __init__(self, item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=1000, embedding_dims=16, activation="Dice", padding_index=0, embedding_layer=None,
                 l2_reg=0.01, return_series=False):
        super().__init__()
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.behavior_series_features = behavior_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.l2_reg = l2_reg
        self.embed = embedding_layer if embedding_layer is not None else Embedding(feature_dims, embedding_dims)
        D = len(item_categorical_features) * embedding_dims
        self.mlp = make_mlp_layer([200, 80], activation=activation, softmax_units=2, input_dim=2 * D)
        self.padding_index = padding_index
        self.return_series = return_series

    def forward(self, inputs):
        X_item = assemble_index(inputs, self.item_categorical_features)
        flag = ops.new_flag(X_item.device) if self.check_ids else None
        sink = self.embed.grad_sink(X_item)        # the series lookups share the item lookup's de-duplication
        q = self.embed(X_item, flag, sink)
        q = q.reshape(q.shape[0], -1)
        series = _stack_ids(inputs, self.behavior_series_features, X_item.device)
        B, T, C = series.shape
        pooled, _ = Fn.IpAttention.apply(self.embed.embeddings, q, series, self.padding_index, flag, sink)
        self._raise_if_oob(flag)
        X_combined = ConcatCols.apply(q, pooled)
        result = {"output": self.mlp(X_combined), "valid_mask": series[:, :, 0] != self.padding_index}
        if self.return_series:
            result["X_series"] = self.embed(series.reshape(B, T * C)).reshape(B, T, -1)
        return result


class FieldAwareInteractionLayer(Layer):
    """Holder of the field-aware table ``v`` [feature_dims, fields_cnt, embedding_dims] (2.FM/CustomLayers.py:428-434):
    v[id, c, :] is the vector id uses against field c.  The interaction itself is fused into Fn.FFM."""

    def __init__(self, fields_cnt, feature_dims=20, embedding_dims=16, **kwargs):
        super().__init__()
        self.v = torch.nn.Parameter(_uniform((feature_dims, fields_cnt, embedding_dims), 0.05))


class FFMLayer(Layer):
    """2.FM/CustomLayers.py:465-497: sigmoid(bias + sum_f w[x_f] + sum_{a<c} <v[x_a,c,:], v[x_c,a,:]>).  (The reference
    builds its FieldAwareInteractionLayer with the DEFAULT feature_dims=20 / embedding_dims=16, ignoring the layer's
    own arguments, :476; the layer's arguments are used here.)"""

    def __init__(self, feature_names=["item_tag1", "item_tag2", "item_tag3", "user_tag0", "user_tag1"], feature_dims=20,
                 embedding_dims=16, **kwargs):
        super().__init__()
        self.feature_names = feature_names
        self.feature_dims = feature_dims
        self.fields_cnt = len(feature_names)
        self.embedding_dims = embedding_dims
        self.bias = torch.nn.Parameter(_uniform((1,), 0.05))
        self.w = torch.nn.Parameter(_uniform((feature_dims, 1), 0.05))
        self.fa_interaction_layer = FieldAwareInteractionLayer(self.fields_cnt, feature_dims, embedding_dims)

    def logit(self, inputs):
        X = assemble_index(inputs, self.feature_names)
        flag = ops.new_flag(X.device) if self.check_ids else None
        z = Fn.FFM.apply(self.fa_interaction_layer.v, self.w, self.bias, X, flag)
        self._raise_if_oob(flag)
        return z

    def forward(self, inputs):
        z = self.logit(inputs)
        return {"output": Fn.Sigmoid.apply(z).reshape(-1, 1)}


class FFMRankingLayer(FFMLayer):
    """2.FM/CustomLayers.py:370-425, the loop form: ``embedding_list[i]`` is the table used against field i and
    ebd_out[i][:, j] * ebd_out[j][:, i] = table_i[x_j] * table_j[x_i].  Same numbers as FFMLayer with
    v[id, i, :] = embedding_list[i][id, :]; the F tables are kept interleaved per id (one id's F vectors contiguous)
    and exposed as strided views."""

    def __init__(self, feature_names=["item_tag1", "item_tag2", "item_tag3"], feature_dims=20, embedding_dims=16,
                 **kwargs):
        super().__init__(feature_names=feature_names, feature_dims=feature_dims, embedding_dims=embedding_dims)

    @property
    def embedding_list(self):
        v = self.fa_interaction_layer.v
        return [v[:, i, :] for i in range(self.fields_cnt)]


class PNNRankingLayer(PNNLayer):
    """2.FM/CustomLayers.py:536-598 (the loop form, InnerProductNetwork :601-624): same numbers as PNNLayer."""


# ---------------------------------------------------------------------------------------------------
# 4.MMOE: MMOE, ESMM, PLE
# ---------------------------------------------------------------------------------------------------

_MMOE_CAT = ["sdk_type", "remote_host", "device_type", "dtu", "click_goods_num", "buy_click_num", "goods_show_num",
             "goods_click_num", "brand_name"]
_MMOE_CONT = ["click_goods_num_origin", "click_goods_num_square", "click_goods_num_cube"]


class MMOELayer(Layer):
    """4.MMOE/CustomLayers.py:107-173: the flattened rows of the categorical ids feed ``expert_num`` expert MLPs [64, 8]
    and one gate MLP [64, expert_num] per task (relu on every layer, the gate's last one too, then a softmax); each
    task's tower, MLP [64, 8] then a sigmoid unit, reads the expert outputs scaled by its gate and FLATTENED (not summed)
    -> {'ctr_output': [B, 1], 'cvr_output': [B, 1]}.  ``continuous_features`` is accepted and unused, as in the
    reference.  The sub-layers hold the parameters under the reference's names; the call packs them and runs everything
    after the lookup as one kernel each way (functional.MMOEBody)."""

    task_names = ("ctr", "cvr")
    gate_softmax_passes = 1
    ctcvr = False

    def __init__(self, categorical_features=_MMOE_CAT, continuous_features=_MMOE_CONT, feature_dims=160000,
                 embedding_dims=16, expert_num=3):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        self.embedding_dims = int(embedding_dims)
        self.expert_num = int(expert_num)
        D, n = len(self.categorical_features) * self.embedding_dims, self.expert_num
        ops.mmoe_check_shape(D, n, len(self.task_names), 64, 8, 64, 8)
        self.embedding_layer = Embedding(feature_dims, self.embedding_dims)
        self.expert_model = torch.nn.ModuleList(
            [MLPLayer(units=[64, 8], activation="relu", input_dim=D) for _ in range(n)])
        self.ctr_gate = MLPLayer(units=[64, n], activation="relu", input_dim=D)
        self.cvr_gate = MLPLayer(units=[64, n], activation="relu", input_dim=D)
        tower = lambda: torch.nn.ModuleList([MLPLayer(units=[64, 8], activation="relu", input_dim=n * 8),
                                             MLPLayer(units=[1], activation="sigmoid", input_dim=8)])
        self.ctr_output = tower()
        self.cvr_output = tower()

    def packed_weights(self):
        """The sub-layers' parameters in the packed layout of include/mi355rec.h (W1, b1, We2, be2, Wg2, bg2, Wt1, bt1,
        Wt2, bt2, Wt3, bt3); gradients flow back through the concatenations."""
        first = list(self.expert_model) + [self.ctr_gate, self.cvr_gate]
        gates, towers = [self.ctr_gate, self.cvr_gate], [self.ctr_output, self.cvr_output]
        cat, stack = torch.cat, torch.stack
        return (cat([m.kernel_0 for m in first], dim=1), cat([m.bias_0 for m in first]),
                stack([m.kernel_1 for m in self.expert_model]), stack([m.bias_1 for m in self.expert_model]),
                stack([m.kernel_1 for m in gates]), stack([m.bias_1 for m in gates]),
                stack([t[0].kernel_0 for t in towers]), stack([t[0].bias_0 for t in towers]),
                stack([t[0].kernel_1 for t in towers]), stack([t[0].bias_1 for t in towers]),
                stack([t[1].kernel_0.reshape(-1) for t in towers]), cat([t[1].bias_0 for t in towers]))

    def task_outputs(self, inputs):
        """[B, 2]: column 0 is 'ctr_output', column 1 'cvr_output' (the dict entries are views of it)."""
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        x = self.embedding_layer(X, flag)
        self._raise_if_oob(flag)
        return Fn.MMOEBody.apply(x.reshape(X.shape[0], -1), self.gate_softmax_passes, self.ctcvr,
                                 *self.packed_weights())

    def forward(self, inputs):
        out = self.task_outputs(inputs)
        return {"ctr_output": out[:, 0:1], "cvr_output": out[:, 1:2]}


class ESMMLayer(MMOELayer):
    """4.MMOE/CustomLayers.py:175-245: MMOE's structure with the gate's softmax applied twice (227-233) and
    'cvr_output' = ctr * cvr (243-244)."""

    gate_softmax_passes = 2
    ctcvr = True

    def __init__(self, categorical_features=_MMOE_CAT, continuous_features=_MMOE_CONT, feature_dims=160000,
                 embedding_dims=16, expert_num=3):
        super().__init__(categorical_features, continuous_features, feature_dims, embedding_dims, expert_num)


class PLELayer(Layer):
    """4.MMOE/CustomLayers.py:248-384: progressive layered extraction.  ``level_num`` CGC levels; a level has
    ``specific_expert_num`` expert MLPs [64, 8] per task and ``shared_expert_num`` shared ones, one gate per task (MLP
    [64, 8], then a bias-free dense layer whose softmax the reference applies TWICE) over the task's experts and the
    shared ones, and, except the last level, a shared gate (softmax once) over all experts; a gate's output is the
    weighted SUM of its experts.  The first level reads the flattened embedding rows for every branch, a later one the
    previous level's outputs, one per task and one shared.  A sigmoid unit per task reads the last level ->
    {'task_0': [B, 1], 'task_1': [B, 1], 'task_2': [B, 1]}.  ``continuous_features`` is accepted and unused, as in the
    reference.  The sub-layers hold the parameters under the reference's names (the gates' dense layers are holders
    of ``kernel_0``: their softmax runs inside the kernel); a call packs them level by level and runs each level as one
    kernel each way (functional.PLELevel)."""

    num_tasks = 3               # the reference fixes it (:271)

    def __init__(self, categorical_features=_MMOE_CAT, continuous_features=_MMOE_CONT, feature_dims=160000,
                 embedding_dims=8, specific_expert_num=3, shared_expert_num=3, level_num=2):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.continuous_features = list(continuous_features)
        self.embedding_dims = int(embedding_dims)
        self.specific_expert_num = int(specific_expert_num)
        self.shared_expert_num = int(shared_expert_num)
        self.level_num = int(level_num)
        if self.level_num < 1:
            raise ValueError("level_num must be at least 1, got %d" % self.level_num)
        T, S, Sh, L = self.num_tasks, self.specific_expert_num, self.shared_expert_num, self.level_num
        D = len(self.categorical_features) * self.embedding_dims
        H1, O, Og = 64, 8, 8
        dins = [D] + [O] * (L - 1)
        for level, din in enumerate(dins):
            ops.ple_check_shape(din, 1 if level == 0 else T + 1, T, S, Sh, H1, O, Og, level == L - 1)
        self.embedding_layer = Embedding(feature_dims, self.embedding_dims)
        ML = torch.nn.ModuleList
        mlp = lambda din: MLPLayer(units=[H1, O], activation="relu", input_dim=din)
        gate = lambda din, width: ML([MLPLayer(units=[H1, Og], activation="relu", input_dim=din),
                                      MLPLayer(units=[width], use_bias=False, activation=None, input_dim=Og)])
        self.specific_expert_networks = ML([ML([mlp(din) for _ in range(T * S)]) for din in dins])
        self.shared_expert_networks = ML([ML([mlp(din) for _ in range(Sh)]) for din in dins])
        self.specific_gates = ML([ML([gate(din, S + Sh) for _ in range(T)]) for din in dins])
        self.shared_gates = ML([gate(din, T * S + Sh) for din in dins[:-1]])       # the last level has no shared output
        self.tower_outputs = ML([MLPLayer(units=[1], activation="sigmoid", input_dim=O) for _ in range(T)])

    def packed_weights(self, level):
        """Level ``level``'s parameters in the packed layout of include/mi355rec.h (W1, b1, We2, be2, Wg2, bg2, Wg3s,
        Wg3h, Wtw, btw; None for the shared gate of the last level and the towers of the others); gradients flow back
        through the concatenations."""
        last = level == self.level_num - 1
        experts = list(self.specific_expert_networks[level]) + list(self.shared_expert_networks[level])
        gates = list(self.specific_gates[level]) + ([] if last else [self.shared_gates[level]])
        first = experts + [gt[0] for gt in gates]
        cat, stack = torch.cat, torch.stack
        return (cat([m.kernel_0 for m in first], dim=1), cat([m.bias_0 for m in first]),
                stack([m.kernel_1 for m in experts]), stack([m.bias_1 for m in experts]),
                stack([gt[0].kernel_1 for gt in gates]), stack([gt[0].bias_1 for gt in gates]),
                stack([gt[1].kernel_0 for gt in self.specific_gates[level]]),
                None if last else self.shared_gates[level][1].kernel_0,
                stack([t.kernel_0.reshape(-1) for t in self.tower_outputs]) if last else None,
                cat([t.bias_0 for t in self.tower_outputs]) if last else None)

    def task_outputs(self, inputs):
        """[B, 3]: column i is 'task_i' (the dict entries are views of it)."""
        X = assemble_index(inputs, self.categorical_features)
        flag = ops.new_flag(X.device) if self.check_ids else None
        x = self.embedding_layer(X, flag)
        self._raise_if_oob(flag)
        cfg = (self.num_tasks, self.specific_expert_num, self.shared_expert_num)
        y = x.reshape(X.shape[0], 1, -1)
        for level in range(self.level_num - 1):
            y = Fn.PLELevel.apply(y, *cfg, False, *self.packed_weights(level))
        return Fn.PLELevel.apply(y, *cfg, True, *self.packed_weights(self.level_num - 1))[1]

    def forward(self, inputs):
        out = self.task_outputs(inputs)
        return {"task_%d" % i: out[:, i:i + 1] for i in range(self.num_tasks)}


# ---------------------------------------------------------------------------------------------------
# 10.POSO: GateNU, POSO-MLP, PEPNet
# ---------------------------------------------------------------------------------------------------

_POSO_ACTS = ("relu", "sigmoid", "linear")


class _Sequential(Layer):
    """tf.keras.models.Sequential of Dense layers: ``layers.{i}.{kernel,bias}``."""

    def __init__(self, layers):
        super().__init__()
        self.layers = torch.nn.ModuleList(layers)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class GateNULayer(Layer):
    """10.POSO/CustomLayers.py:76-89: 2 * sigmoid(relu(x A + a) Bm + bm), parameters ``gate.layers.{0,1}.{kernel,bias}``.
    ``input_dim`` builds the parameters at construction (the fused layers below read them; they never call this layer).
    A direct call runs the two Dense layers on their own kernels."""

    def __init__(self, hidden_unit=16, output_unit=16, input_dim=None):
        super().__init__()
        self.hidden_unit, self.output_unit = int(hidden_unit), int(output_unit)
        self.gate = _Sequential([Dense(self.hidden_unit, activation="relu", input_dim=input_dim),
                                 Dense(self.output_unit, activation="sigmoid", input_dim=self.hidden_unit)])

    def forward(self, inputs):
        shape = inputs.shape
        return (2.0 * self.gate(inputs.reshape(-1, shape[-1]))).reshape(*shape[:-1], self.output_unit)


class _Holder(Layer):
    """``kernel`` / ``bias`` of a Dense layer that only a fused kernel reads."""

    def __init__(self, input_dim, units):
        super().__init__()
        self.kernel = torch.nn.Parameter(glorot_uniform((int(input_dim), int(units))))
        self.bias = torch.nn.Parameter(torch.zeros(int(units)))


class PosoForMLPLayer(Layer):
    """10.POSO/CustomLayers.py:92-119: an MLP whose every layer is scaled by a GateNU of a second input and a trainable
    scalar, act_i(C_i (in W_i + b_i) (.) GateNU_i(gate input)), called as ``layer(main, gate)`` -> [B, units[-1]].
    Parameters under the reference's names: ``dense_layers.{i}.{kernel,bias}``, ``gates.{i}.gate.layers.{0,1}.{kernel,
    bias}``, ``C_list.{i}``.  Activations: 'relu', 'sigmoid', 'linear'; 'PReLU' and ``norm`` (which the reference builds
    as a fresh, untrained Keras layer inside every call: nothing stable to mirror) raise NotImplementedError.

    ``chain_layers=False`` (the default) is the reference AS WRITTEN: every layer reads ``main`` (:109), the loop keeps
    only the last layer's activation (:118-119), so the output is the last layer applied to ``main``; the layers before
    it hold parameters of input width ``main_dim``, are not computed and get no gradient (None, as in TF).
    ``chain_layers=True`` is an EXTENSION, not reference behaviour (in the sense of DINLayer(mask_mode='valid')): the
    MLP the loop's ``inputs=`` assignment and the POSO paper mean, layer i reading layer i-1's activation, so W_i is
    [units[i-1], units[i]].  Both run on one kernel each way (functional.PosoMLP): literal mode is that kernel with one
    layer."""

    def __init__(self, units=[32, 16, 8], activations=["relu", "relu", "relu"], gate_hidden_multiple=2, norm=None,
                 main_dim=None, gate_dim=None, chain_layers=False):
        super().__init__()
        if norm is not None:
            raise NotImplementedError("PosoForMLPLayer(norm=%r): the reference constructs an untrained normalisation "
                                      "layer inside every call; only norm=None is built" % (norm,))
        self.units = [int(u) for u in units]
        self.activations = list(activations)
        if len(self.activations) != len(self.units) or not self.units:
            raise ValueError("units and activations must have the same, positive length, got %d and %d"
                             % (len(self.units), len(self.activations)))
        for act in self.activations:
            if act not in _POSO_ACTS:
                raise NotImplementedError("PosoForMLPLayer covers the activations %s, got %r" % (_POSO_ACTS, act))
        if main_dim is None or gate_dim is None:
            raise ValueError("PosoForMLPLayer needs main_dim and gate_dim: its kernel reads parameters built at "
                             "construction")
        self.gate_hidden_multiple = int(gate_hidden_multiple)
        self.main_dim, self.gate_dim, self.chain_layers = int(main_dim), int(gate_dim), bool(chain_layers)
        self.norm = None
        self.layer_depth = len(self.units)
        ops.poso_mlp_check_shape(self.main_dim, self.gate_dim, 1, self.live_units(), self.gate_hidden_multiple)
        dims = [self.main_dim] + (self.units[:-1] if self.chain_layers else [self.main_dim] * (self.layer_depth - 1))
        self.dense_layers = torch.nn.ModuleList([_Holder(k, u) for k, u in zip(dims, self.units)])
        self.gates = torch.nn.ModuleList(
            [GateNULayer(self.gate_hidden_multiple * u, u, input_dim=self.gate_dim) for u in self.units])
        self.C_list = torch.nn.ParameterList([torch.nn.Parameter(torch.ones(())) for _ in self.units])

    def live_layers(self):
        """indices of the layers that reach the output: all of them when chained, the last one as written"""
        return list(range(self.layer_depth)) if self.chain_layers else [self.layer_depth - 1]

    def live_units(self):
        return [self.units[i] for i in self.live_layers()]

    def live_activations(self):
        return [self.activations[i] for i in self.live_layers()]

    def forward(self, inputs_for_main, inputs_for_gate):
        weights = pack_poso_weights([self])
        out = Fn.PosoMLP.apply(inputs_for_main, inputs_for_gate, self.live_units(), self.live_activations(),
                               self.gate_hidden_multiple, 0, *weights)
        return out[:, 0, :]


def pack_poso_weights(towers):
    """The live layers' parameters of T PosoForMLPLayers of one shape in the packed layout of include/mi355rec.h (Wg1,
    bg1, Wg2, bg2, W, b, C); gradients flow back through the concatenations."""
    cat = torch.cat
    pairs = [(t, i) for t in towers for i in t.live_layers()]
    g0 = lambda t, i: t.gates[i].gate.layers[0]
    g1 = lambda t, i: t.gates[i].gate.layers[1]
    return (cat([g0(t, i).kernel for t, i in pairs], dim=1), cat([g0(t, i).bias for t, i in pairs]),
            cat([g1(t, i).kernel.reshape(-1) for t, i in pairs]), cat([g1(t, i).bias for t, i in pairs]),
            cat([t.dense_layers[i].kernel.reshape(-1) for t, i in pairs]),
            cat([t.dense_layers[i].bias for t, i in pairs]),
            torch.stack([t.C_list[i] for t, i in pairs]).reshape(len(towers), -1))


_PEPNET_PP = ["ppnet_cate1", "ppnet_cate2"]
_PEPNET_EP = ["epnet_cate1", "epnet_cate2"]


class PEPNetLayer(Layer):
    """10.POSO/CustomLayers.py:371-462: parameter- and embedding-personalised network.  ONE table serves the
    ``categorical_features`` (main rows [B, F, E]) and the ``ppnet_input_features`` (pp [B, P E]).  EPNet: field f's
    rows are multiplied by GateNU_f(pp).  PPNet: ``num_tasks`` PosoForMLPLayers (units ``poso_mlp_units``, relu, relu,
    sigmoid) read the flattened gated rows c, gated by concat(stop_gradient(c), pp) -> a TENSOR [B, num_tasks,
    poso_mlp_units[-1]] (tf.stack(axis=1)), not a dict.
    Kept as the reference has it: the EPNet input is built from ``ppnet_input_features`` a second time (:439), so
    ``epnet_input_features`` is stored and never read (a batch needs no such keys); no gradient reaches c, the main
    ids' rows or the EPNet gates through the towers' gate input; with ``chain_layers=False`` every tower layer reads c
    and only the last one reaches the output (see PosoForMLPLayer; ``chain_layers=True`` is the extension described
    there).  The lookup, the EPNet gates and the product are one kernel each way (functional.EmbEPNetLookup), whose
    output is both the towers' main input (its leading F E columns) and their gate input; the towers are one kernel
    each way (functional.PosoMLP)."""

    def __init__(self, categorical_features=_MMOE_CAT, ppnet_input_features=_PEPNET_PP,
                 epnet_input_features=_PEPNET_EP, feature_dims=160000, embedding_dims=8, gate_hidden_dim=16,
                 num_tasks=3, poso_mlp_units=[64, 16, 1], chain_layers=False):
        super().__init__()
        self.categorical_features = list(categorical_features)
        self.ppnet_input_features = list(ppnet_input_features)
        self.epnet_input_features = list(epnet_input_features)      # stored, never read: as the reference
        self.embedding_dims, self.gate_hidden_dim = int(embedding_dims), int(gate_hidden_dim)
        self.num_tasks, self.chain_layers = int(num_tasks), bool(chain_layers)
        self.poso_mlp_units = [int(u) for u in poso_mlp_units]
        if len(self.poso_mlp_units) != 3:
            raise ValueError("PEPNetLayer fixes three activations (relu, relu, sigmoid): poso_mlp_units needs three "
                             "widths, got %s" % (self.poso_mlp_units,))
        F, P, E = len(self.categorical_features), len(self.ppnet_input_features), self.embedding_dims
        ops.pepnet_check_shape(F, P, E, self.gate_hidden_dim, self.num_tasks, self.poso_mlp_units, 2, self.chain_layers)
        self.embedding_layer = Embedding(feature_dims, E)
        self.poso_gate_for_embedding = torch.nn.ModuleList(
            [GateNULayer(self.gate_hidden_dim, E, input_dim=P * E) for _ in range(F)])
        self.poso_mlp_layers = torch.nn.ModuleList(
            [PosoForMLPLayer(units=self.poso_mlp_units, activations=["relu", "relu", "sigmoid"], gate_hidden_multiple=2,
                             norm=None, main_dim=F * E, gate_dim=(F + P) * E, chain_layers=self.chain_layers)
             for _ in range(self.num_tasks)])

    def packed_epnet_weights(self):
        """The EPNet gates' parameters stacked over the fields: A [F, P E, Hg], a [F, Hg], Bm [F, Hg, E], bm [F, E]."""
        gates = [gt.gate.layers for gt in self.poso_gate_for_embedding]
        stack = torch.stack
        return (stack([g[0].kernel for g in gates]), stack([g[0].bias for g in gates]),
                stack([g[1].kernel for g in gates]), stack([g[1].bias for g in gates]))

    def forward(self, inputs):
        F = len(self.categorical_features)
        ids = assemble_index(inputs, self.categorical_features + self.ppnet_input_features)
        flag = ops.new_flag(ids.device) if self.check_ids else None
        u = Fn.EmbEPNetLookup.apply(self.embedding_layer.embeddings, ids, F, flag, *self.packed_epnet_weights())
        self._raise_if_oob(flag)
        tower = self.poso_mlp_layers[0]
        return Fn.PosoMLP.apply(None, u, tower.live_units(), tower.live_activations(), tower.gate_hidden_multiple,
                                F * self.embedding_dims, *pack_poso_weights(self.poso_mlp_layers))

    def task_outputs(self, inputs):
        """[B, num_tasks]: column t is task t's output (a view of forward's tensor); needs poso_mlp_units[-1] == 1."""
        if self.poso_mlp_units[-1] != 1:
            raise ValueError("task_outputs needs one output unit per task, poso_mlp_units ends in %d"
                             % self.poso_mlp_units[-1])
        return self.forward(inputs)[:, :, 0]


# ---------------------------------------------------------------------------------------------------
# MIND: multi-interest retrieval (6.MIND/CustomLayers.py:62-285)
# ---------------------------------------------------------------------------------------------------

def _stack_ids(inputs, names, device, pack=None):
    """tf.stack(axis=2) of 2-D id features: [B,T] each -> int64 [B,T,len(names)] on ``device``.  ``pack``: what joins
    the columns in place of ops.index_pack (a composed path that runs on torch alone, on any device)."""
    cols = []
    for name in names:
        t = inputs[name]
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        t = t.to(device=device, dtype=torch.int64).contiguous()
        if t.dim() != 2:
            raise ValueError("feature %r must have shape [B,T], got %s" % (name, tuple(t.shape)))
        cols.append(t)
    B, T = cols[0].shape
    return (pack or ops.index_pack)(cols).reshape(B, T, len(cols))


def mind_capsule_count_table(max_length, capsules_num):
    """int32 [max_length + 1]: the number of valid capsules of an example with n valid behaviours.  The reference computes
    ``log(n) / log(2.)`` in fp32, clips it at capsules_num and masks capsule k where ``k + 1 >`` it
    (6.MIND/CustomLayers.py:214-218).  This is the numpy-float32 reading of those lines, in that order of operations, built
    once on the host (nobody here can run TensorFlow); n = 0 gives -inf and so 0 capsules."""
    import numpy as np
    n = np.arange(int(max_length) + 1, dtype=np.float32)
    with np.errstate(divide="ignore"):
        v = np.log(n) / np.log(np.float32(2.))
    v = np.minimum(v, np.float32(capsules_num))
    k1 = np.arange(int(capsules_num), dtype=np.float32) + np.float32(1)
    assert v.dtype == np.float32 and k1.dtype == np.float32
    return torch.from_numpy((~(k1[None, :] > v[:, None])).sum(axis=1).astype(np.int32))


class MultiInterestExtractorLayer(Layer):
    """6.MIND/CustomLayers.py:62-138: B2I dynamic routing of a behaviour series into ``capsules_num`` interest capsules.
    ``S`` [D, capsules_dim] is trained, the routing logits ``B`` [capsules_num, T] are a buffer (the reference's
    non-trainable weight); both random_normal(stddev 0.05).  squash is evaluated as c n / (1 + n^2), zero with a zero
    gradient at n = 0 where the reference's n^2 / ((1 + n^2) n) is 0/0.
    The lookup is part of the kernel, so the call takes ``(table, series)`` -- the embedding matrix [V,E] and the stacked
    ids [B,T,C] -- where the reference takes the looked-up behaviours and their mask; the mask is
    ``series[:, :, 0] != padding_index``, as MINDLayer computes it.  ``input_shape=(T, D)`` (extension) builds eagerly."""

    def __init__(self, capsules_num, capsules_dim, routing_rounds=3, input_shape=None):
        super().__init__()
        self.capsules_num = capsules_num
        self.capsules_dim = capsules_dim
        self.routing_rounds = routing_rounds
        self.built = False
        if input_shape is not None:
            self.build(input_shape)

    def build(self, input_shape):
        T, D = (int(v) for v in tuple(input_shape)[-2:])
        ops.mind_check_shape(D, self.capsules_dim, self.capsules_num, self.routing_rounds, T=T)
        init = _initializer("random_normal")
        self.S = torch.nn.Parameter(init((D, self.capsules_dim)))
        self.register_buffer("B", init((self.capsules_num, T)))
        self.built = True

    def forward(self, inputs, padding_index=0, oob=None):
        table, series = inputs
        if not self.built:
            self.build((series.shape[1], series.shape[2] * table.shape[1]))
            self.to(table.device)
        return Fn.CapsuleRouting.apply(table, series, self.S, self.B, self.routing_rounds, padding_index, oob)


class LabelAwareAttention(Layer):
    """6.MIND/CustomLayers.py:141-158 together with the inner products and the loss of MINDLayer.call (:267-285), which is
    where its output goes: the capsule weights are a masked softmax over the capsules' scores against every sampled item,
    ``output[b,s]`` the weighted capsule's inner product with item s, ``loss[b]`` the softmax cross entropy with the label
    at sample 0.  The item lookup is part of the kernel: the call takes the table, the stacked item ids [B,Ns,C], the
    capsules [B,K,C E] and the number of valid capsules int32 [B] (capsule k is masked iff k >= that number)."""

    def forward(self, table, items, mlped_capsules, valid_capsules_num, oob=None):
        return Fn.LabelAwareAttention.apply(table, items, mlped_capsules, valid_capsules_num, oob)


class MINDLayer(Layer):
    """6.MIND/CustomLayers.py:161-285.  ``seq_length`` (extension): the length T of the behaviour series; given, the
    extractor's ``S`` / ``B`` exist from construction (a state dict can be loaded), otherwise they are built by the first
    call.  ``generate_interest_capsules`` returns the capsule COUNT int32 [B] as ``valid_capsules_num`` (what
    save_interest_capsules casts the reference's fp32 log2 to; 0 where that is -inf), see mind_capsule_count_table."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["label_goods_ids", "label_shop_ids", "label_cate_ids"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=160000, embedding_dims=16, activation="ReLU", padding_index=0, capsules_num=4,
                 seq_length=None):
        super().__init__()
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.behavior_series_features = behavior_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.embed = Embedding(feature_dims, embedding_dims)
        capsules_dim = embedding_dims * len(item_categorical_features)
        ops.mind_check_shape(capsules_dim, capsules_dim, capsules_num)
        self.context_mlp = Dense(capsules_dim // 2, activation="sigmoid",
                                 input_dim=len(user_and_context_categorical_features) * embedding_dims)
        self.context_bn = BatchNormalization(input_dim=capsules_dim // 2)
        if isinstance(activation, str) and activation not in ("PReLU", "Dice", "None"):
            activation = activation.lower()              # Keras resolves 'ReLU' and 'relu' to the same function
        self.final_mlp = make_mlp_layer([capsules_dim * 4, capsules_dim], activation=activation,
                                        input_dim=capsules_dim // 2 + capsules_dim)
        self.padding_index = padding_index
        self.capsules_num = capsules_num
        self.MIE_layer = MultiInterestExtractorLayer(
            capsules_num=capsules_num, capsules_dim=capsules_dim,
            input_shape=None if seq_length is None else (seq_length, capsules_dim))
        self.LAA_layer = LabelAwareAttention()
        self._count_table = None

    def _capsule_counts(self, series):
        T = series.shape[1]
        if self._count_table is None or self._count_table.numel() != T + 1 or self._count_table.device != series.device:
            self._count_table = mind_capsule_count_table(T, self.capsules_num).to(series.device)
        n_valid = (series[:, :, 0] != self.padding_index).sum(dim=1)
        return self._count_table[n_valid]

    def _capsules(self, inputs, flag):
        device = self._device()
        series = _stack_ids(inputs, self.behavior_series_features, device)
        interest_capsules = self.MIE_layer((self.embed.embeddings, series), self.padding_index, flag)
        valid_capsules_num = self._capsule_counts(series)
        K = self.capsules_num
        capsules_mask = torch.arange(K, device=device)[None, :] >= valid_capsules_num[:, None]
        X_cate = assemble_index(inputs, self.user_and_context_categorical_features)
        profile = self.embed(X_cate, flag)
        profile_output = self.context_bn(self.context_mlp(profile.reshape(profile.shape[0], -1)))
        B, half = profile_output.shape
        concated = torch.cat([profile_output[:, None, :].expand(B, K, half), interest_capsules], dim=2)
        mlped_capsules = self.final_mlp(concated.reshape(B * K, -1)).reshape(B, K, -1)
        return mlped_capsules, capsules_mask, valid_capsules_num

    def generate_interest_capsules(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        result = self._capsules(inputs, flag)
        self._raise_if_oob(flag)
        return result

    def forward(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        mlped_capsules, _, valid_capsules_num = self._capsules(inputs, flag)
        items = _stack_ids(inputs, self.item_categorical_features, mlped_capsules.device)
        output, loss = self.LAA_layer(self.embed.embeddings, items, mlped_capsules, valid_capsules_num, flag)
        self._raise_if_oob(flag)
        return {"output": output, "loss": loss}


# ---------------------------------------------------------------------------------------------------
# ComiRec: multi-interest retrieval with hard attention (6.MIND/CustomLayers.py:528-866)
# ---------------------------------------------------------------------------------------------------

def comirec_positional_table(seq_length, d_model):
    """float32 [seq_length, d_model]: ComiRecSelfAttentiveLayer.positional_encoding (6.MIND/CustomLayers.py:625-642) as
    numpy float32 reads it, in that order of operations -- pos * (1 / 10000 ** (2 (i // 2) / d_model)), sin on the even
    columns and cos on the odd ones -- built once on the host (nobody here can run TensorFlow)."""
    import numpy as np
    pos = np.arange(int(seq_length), dtype=np.float32)[:, None]
    i = np.arange(int(d_model), dtype=np.float32)[None, :]
    rates = np.float32(1) / np.power(np.float32(10000.0), (np.float32(2) * np.floor_divide(i, np.float32(2)))
                                     / np.float32(d_model))
    angle = pos * rates
    assert angle.dtype == np.float32
    even = (np.arange(int(d_model)) % 2 == 0)[None, :]
    return torch.from_numpy(np.where(even, np.sin(angle), np.cos(angle)).astype(np.float32))


class ComiRecDynamicRoutingLayer(Layer):
    """6.MIND/CustomLayers.py:528-594: dynamic routing with one projection per capsule and position.  ``W``
    [capsules_num, T, D, capsules_dim] random_normal(stddev 0.05), trained; the routing logits ``B`` [capsules_num, T]
    zeros, a buffer (the reference's non-trainable weight).  squash as in MultiInterestExtractorLayer.
    The lookup is part of the kernel, so the call is ``layer((table, series), padding_index, keep_padding)`` with the
    embedding matrix [V,E] and the stacked ids [B,T,C] where the reference takes the looked-up behaviours and a mask in
    which True means "takes part": position t takes part iff ``(series[b,t,0] == padding_index) == keep_padding``.
    ``seq_length`` and ``embedding_dims`` (extensions; the latter is D = C E) build at construction."""

    def __init__(self, capsules_num, capsules_dim, routing_rounds=3, *, seq_length=None, embedding_dims=None):
        super().__init__()
        self.capsules_num = capsules_num
        self.capsules_dim = capsules_dim
        self.routing_rounds = routing_rounds
        self.built = False
        if seq_length is not None and embedding_dims is not None:
            self.build((seq_length, embedding_dims))

    def build(self, input_shape):
        T, D = (int(v) for v in tuple(input_shape)[-2:])
        ops.comirec_check_shape(D, self.capsules_dim, self.capsules_num, self.routing_rounds, T=T, mode="DR")
        self.W = torch.nn.Parameter(_initializer("random_normal")((self.capsules_num, T, D, self.capsules_dim)))
        self.register_buffer("B", torch.zeros(self.capsules_num, T))
        self.built = True

    def forward(self, inputs, padding_index=0, keep_padding=True, oob=None):
        table, series = inputs
        if not self.built:
            self.build((series.shape[1], series.shape[2] * table.shape[1]))
            self.to(table.device)
        return Fn.ComiRecRouting.apply(table, series, self.W, self.B, self.routing_rounds, padding_index,
                                       bool(keep_padding), oob)


class ComiRecSelfAttentiveLayer(Layer):
    """6.MIND/CustomLayers.py:597-665: ``tanh((behaviours + positional encoding) W1)``, ``capsules_num`` attention heads
    from ``W2``, a masked softmax over the positions and the weighted sum of the TRANSFORMED behaviours (the reference's
    choice, so that both extractors return [B, capsules_num, capsules_dim]).  ``W1`` [D, capsules_dim] and ``W2``
    [capsules_num, capsules_dim] glorot_normal; the positional table is a constant built once on the host
    (comirec_positional_table).  Called as ComiRecDynamicRoutingLayer."""

    def __init__(self, capsules_num, capsules_dim, add_pos_emb=True, *, seq_length=None, embedding_dims=None):
        super().__init__()
        self.capsules_num = capsules_num
        self.capsules_dim = capsules_dim
        self.add_pos_emb = add_pos_emb
        self.built = False
        self._pos = None
        if embedding_dims is not None:
            self.build((seq_length, embedding_dims))

    def build(self, input_shape):
        T, D = tuple(input_shape)[-2:]
        ops.comirec_check_shape(int(D), self.capsules_dim, self.capsules_num, T=None if T is None else int(T), mode="SA")
        self.W1 = torch.nn.Parameter(glorot_normal((int(D), self.capsules_dim)))
        self.W2 = torch.nn.Parameter(glorot_normal((self.capsules_num, self.capsules_dim)))
        self.built = True

    def _positions(self, T, D, device):
        if not self.add_pos_emb:
            return None
        if self._pos is None or tuple(self._pos.shape) != (T, D) or self._pos.device != device:
            self._pos = comirec_positional_table(T, D).to(device)
        return self._pos

    def forward(self, inputs, padding_index=0, keep_padding=True, oob=None):
        table, series = inputs
        T, D = series.shape[1], series.shape[2] * table.shape[1]
        if not self.built:
            self.build((T, D))
            self.to(table.device)
        return Fn.ComiRecSelfAttention.apply(table, series, self.W1, self.W2, self._positions(T, D, table.device),
                                             padding_index, bool(keep_padding), oob)


class ComiRecLayer(Layer):
    """6.MIND/CustomLayers.py:668-810.  ``forward`` returns ``{'output': the selected capsules [B,Ns,Dc], 'loss': [B]}``:
    every sampled item picks the capsule with the largest inner product (smallest index on a tie, tf.argmax) and the
    softmax cross entropy with the label at sample 0 runs over those inner products.
    Extensions, keyword-only: ``seq_length``, as in MINDLayer, builds the extractor's weights at construction;
    ``reference_mask``: the reference hands ``series == padding_index`` to an extractor whose mask means "takes part"
    (:714, :724), so read literally it routes over the PADDED positions -- True keeps that, False routes over the
    behaviours, which is what the paper and MINDLayer mean.
    ``negative_sample_type='auto'`` is tf.nn.sampled_softmax_loss with a random log-uniform sampler: nothing
    deterministic to mirror, NotImplementedError.  The greedy_search_inference methods and save_interest_capsules are
    host-side serving code and are not ported."""

    def __init__(self, item_categorical_features=["label_goods_ids", "label_shop_ids", "label_cate_ids"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=160000, embedding_dims=16, activation="ReLU", padding_index=0, capsules_num=4, mode="DR",
                 routing_rounds=3, add_pos_emb=True, negative_sample_type="manual", *, seq_length=None,
                 reference_mask=True):
        super().__init__()
        if negative_sample_type not in ("auto", "manual"):
            raise ValueError("negative_sample_type must be in ('auto','manual')")
        if negative_sample_type == "auto":
            raise NotImplementedError("negative_sample_type='auto' draws its negatives from tf.nn.sampled_softmax_loss' "
                                      "random log-uniform sampler; only 'manual' is implemented")
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.behavior_series_features = behavior_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.embed = Embedding(feature_dims, embedding_dims)
        capsules_dim = embedding_dims * len(item_categorical_features)
        self.padding_index = padding_index
        self.capsules_num = capsules_num
        self.reference_mask = bool(reference_mask)
        ops.comirec_check_shape(capsules_dim, capsules_dim, capsules_num)
        built = dict(seq_length=seq_length, embedding_dims=None if seq_length is None else capsules_dim)
        if mode == "DR":
            self.interest_extractor = ComiRecDynamicRoutingLayer(capsules_num, capsules_dim, routing_rounds, **built)
        elif mode == "SA":
            self.interest_extractor = ComiRecSelfAttentiveLayer(capsules_num, capsules_dim, add_pos_emb, **built)
        else:
            raise ValueError("mode must be in ('DR','SA')")
        self.negative_sample_type = negative_sample_type

    def _capsules(self, inputs, flag):
        series = _stack_ids(inputs, self.behavior_series_features, self._device())
        return self.interest_extractor((self.embed.embeddings, series), self.padding_index, self.reference_mask, flag)

    def generate_interest_capsules(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        interest_capsules = self._capsules(inputs, flag)
        self._raise_if_oob(flag)
        return interest_capsules

    def forward(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        interest_capsules = self._capsules(inputs, flag)
        items = _stack_ids(inputs, self.item_categorical_features, interest_capsules.device)
        selected, _, loss, _ = Fn.ComiRecSelect.apply(self.embed.embeddings, items, interest_capsules, flag)
        self._raise_if_oob(flag)
        return {"output": selected, "loss": loss}


class SINELayer(Layer):
    """6.MIND/CustomLayers.py:966-1176, the sparse-interest network: every example selects the K of L concepts of
    ``interest_pool`` closest to its attention-pooled series (tf.math.top_k: descending, the lower index first on equal
    values), each selection brings its own matrix ``Wk1[l]`` into a tanh-attention over the series, and the K interests are
    mixed by a softmax at temperature ``tau``.  ``forward`` returns ``{'user_interest': [B,D], 'main_loss': [B],
    'aux_loss': scalar}``; ``main_loss`` is the softmax cross entropy with the label at sample 0 over the inner products of
    the looked-up items with ``user_interest`` (the hard-attention kernel of ComiRec with one capsule).  Only the first
    attention masks padded positions, as in the reference; its LayerNormalization layers are built inside ``call`` and so
    never trained: no gamma, no beta, eps 1e-3.  The whole extractor is one launch each way (csrc/sine.hip).
    The one deliberate deviation: the reference writes the auxiliary loss as 0.5 square(norm), whose TF gradient is NaN
    when the off-diagonal of the pool's covariance is zero throughout (L = 1, say); here that gradient is zero."""

    def __init__(self, item_categorical_features=["label_goods_ids", "label_shop_ids", "label_cate_ids"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=160000, embedding_dims=16, padding_index=0, L=100, K=5, tau=0.1):
        super().__init__()
        assert len(item_categorical_features) == len(behavior_series_features)
        self.item_categorical_features = item_categorical_features
        self.behavior_series_features = behavior_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.L = L
        self.K = K
        self.D = D = len(item_categorical_features) * embedding_dims
        self.tau = tau
        ops.sine_check_shape(D, L, K)
        if not tau > 0:
            raise ValueError("tau must be positive, got %r" % (tau,))
        self.embed = Embedding(feature_dims, embedding_dims)
        normal = _initializer("random_normal")
        self.interest_pool = torch.nn.Parameter(normal((L, D)))
        self.W1 = torch.nn.Parameter(normal((D, D)))
        self.W2 = torch.nn.Parameter(normal((D,)))
        self.Wk1 = torch.nn.Parameter(normal((L, D, D)))
        self.Wk2 = torch.nn.Parameter(normal((L, D)))
        self.W3 = torch.nn.Parameter(normal((D, D)))
        self.W4 = torch.nn.Parameter(normal((D,)))
        self.padding_index = padding_index

    def _interest(self, inputs, flag):
        series = _stack_ids(inputs, self.behavior_series_features, self._device())
        return Fn.SineInterest.apply(self.embed.embeddings, series, self.interest_pool, self.W1, self.W2, self.Wk1,
                                     self.Wk2, self.W3, self.W4, self.K, self.tau, self.padding_index, flag)[0]

    def generate_user_interest(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        user_interest = self._interest(inputs, flag)
        self._raise_if_oob(flag)
        return user_interest

    def compute_auxiliary_loss(self):
        return Fn.SineAux.apply(self.interest_pool)

    def forward(self, inputs):
        flag = ops.new_flag(self._device()) if self.check_ids else None
        user_interest = self._interest(inputs, flag)
        items = _stack_ids(inputs, self.item_categorical_features, user_interest.device)
        _, _, main_loss, _ = Fn.ComiRecSelect.apply(self.embed.embeddings, items, user_interest[:, None, :], flag)
        self._raise_if_oob(flag)
        return {"user_interest": user_interest, "main_loss": main_loss, "aux_loss": self.compute_auxiliary_loss()}


class CoActionUnit(Layer):
    """7.SIM/CustomLayers.py:285-378, the CAN co-action: the induction row of the target item IS the weights and biases of
    a small MLP (layer l maps feed_feature_dim * coef_l to feed_feature_dim * coef_l+1 columns) that is applied to every
    feed feature of the example raised to the powers 1..order; a feed id equal to ``padding_index`` gives zeros.
    ``forward([induction_feature, feed_feature])`` returns the reference's list of ``order`` tensors: induction_feature
    [B] or [B,1]; feed_feature [B] (outputs [B, Eo]) or [B,T] (outputs [B,T,Eo]).  Both lookups and the MLP of every order
    are one launch (csrc/can.hip).  A reference quirk that is kept: the layers are zipped with a list of ``order``
    activations, so only min(len(layer_unit_coef), order) layers are applied and Eo is the width of the last one applied;
    the induction rows still hold every layer, the unused tail gets a zero gradient.  With ``order_independent=False``
    every order reads ONE table (state dict: only ``induction_embedding.0.embeddings``) and its gradient is the sum over
    the orders.  Activations: 'tanh', 'relu', 'sigmoid', 'linear' / None; anything else Keras knows: NotImplementedError.
    Extension: ``pooled([induction_feature, feed_feature])`` -> [B, Eo], the sum of the list over orders and positions
    (what CANLayer takes from its series co-action), fused: the list is never materialised."""

    def __init__(self, induction_feature_num=1000, feed_feature_num=1000, feed_feature_dim=16, layer_unit_coef=None,
                 order=3, order_independent=True, activation="tanh", padding_index=0):
        super().__init__()
        if layer_unit_coef is None:
            layer_unit_coef = [1, 1, 1]
        if activation not in ops.ACT_CODE:
            raise NotImplementedError("CoActionUnit implements the activations 'tanh', 'relu', 'sigmoid' and 'linear' / "
                                      "None, got %r" % (activation,))
        self.layer_unit_coef = [int(c) for c in layer_unit_coef]
        self.order = int(order)
        self.order_independent = bool(order_independent)
        self.act = ops.ACT_CODE[activation]
        self.padding_index = padding_index
        self.feed_feature_dim = int(feed_feature_dim)
        ops.can_check_shape(self.feed_feature_dim, self.layer_unit_coef, self.order)
        self.feed_embedding = Embedding(feed_feature_num, feed_feature_dim)
        induction_feature_dim = ops.can_row_floats(feed_feature_dim, self.layer_unit_coef)
        self.induction_embedding = torch.nn.ModuleList(
            [Embedding(induction_feature_num, induction_feature_dim)
             for _ in range(self.order if self.order_independent else 1)])    # not independent: one table, every order
        applied = min(len(self.layer_unit_coef), self.order)
        self.output_dim = ops.can_widths(feed_feature_dim, self.layer_unit_coef)[applied]

    def _ids(self, inputs):
        induction_feature, feed_feature = inputs
        dev = self._device()
        as_ids = lambda t: (t if isinstance(t, torch.Tensor) else torch.as_tensor(t)).to(device=dev, dtype=torch.int64)
        iid, fid = as_ids(induction_feature), as_ids(feed_feature)
        if iid.dim() == 2 and iid.shape[1] == 1:
            iid = iid.squeeze(1)
        if fid.dim() not in (1, 2):
            raise ValueError("feed_vector维度必须是2维或者3维")
        if iid.dim() != 1 or iid.shape[0] != fid.shape[0]:
            raise ValueError("induction_feature must be [B] or [B,1] with the batch of feed_feature, got %s and %s"
                             % (tuple(iid.shape), tuple(fid.shape)))
        return iid.contiguous(), fid.reshape(fid.shape[0], -1).contiguous(), fid.dim() == 1

    def _run(self, inputs, pooled):
        iid, fid, flat = self._ids(inputs)
        flag = ops.new_flag(iid.device) if self.check_ids else None
        res = Fn.CoAction.apply(self.feed_embedding.embeddings, iid, fid, self.layer_unit_coef, self.order, self.act,
                                self.padding_index, pooled, flag, *[e.embeddings for e in self.induction_embedding])
        self._raise_if_oob(flag)
        return res, flat

    def forward(self, inputs):
        out, flat = self._run(inputs, False)
        return [o[:, 0] if flat else o for o in out.unbind(0)]

    def pooled(self, inputs):
        return self._run(inputs, True)[0]


# ---------------------------------------------------------------------------------------------------
# 8.DMR: FinalMLP
# ---------------------------------------------------------------------------------------------------

def _keras_name(name):
    """Keras resolves 'ReLU' and 'relu' alike; the 8.DMR chapter spells the former.  'None' stays the chapter's "no such
    layer"."""
    return name.lower() if isinstance(name, str) and name.lower() in ops.DACT_CODE else name


class FeatureSelectionLayer(Layer):
    """8.DMR/CustomLayers.py:390-414.  ``forward([X_shared, X_item, X_user])``: gate 1 reads the ITEM ids through
    ``fs1_embedding``, gate 2 the USER ids through ``fs2_embedding``; a gate is g = 2 sigmoid(Dense(hidden(rows))), with
    ``hidden`` = make_mlp_layer(units[:-1], activation, norm) and units[-1] the width of X_shared -> (g1 (.) X_shared,
    g2 (.) X_shared).  ``input_dims`` = (item fields, user fields) (extension: layers are built eagerly)."""

    def __init__(self, fs1_feature_dims=160000, fs2_feature_dims=160000, fs1_emd_dim=16, fs2_emd_dim=16, fs1_units=None,
                 fs2_units=None, fs1_activation="ReLU", fs2_activation="ReLU", fs1_norm="None", fs2_norm="None",
                 input_dims=(5, 5)):
        super().__init__()
        fs1_units = [64, 160] if fs1_units is None else list(fs1_units)
        fs2_units = [64, 160] if fs2_units is None else list(fs2_units)
        self.fs1_embedding = Embedding(fs1_feature_dims, fs1_emd_dim)
        self.fs2_embedding = Embedding(fs2_feature_dims, fs2_emd_dim)
        d1, d2 = int(input_dims[0]) * int(fs1_emd_dim), int(input_dims[1]) * int(fs2_emd_dim)
        a1, a2 = _keras_name(fs1_activation), _keras_name(fs2_activation)
        self.mlp_gate1_hidden = make_mlp_layer(fs1_units[:-1], a1, fs1_norm, input_dim=d1)
        self.mlp_gate2_hidden = make_mlp_layer(fs2_units[:-1], a2, fs2_norm, input_dim=d2)
        self.mlp_gate1_output = make_mlp_layer(fs1_units[-1:], "sigmoid", fs1_norm, input_dim=(fs1_units[:-1] or [d1])[-1])
        self.mlp_gate2_output = make_mlp_layer(fs2_units[-1:], "sigmoid", fs2_norm, input_dim=(fs2_units[:-1] or [d2])[-1])

    def gate_rows(self, X_item, X_user, flag=None):
        """the flattened rows the two gates read: ([B, Fi fs1_emd_dim], [B, Fu fs2_emd_dim])"""
        return (self.fs1_embedding(X_item, flag).reshape(X_item.shape[0], -1),
                self.fs2_embedding(X_user, flag).reshape(X_user.shape[0], -1))

    def forward(self, inputs):
        X_shared, X_item, X_user = inputs
        flag = ops.new_flag(X_shared.device) if self.check_ids else None
        x1, x2 = self.gate_rows(X_item, X_user, flag)
        self._raise_if_oob(flag)
        g1 = self.mlp_gate1_output(self.mlp_gate1_hidden(x1)) * 2
        g2 = self.mlp_gate2_output(self.mlp_gate2_hidden(x2)) * 2
        return g1 * X_shared, g2 * X_shared


class DualPartsInteractionLayer(Layer):
    """8.DMR/CustomLayers.py:416-442: out = m1 W_1 + c_1 + m2 W_2 + c_2 + sum over heads of m1_h^T W_12[h] m2_h, no
    activation -> [B, output_dim].  ``W_12`` [num_heads, d1 / num_heads, d2 / num_heads, output_dim], glorot-uniform
    with Keras' rank-4 fans.  ``input_dims`` = (d1, d2) builds it eagerly; otherwise the first call does."""

    def __init__(self, num_heads=8, output_dim=1, input_dims=None):
        super().__init__()
        self.num_heads, self.output_dim = int(num_heads), int(output_dim)
        self.built = False
        if input_dims is not None:
            self.build(*input_dims)

    def build(self, dim1, dim2):
        dim1, dim2, n = int(dim1), int(dim2), self.num_heads
        if dim1 % n or dim2 % n:
            raise ValueError("输入维度必须被num_heads整除")
        self.head_dim1, self.head_dim2 = dim1 // n, dim2 // n
        self.W_1 = Dense(self.output_dim, input_dim=dim1)
        self.W_2 = Dense(self.output_dim, input_dim=dim2)
        self.W_12 = torch.nn.Parameter(glorot_uniform((n, self.head_dim1, self.head_dim2, self.output_dim)))
        self.built = True

    def forward(self, inputs):
        m1, m2 = inputs
        if not self.built:
            self.build(m1.shape[-1], m2.shape[-1])
            self.to(m1.device)
        n = self.num_heads
        t = torch.einsum("bnx,nxyo->bnyo", m1.reshape(-1, n, self.head_dim1), self.W_12)
        t = torch.einsum("bnyo,bny->bno", t, m2.reshape(-1, n, self.head_dim2)).sum(dim=1)
        return self.W_1(m1) + self.W_2(m2) + t


class FinalMLPLayer(Layer):
    """8.DMR/CustomLayers.py:319-387: the flattened shared rows of the user and item ids (users first) are gated twice
    (FeatureSelectionLayer: gate 1 from the item ids, gate 2 from the user ids), each gated copy runs through its own
    Dense -> BatchNormalization -> activation stream, and DualPartsInteractionLayer joins the two -> {'output': [B,
    output_dim]} after a sigmoid.  The constructor arguments and defaults are the reference's.

    ``fused`` ('auto' | True | False; extension): the fused path runs everything behind the three lookups on the kernels
    of csrc/finalmlp.hip (functional.FinalMLPBody).  It needs one ReLU hidden layer without a norm in both gates, ReLU +
    'batchnorm' streams of the same depth 1..4 and sizes inside the kernel limits; 'auto' takes it where that holds, True
    raises NotImplementedError where it does not.  The composed path strings the earlier entry points together (Dense,
    BatchNormalization, Activation, torch for the head's einsum) and serves every argument combination."""

    def __init__(self, user_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_features=["iid", "itag1", "itag2", "itag3", "itag4"], feature_dims=160000, embedding_dims=16,
                 fs1_feature_dims=160000, fs2_feature_dims=160000, fs1_emd_dim=16, fs2_emd_dim=16, fs1_hidden_units=[64],
                 fs2_hidden_units=[64], fs1_activation="ReLU", fs2_activation="ReLU", fs1_norm="None", fs2_norm="None",
                 mlp1_hidden_units=[64, 64, 64], mlp2_hidden_units=[64, 64, 64], mlp1_activation="ReLU",
                 mlp2_activation="ReLU", mlp1_norm="batchnorm", mlp2_norm="batchnorm", num_heads=8, output_dim=1,
                 fused="auto"):
        super().__init__()
        if fused not in ("auto", True, False):
            raise ValueError("fused is 'auto', True or False, got %r" % (fused,))
        self.user_features, self.item_features = list(user_features), list(item_features)
        Fu, Fi = len(self.user_features), len(self.item_features)
        D = (Fu + Fi) * int(embedding_dims)
        w1, w2 = [int(w) for w in mlp1_hidden_units], [int(w) for w in mlp2_hidden_units]
        if not w1 or not w2:
            raise ValueError("mlp1_hidden_units and mlp2_hidden_units must not be empty")
        if w1[-1] % int(num_heads) or w2[-1] % int(num_heads):
            raise ValueError("输入维度必须被num_heads整除")
        self.shared_embedding = Embedding(feature_dims, embedding_dims)
        self.fs_layer = FeatureSelectionLayer(
            fs1_feature_dims=fs1_feature_dims, fs2_feature_dims=fs2_feature_dims, fs1_emd_dim=fs1_emd_dim,
            fs2_emd_dim=fs2_emd_dim, fs1_units=list(fs1_hidden_units) + [D], fs2_units=list(fs2_hidden_units) + [D],
            fs1_activation=fs1_activation, fs2_activation=fs2_activation, fs1_norm=fs1_norm, fs2_norm=fs2_norm,
            input_dims=(Fi, Fu))
        self.mlp1 = make_mlp_layer(w1, _keras_name(mlp1_activation), mlp1_norm, input_dim=D)
        self.mlp2 = make_mlp_layer(w2, _keras_name(mlp2_activation), mlp2_norm, input_dim=D)
        self.interaction_layer = DualPartsInteractionLayer(num_heads, output_dim, input_dims=(w1[-1], w2[-1]))

        why = None                                           # what keeps this configuration off the fused path
        gates = [(list(fs1_hidden_units), fs1_activation, fs1_norm), (list(fs2_hidden_units), fs2_activation, fs2_norm)]
        streams = [(mlp1_activation, mlp1_norm), (mlp2_activation, mlp2_norm)]
        if any(len(u) != 1 or _keras_name(a) != "relu" or n != "None" for u, a, n in gates):
            why = "the fused FinalMLP path takes gates with exactly one hidden layer, ReLU and norm 'None'"
        elif any(_keras_name(a) != "relu" or n != "batchnorm" for a, n in streams) or len(w1) != len(w2):
            why = "the fused FinalMLP path takes ReLU + 'batchnorm' streams of the same depth"
        else:
            self._dims = (int(fs1_hidden_units[0]), int(fs2_hidden_units[0]), w1, w2, int(num_heads), int(output_dim))
            try:
                ops.finalmlp_check_shape(D, Fi * int(fs1_emd_dim), Fu * int(fs2_emd_dim), *self._dims)
            except NotImplementedError as e:
                why = str(e)
        if fused is True and why is not None:
            raise NotImplementedError(why)
        self.fused = why is None and fused is not False

    def _streams(self):
        """[(Dense, BatchNormalization)] of stream 1, then of stream 2 (fused configurations)"""
        return [(m.layers[i], m.layers[i + 1]) for m in (self.mlp1, self.mlp2) for i in range(0, len(m.layers), 3)]

    def packed_params(self):
        """The sub-layers' parameters laid end to end in the order of include/mi355rec.h (one concatenation per call;
        gradients flow back through its views)."""
        fs, il = self.fs_layer, self.interaction_layer
        ts = []
        for hid, outp in ((fs.mlp_gate1_hidden, fs.mlp_gate1_output), (fs.mlp_gate2_hidden, fs.mlp_gate2_output)):
            ts += [hid.layers[0].kernel, hid.layers[0].bias, outp.layers[0].kernel, outp.layers[0].bias]
        for dense, bn in self._streams():
            ts += [dense.kernel, dense.bias, bn.gamma, bn.beta]
        ts += [il.W_1.kernel, il.W_1.bias, il.W_2.kernel, il.W_2.bias, il.W_12]
        return torch.cat([t.reshape(-1) for t in ts])

    def forward(self, inputs):
        X_user = assemble_index(inputs, self.user_features)
        X_item = assemble_index(inputs, self.item_features)
        X_shared = torch.cat([X_user, X_item], dim=1)
        flag = ops.new_flag(X_shared.device) if self.check_ids else None
        xs = self.shared_embedding(X_shared, flag).reshape(X_shared.shape[0], -1)
        if self.fused:
            x1, x2 = self.fs_layer.gate_rows(X_item, X_user, flag)
            self._raise_if_oob(flag)
            bns = [bn for _, bn in self._streams()]
            moving = [bn.moving_mean for bn in bns] + [bn.moving_variance for bn in bns]
            out = Fn.FinalMLPBody.apply(xs, x1, x2, self.packed_params(), moving, self._dims, self.training,
                                        bns[0].epsilon, bns[0].momentum)
            return {"output": out}
        self._raise_if_oob(flag)
        part1, part2 = self.fs_layer([xs, X_item, X_user])
        out = self.interaction_layer((self.mlp1(part1), self.mlp2(part2)))
        return {"output": Fn.FeatAct.apply(out.contiguous(), ops.DACT_SIGMOID, None, None, None)}


# ---------------------------------------------------------------------------------------------------
# DMR (8.DMR/CustomLayers.py:76-316): item-to-item and user-to-item attention with an auxiliary match loss
# ---------------------------------------------------------------------------------------------------

def _dmr_attention(scores, valid):
    """softmax of ``scores`` [B,T] over the valid positions, 0 elsewhere (where(valid, s, -inf) then softmax, :243-244
    and :305-306); an example without a valid position gets zeros, where the reference's softmax of all -inf is NaN"""
    has = valid.any(dim=1, keepdim=True)
    masked = torch.where(valid, scores, torch.full_like(scores, -math.inf))
    masked = torch.where(has, masked, torch.zeros_like(scores))
    return torch.softmax(masked, dim=-1) * (valid & has).to(scores.dtype)


class DMRI2INetworkLayer(Layer):
    """8.DMR/CustomLayers.py:203-248: s_t = z . tanh(xi Wc + x_t We + pos_t Wp), softmax over the valid positions ->
    [sum_t a_t x_t, sum over the valid t of s_t], [B, D + 1].  ``input_dim`` (extension) is needed because layers are
    built eagerly.  ``b`` is created and never used, as in the reference (:219): it stays in the state dict and its
    gradient is None.  ``forward`` is the composed path in the reference's operation order."""

    def __init__(self, hidden_dim=48, input_dim=None):
        super().__init__()
        if input_dim is None:
            raise ValueError("DMRI2INetworkLayer needs input_dim")
        self.hidden_dim = hidden_dim
        self.Wc = torch.nn.Parameter(glorot_uniform((input_dim, hidden_dim)))
        self.Wp = torch.nn.Parameter(glorot_uniform((input_dim, hidden_dim)))
        self.We = torch.nn.Parameter(glorot_uniform((input_dim, hidden_dim)))
        self.b = torch.nn.Parameter(glorot_uniform((hidden_dim,)))
        self.z = torch.nn.Parameter(glorot_uniform((hidden_dim,)))

    def forward(self, inputs):
        X_series, pos_series, X_item, valid_mask = inputs
        pre = (X_item @ self.Wc)[:, None, :] + X_series @ self.We + (pos_series @ self.Wp)[None, :, :]
        scores = (self.z[None, None, :] * torch.tanh(pre)).sum(-1)                       # [B,T]
        score_sum = torch.where(valid_mask, scores, torch.zeros_like(scores)).sum(-1, keepdim=True)
        attention = _dmr_attention(scores, valid_mask)
        attention_output = (attention[:, :, None] * X_series).sum(1)
        return torch.cat([attention_output, score_sum], dim=1)


class DMRU2INetworkLayer(Layer):
    """8.DMR/CustomLayers.py:251-316: s_t = z . tanh(x_t We + pos_t Wp), av_t = a_t x_t, u = sum_t av_t -> ([u, u . xi]
    [B, D + 1], auxiliary_loss [B]).  The loss is always computed: ``stage == 'train' or 'eval'`` (:312) is always true
    in the reference, and so it is here whatever ``stage`` says.  With last = (number of valid positions) - 1 it sets
    av[last] against ov = sum_{t < last} av_t (the mask is range(T) < last, not validity, :277) and every negative
    against ov; tf.keras.losses.CosineSimilarity returns MINUS the cosine (:281-284), so the logits are (1 - cos) / 2,
    into the sigmoid cross entropy with label 1 and 0.  ``b`` is created and never used (:264).  An example without a
    valid position gives zeros (the reference fails there: gather_nd at -1)."""

    def __init__(self, hidden_dim=48, input_dim=None):
        super().__init__()
        if input_dim is None:
            raise ValueError("DMRU2INetworkLayer needs input_dim")
        self.hidden_dim = hidden_dim
        self.Wp = torch.nn.Parameter(glorot_uniform((input_dim, hidden_dim)))
        self.We = torch.nn.Parameter(glorot_uniform((input_dim, hidden_dim)))
        self.b = torch.nn.Parameter(glorot_uniform((hidden_dim,)))
        self.z = torch.nn.Parameter(glorot_uniform((hidden_dim,)))

    @staticmethod
    def _neg_cosine(p, q):
        """tf.keras.losses.CosineSimilarity(axis=-1): -sum(l2_normalize(p) l2_normalize(q)), epsilon 1e-12"""
        nrm = lambda v: v * torch.rsqrt(torch.clamp((v * v).sum(-1, keepdim=True), min=1e-12))
        return -(nrm(p) * nrm(q)).sum(-1)

    def compute_auxiliary_loss(self, attentioned_vectors, valid_mask, X_negative):
        B, T = valid_mask.shape
        n = valid_mask.sum(1)
        last = n - 1
        lv = attentioned_vectors[torch.arange(B, device=last.device), last.clamp(min=0)]
        new_mask = torch.arange(T, device=last.device)[None, :] < last[:, None]
        ov = (attentioned_vectors * new_mask[:, :, None].to(attentioned_vectors.dtype)).sum(1)
        pos_logits = (self._neg_cosine(lv, ov) + 1) / 2
        neg_logits = (self._neg_cosine(X_negative, ov[:, None, :].expand_as(X_negative)) + 1) / 2
        softplus = torch.nn.functional.softplus      # sigmoid CE: label 1 -> softplus(-x), label 0 -> softplus(x)
        loss = softplus(-pos_logits) + softplus(neg_logits).sum(-1)
        return torch.where(n > 0, loss, torch.zeros_like(loss))

    def forward(self, inputs):
        X_series, pos_series, X_item, valid_mask, stage, X_negative = inputs
        pre = X_series @ self.We + (pos_series @ self.Wp)[None, :, :]
        scores = (self.z[None, None, :] * torch.tanh(pre)).sum(-1)
        attention = _dmr_attention(scores, valid_mask)
        attentioned_vectors = attention[:, :, None] * X_series
        attention_output = attentioned_vectors.sum(1)
        inner_product = (attention_output * X_item).sum(-1, keepdim=True)
        auxiliary_loss = self.compute_auxiliary_loss(attentioned_vectors, valid_mask, X_negative)
        return torch.cat([attention_output, inner_product], dim=1), auxiliary_loss


class DMRLayer(Layer):
    """8.DMR/CustomLayers.py:76-200, Deep Match to Rank: the profile rows, an item-to-item attention of the candidate
    over the behaviour series and a user-to-item attention of the series alone, both with a trained positional table,
    into make_mlp_layer([200, 80], sigmoid_units=True); the u2i unit also yields the auxiliary match loss over the sampled
    negatives.  ``forward`` returns ``{'output': [B,1], 'auxiliary_loss': [B]}``; the reference nowhere says how the loss
    enters training.  The series length must equal ``max_length`` (pos_embed(tf.range(max_length)) is added to it, :181).
    ``fused=True`` (extension): everything behind the lookups of both units and of the loss is one launch each way
    (csrc/dmr.hip), and one profile lookup serves ``profile`` and the candidate's rows, its de-duplication shared with
    the series and negative lookups; ``fused=False`` composes the two sub-layers in torch.  The loss is computed in
    every stage, as in the reference (:312).  Padding in the middle of a series is not an error: last is still the
    number of valid positions minus one.
    The one deliberate deviation: an example whose series has no valid position makes the reference fail (gather_nd at
    index -1, a softmax of all -inf); here it yields zero attention vectors, score sum 0, inner product 0 and
    auxiliary loss 0, with zero gradients, and no row is read at position -1."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 negative_sample_features=["negative_goods_ids", "negative_shop_ids", "negative_cate_ids"],
                 feature_dims=160000, embedding_dims=16, activation="PReLU", padding_index=0, stage="train",
                 max_length=10, fused=True):
        super().__init__()
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features) == len(negative_sample_features), \
            "Features to be interacted should match in item and behavior/negative series"
        self.behavior_series_features = behavior_series_features
        self.negative_sample_features = negative_sample_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        D = len(item_categorical_features) * embedding_dims
        ops.dmr_check_shape(D, D, T=max_length, Nn=1)
        self.id_embed = Embedding(feature_dims, embedding_dims)
        self.max_length = max_length
        self.pos_embed = Embedding(max_length, D)
        n_profile = len(user_and_context_categorical_features) + len(item_categorical_features)
        self.mlp = make_mlp_layer([200, 80], activation=activation, sigmoid_units=True,
                                  input_dim=n_profile * embedding_dims + 2 * (D + 1))
        self.padding_index = padding_index
        self.stage = stage
        self.i2i_network = DMRI2INetworkLayer(D, input_dim=D)
        self.u2i_network = DMRU2INetworkLayer(D, input_dim=D)
        self.fused = fused

    def set_stage(self, stage):
        assert stage in ("train", "valid", "inference")
        self.stage = stage

    def forward(self, inputs):
        shape = tuple(getattr(inputs[self.behavior_series_features[0]], "shape", ()))
        if len(shape) == 2 and shape[1] != self.max_length:      # before anything is moved or launched
            raise ValueError("the behaviour series must have max_length = %d positions, got %d"
                             % (self.max_length, shape[1]))
        prof_names = self.user_and_context_categorical_features + self.item_categorical_features
        X_cate = assemble_index(inputs, prof_names)
        dev = X_cate.device
        series = _stack_ids(inputs, self.behavior_series_features, dev)
        negatives = _stack_ids(inputs, self.negative_sample_features, dev)
        B, T, Cn = series.shape
        if T != self.max_length:
            raise ValueError("the behaviour series must have max_length = %d positions, got %d" % (self.max_length, T))
        flag = ops.new_flag(dev) if self.check_ids else None
        n_item = len(self.item_categorical_features)
        i2i_net, u2i_net = self.i2i_network, self.u2i_network
        # one lookup serves both: the candidate item's rows are the tail of the profile rows (the reference looks the item
        # ids up a second time, :165-172 -- same values)
        sink = self.id_embed.grad_sink(X_cate) if self.fused else None
        profile = self.id_embed(X_cate, flag, sink)
        profile_output = profile.reshape(B, -1)
        X_item = profile[:, profile.shape[1] - n_item:, :].reshape(B, -1)
        pos_series = self.pos_embed.embeddings                   # pos_embed(tf.range(max_length)): the whole table
        if self.fused:
            i2i_vector, u2i_vector, auxiliary_loss = Fn.DmrMatch.apply(
                self.id_embed.embeddings, X_item, series, negatives, pos_series, i2i_net.Wc, i2i_net.Wp, i2i_net.We,
                i2i_net.z, u2i_net.Wp, u2i_net.We, u2i_net.z, self.padding_index, flag, sink)
        else:
            X_series = self.id_embed(series.reshape(B, T * Cn), flag).reshape(B, T, -1)
            X_negative = self.id_embed(negatives.reshape(B, -1), flag).reshape(B, negatives.shape[1], -1)
            valid_mask = series[:, :, 0] != self.padding_index
            i2i_vector = i2i_net([X_series, pos_series, X_item, valid_mask])
            u2i_vector, auxiliary_loss = u2i_net([X_series, pos_series, X_item, valid_mask, self.stage, X_negative])
        self._raise_if_oob(flag)
        X_combined = ConcatCols.apply(profile_output, i2i_vector, u2i_vector)
        return {"output": self.mlp(X_combined), "auxiliary_loss": auxiliary_loss}


# ---------------------------------------------------------------------------------------------------
# DIEN (5.DIN/CustomLayers.py:292-517): interest extractor, auxiliary loss, attention scores, interest evolution
# ---------------------------------------------------------------------------------------------------

def orthogonal(shape):
    """tf.keras.initializers.Orthogonal(): the Q of a normal matrix's QR decomposition, signs fixed by R's diagonal"""
    rows, cols = shape
    a = torch.randn((max(rows, cols), min(rows, cols)), generator=_init_gen)
    qm, r = torch.linalg.qr(a)
    qm = qm * torch.sign(torch.diagonal(r))[None, :]
    return (qm if rows >= cols else qm.t()).contiguous()


class GRU(Layer):
    """The weights of tf.keras.layers.GRU(units) under their Keras names -- ``kernel`` [input_dim, 3 units] (Glorot
    uniform), ``recurrent_kernel`` [units, 3 units] (orthogonal), ``bias`` [2, 3 units] (zeros; reset_after=True), gate
    order z, r, h -- and the composed recurrence in torch: ``forward(x, mask)`` returns every state [B,T,units]; where
    the mask is false the state is carried and is the output of that step (zero before the first valid step).
    DIENLayer runs these weights through csrc/dien.hip instead."""

    def __init__(self, units, input_dim=None):
        super().__init__()
        if input_dim is None:
            raise ValueError("GRU needs input_dim")
        self.units = units
        self.kernel = torch.nn.Parameter(glorot_uniform((input_dim, 3 * units)))
        self.recurrent_kernel = torch.nn.Parameter(orthogonal((units, 3 * units)))
        self.bias = torch.nn.Parameter(torch.zeros((2, 3 * units)))

    def forward(self, x, mask=None):
        B, T, _ = x.shape
        H = self.units
        h = x.new_zeros((B, H))
        outs = []
        for t in range(T):
            xi = x[:, t] @ self.kernel + self.bias[0]
            hi = h @ self.recurrent_kernel + self.bias[1]
            z = torch.sigmoid(xi[:, :H] + hi[:, :H])
            r = torch.sigmoid(xi[:, H:2 * H] + hi[:, H:2 * H])
            hh = torch.tanh(xi[:, 2 * H:] + r * hi[:, 2 * H:])
            hn = z * h + (1 - z) * hh
            h = hn if mask is None else torch.where(mask[:, t, None], hn, h)
            outs.append(h)
        return torch.stack(outs, 1)


class DienActivationLayer(Layer):
    """5.DIN/CustomLayers.py:292-317: scores = exp((gru_output W) . X_item) (.) ~mask over their row sum, NaN -> 0 -- as
    written the positions the mask passed in marks FALSE score, and DIENLayer passes the valid mask (see its
    ``mask_mode``).  A row with nothing selected scores zeros and sends no gradient through the scores (TensorFlow's
    gradient of the 0 / 0 would be NaN).  ``forward`` is the composed path; DIENLayer fuses it with the evolution."""

    def __init__(self, embedding_dims1, embedding_dims2=None, **kwargs):
        super().__init__()
        if not embedding_dims2:
            embedding_dims2 = embedding_dims1
        self.W = torch.nn.Parameter(torch.randn((embedding_dims2, embedding_dims1), generator=_init_gen) * 0.05)

    def forward(self, inputs):
        gru_output, X_item, mask = inputs
        product = ((gru_output @ self.W) * X_item[:, None, :]).sum(-1)
        masked = torch.exp(product) * (~mask).to(product.dtype)
        denominator = masked.sum(-1, keepdim=True)
        return masked / torch.where(denominator > 0, denominator, torch.ones_like(denominator))


class CustomGRUCell(Layer):
    """5.DIN/CustomLayers.py:320-359: one step of the attention GRU on inputs [x | a].  The inner GRUCell the reference
    creates is never built and owns no weights: it has no counterpart here.  ``units`` doubles as the input width."""

    def __init__(self, units, mode, **kwargs):
        super().__init__()
        self.units = units
        self.mode = mode
        self.state_size = units
        for g in ("r", "h") + (("z",) if mode == "AUGRU" else ()):
            setattr(self, "W_" + g, torch.nn.Parameter(glorot_uniform((units, units))))
            setattr(self, "U_" + g, torch.nn.Parameter(glorot_uniform((units, units))))
            setattr(self, "b_" + g, torch.nn.Parameter(torch.zeros(units)))

    def forward(self, inputs, states):
        h_prev = states[0]
        x = inputs[:, :self.units]
        a = inputs[:, self.units:]
        r = torch.sigmoid(x @ self.W_r + h_prev @ self.U_r + self.b_r)
        h_tilda = torch.tanh(x @ self.W_h + r * (h_prev @ self.U_h) + self.b_h)
        if self.mode == "AGRU":
            h = (1 - a) * h_prev + a * h_tilda
        elif self.mode == "AUGRU":
            u = torch.sigmoid(x @ self.W_z + h_prev @ self.U_z + self.b_z)
            u_hat = a * u
            h = (1 - u_hat) * h_prev + u_hat * h_tilda
        return h, [h]

    def weights(self):
        names = ("W_r", "U_r", "b_r", "W_h", "U_h", "b_h") + (("W_z", "U_z", "b_z") if self.mode == "AUGRU" else ())
        return [getattr(self, n) for n in names]


class DienGRU(Layer):
    """5.DIN/CustomLayers.py:362-386: the interest evolution over (gru_output, activation_scores) under the valid mask
    (a masked step carries the state) -> the final state [B, units].  AIGRU: a second Keras GRU on gru_output (.) scores;
    AGRU / AUGRU: CustomGRUCell.  ``forward`` is the composed path in torch; ``evolve`` is the fused one: scores and
    recurrence in one launch each way (csrc/dien.hip; AIGRU: the scores composed from the existing ops, then the dense
    mode of the GRU kernels)."""

    def __init__(self, units, mode, **kwargs):
        super().__init__()
        self.units = units
        self.mode = mode
        if mode == "AIGRU":
            self.gru = GRU(units, input_dim=units)
        elif mode in ["AGRU", "AUGRU"]:
            self.gru_cell = CustomGRUCell(units, mode)

    def forward(self, inputs, valid_mask):
        gru_input, activation_scores = inputs
        if self.mode == "AIGRU":
            return self.gru(gru_input * activation_scores[:, :, None], mask=valid_mask)[:, -1]
        x = torch.cat([gru_input, activation_scores[:, :, None]], dim=-1)
        h = gru_input.new_zeros((gru_input.shape[0], self.units))
        for t in range(gru_input.shape[1]):
            hn, _ = self.gru_cell(x[:, t], [h])
            h = torch.where(valid_mask[:, t, None], hn, h)
        return h

    def evolve(self, gru_output, X_item, activation, series, padding_index, mask_valid):
        """gru_output [B,T,H], the candidate's rows [B,H], the DienActivationLayer and the series ids [B,T,C]"""
        if self.mode == "AIGRU":
            valid = series[:, :, 0] != padding_index
            scores = activation((gru_output, X_item, valid if mask_valid == 0 else ~valid))
            _, final, _ = Fn.DienGru.apply(None, None, None, gru_output * scores[:, :, None],
                                           series[:, :, 0].contiguous(), self.gru.kernel, self.gru.recurrent_kernel,
                                           self.gru.bias, padding_index)
            return final
        final, _ = Fn.DienAugru.apply(gru_output, X_item, activation.W, series, ops.DIEN_MODE[self.mode], padding_index,
                                      mask_valid, *self.gru_cell.weights())
        return final


class DIENLayer(Layer):
    """5.DIN/CustomLayers.py:389-517, Deep Interest Evolution Network: the profile rows and the evolved interest into
    make_mlp_layer([200, 80], softmax_units=2).  The interest extractor is a masked Keras GRU over the looked-up
    behaviour series (``gru``); in stage 'train' its states are scored against the next behaviour and a sampled negative
    (``auxiliary_loss``, a scalar summed over the batch, oddities kept: p and n pass through a sigmoid BEFORE the
    sigmoid cross entropy; 0, a Python number, in stage 'inference', which never reads the negative features);
    DienActivationLayer scores the states against the candidate and DienGRU evolves them.  ``forward`` returns
    ``{'X_combined', 'output', 'auxiliary_loss'}``; the reference nowhere adds the auxiliary loss to its training loss
    (INTEGRATION.md shows how to).
    ``mask_mode`` (extension, as DINLayer's): 'reference' keeps the activation's mask as written -- only PADDED positions
    score.  With AGRU / AUGRU every valid step then has a = 0 and every padded step is skipped, so the evolved interest
    is exactly zero whatever the weights, and ``dien_activation_layer.W`` and the cell get exactly zero gradient;
    'valid' scores the valid positions.  ``fused`` (extension): True runs csrc/dien.hip -- series lookup + GRU + auxiliary
    loss in one launch each way, scores + AGRU / AUGRU in another -- and one profile lookup serves ``profile`` and the
    candidate's rows, its de-duplication shared with the series and negative lookups; False composes the sub-layers in
    torch."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 negative_sample_features=["negative_goods_ids", "negative_shop_ids", "negative_cate_ids"],
                 feature_dims=160000, embedding_dims=16, activation="Dice", padding_index=0, mode="AUGRU", stage="train",
                 mask_mode="reference", fused=True):
        super().__init__()
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features) == len(negative_sample_features), \
            "Features to be interacted should match in item and behavior/negative series"
        self.behavior_series_features = behavior_series_features
        self.negative_sample_features = negative_sample_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        if mask_mode not in ("reference", "valid"):
            raise ValueError("mask_mode must be 'reference' or 'valid'")
        self.mask_mode = mask_mode
        H = len(behavior_series_features) * embedding_dims
        ops.dien_check_shape(H)
        self.embed = Embedding(feature_dims, embedding_dims)
        self.gru = GRU(H, input_dim=H)
        self.dien_activation_layer = DienActivationLayer(embedding_dims1=H)
        assert mode in ("AIGRU", "AGRU", "AUGRU")
        self.mode = mode
        self.dien_gru = DienGRU(H, mode)
        n_profile = len(user_and_context_categorical_features) + len(item_categorical_features)
        self.mlp = make_mlp_layer([200, 80], activation=activation, softmax_units=2,
                                  input_dim=n_profile * embedding_dims + H)
        self.padding_index = padding_index
        self.stage = stage
        self.fused = fused

    def set_stage(self, stage):
        assert stage in ("train", "inference")
        self.stage = stage

    def get_auxiliary_loss(self, X_series, gru_output, X_negative, valid_mask):
        X_series, gru_output, X_negative = X_series[:, :-1], gru_output[:, 1:], X_negative[:, 1:]
        pos_logits = torch.sigmoid((X_series * gru_output).sum(-1))
        neg_logits = torch.sigmoid((X_series * X_negative).sum(-1))
        sce = lambda v, label: torch.clamp(v, min=0) - v * label + torch.log1p(torch.exp(-v.abs()))
        mask = valid_mask[:, 1:].to(X_series.dtype)
        return (sce(pos_logits, 1.0) * mask).sum() + (sce(neg_logits, 0.0) * mask).sum()

    def body(self, X_series, X_negative, X_item, valid_mask):
        """The composed layer between the lookups and the MLP, in torch (any device): X_series [B,T,H], X_negative
        [B,T,H] or None (stage 'inference'), X_item [B,H], valid_mask [B,T] -> (evolved interest [B,H], auxiliary loss)"""
        gru_output = self.gru(X_series, mask=valid_mask)
        if self.stage == "train":
            auxiliary_loss = self.get_auxiliary_loss(X_series, gru_output, X_negative, valid_mask)
        else:
            auxiliary_loss = 0
        mask = valid_mask if self.mask_mode == "reference" else ~valid_mask
        activation_scores = self.dien_activation_layer((gru_output, X_item, mask))
        return self.dien_gru((gru_output, activation_scores), valid_mask), auxiliary_loss

    def forward(self, inputs):
        prof_names = self.user_and_context_categorical_features + self.item_categorical_features
        X_cate = assemble_index(inputs, prof_names)
        dev = X_cate.device
        series = _stack_ids(inputs, self.behavior_series_features, dev)
        train = self.stage == "train"
        negatives = _stack_ids(inputs, self.negative_sample_features, dev) if train else None
        B, T, Cn = series.shape
        if negatives is not None and tuple(negatives.shape) != (B, T, Cn):
            raise ValueError("the negative samples must have the behaviour series' shape %s, got %s"
                             % ((B, T), tuple(negatives.shape[:2])))
        ops.dien_check_shape(Cn * self.embedding_dims, T, ops.DIEN_MODE.get(self.mode))
        flag = ops.new_flag(dev) if self.check_ids else None
        n_item = len(self.item_categorical_features)
        # one lookup serves both: the candidate item's rows are the tail of the profile rows (the reference looks the item
        # ids up a second time, :471-478 -- same values)
        sink = self.embed.grad_sink(X_cate) if self.fused else None
        profile = self.embed(X_cate, flag, sink)
        profile_output = profile.reshape(B, -1)
        X_item = profile[:, profile.shape[1] - n_item:, :].reshape(B, -1)
        if self.fused:
            mask_valid = 1 if self.mask_mode == "valid" else 0
            gru_output, _, aux = Fn.DienGru.apply(self.embed.embeddings, series, negatives, None, None, self.gru.kernel,
                                                  self.gru.recurrent_kernel, self.gru.bias, self.padding_index, flag,
                                                  sink, X_item)
            auxiliary_loss = aux if train else 0
            evolved = self.dien_gru.evolve(gru_output, X_item, self.dien_activation_layer, series, self.padding_index,
                                           mask_valid)
        else:
            X_series = self.embed(series.reshape(B, T * Cn), flag).reshape(B, T, -1)
            X_negative = self.embed(negatives.reshape(B, T * Cn), flag).reshape(B, T, -1) if train else None
            evolved, auxiliary_loss = self.body(X_series, X_negative, X_item, series[:, :, 0] != self.padding_index)
        self._raise_if_oob(flag)
        X_combined = ConcatCols.apply(profile_output, evolved)
        return {"X_combined": X_combined, "output": self.mlp(X_combined), "auxiliary_loss": auxiliary_loss}


class _EinsumDense(Layer):
    """One projection of Keras' MultiHeadAttention: ``kernel`` (rank 3, glorot_uniform) and ``bias`` (zeros)"""

    def __init__(self, kernel_shape, bias_shape):
        super().__init__()
        self.kernel = torch.nn.Parameter(glorot_uniform(tuple(kernel_shape)))
        self.bias = torch.nn.Parameter(torch.zeros(tuple(bias_shape)))


class MultiHeadAttention(Layer):
    """tf.keras.layers.MultiHeadAttention(num_heads, key_dim) of Keras 2.x with value_dim = key_dim, no dropout and the
    output width of the query, built eagerly for ``input_dim``-wide queries, keys and values.  Sub-modules
    ``_query_dense``, ``_key_dense``, ``_value_dense`` (kernel [D,H,dk], bias [H,dk]) and ``_output_dense`` (kernel
    [H,dk,D], bias [D]): Keras' checkpoint names with '/' -> '.'.  ``forward(query [B,1,D], value [B,K,D], key=None,
    attention_mask=[B,1,K] bool)`` -> [B,1,D]: one query over K keys, the case the reference uses.  The mask is Keras'
    additive one, float32(logit + (1 - mask) * -1e9) -- a row with every position masked attends uniformly.  GPU
    tensors with key = value run csrc/sim.hip; anything else runs ``composed``, the einsum form of Keras in torch."""

    def __init__(self, num_heads, key_dim, input_dim):
        super().__init__()
        self.num_heads, self.key_dim, self.input_dim = num_heads, key_dim, input_dim
        D, H, dk = input_dim, num_heads, key_dim
        self._query_dense = _EinsumDense((D, H, dk), (H, dk))
        self._key_dense = _EinsumDense((D, H, dk), (H, dk))
        self._value_dense = _EinsumDense((D, H, dk), (H, dk))
        self._output_dense = _EinsumDense((H, dk, D), (D,))

    def weights(self):
        return tuple(t for m in (self._query_dense, self._key_dense, self._value_dense, self._output_dense)
                     for t in (m.kernel, m.bias))

    def composed(self, query, value, key=None, attention_mask=None):
        key = value if key is None else key
        Wq, bq, Wk, bk, Wv, bv, Wo, bo = self.weights()
        q = torch.einsum("bqd,dhk->bqhk", query, Wq) + bq
        k = torch.einsum("bjd,dhk->bjhk", key, Wk) + bk
        v = torch.einsum("bjd,dhk->bjhk", value, Wv) + bv
        q = q * (1.0 / math.sqrt(float(self.key_dim)))
        logits = torch.einsum("bjhk,bqhk->bhqj", k, q)
        if attention_mask is not None:
            logits = logits + (1.0 - attention_mask[:, None].to(logits.dtype)) * -1e9
        p = torch.softmax(logits, -1)
        o = torch.einsum("bhqj,bjhk->bqhk", p, v)
        return torch.einsum("bqhk,hkd->bqd", o, Wo) + bo

    def forward(self, query, value, key=None, attention_mask=None, fused=True):
        if query.dim() != 3 or query.shape[1] != 1 or value.dim() != 3:
            raise ValueError("MultiHeadAttention takes one query [B,1,D] over value [B,K,D], got %s and %s"
                             % (tuple(query.shape), tuple(value.shape)))
        if not (fused and query.is_cuda and (key is None or key is value)):
            return self.composed(query, value, key, attention_mask)
        B, K, D = value.shape
        ops.sim_check_shape(D, None, K, self.num_heads, self.key_dim)
        if attention_mask is None:
            mask = torch.ones((B, K), dtype=torch.int32, device=value.device)
        else:
            mask = attention_mask.reshape(B, K)
        return Fn.EsuAttention.apply(query[:, 0], value, mask, *self.weights()).unsqueeze(1)


class ESULayer(Layer):
    """7.SIM/CustomLayers.py:130-201 (exact search unit): a frozen DIENLayer's ``X_combined`` beside a multi-head
    attention of the candidate item over the K extracted behaviours, into make_mlp_layer([200, 80], softmax_units=2).
    ``forward`` reads ``inputs['extracted_series']`` [B,K,D] and ``inputs['series_mask']`` [B,K] (True = padded), as the
    reference does, and returns ``{'output'}``.
    Extensions, after the reference's arguments: ``dien_layer`` -- a trained DIENLayer to embed (what the reference's
    commented load_weights line intends); None builds DIENLayer(stage='inference') with its own defaults.  It is frozen
    (requires_grad False, run under no_grad and in eval mode, absent from ``trainable_variables``, present in
    ``state_dict()``).  ``mask_mode``: 'reference' passes series_mask as Keras' attention_mask as written, so only PADDED
    selections are attended (with all K selections valid every logit is masked and the attention is the uniform mean of
    the values); 'valid' attends the valid selections.  ``fused``: True runs csrc/sim.hip, False the torch composition."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=1000, embedding_dims=16, activation="Dice", padding_index=0, num_heads=8,
                 embedding_layer=None, l2_reg=0.01, dien_layer=None, mask_mode="reference", fused=True):
        super().__init__()
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.behavior_series_features = behavior_series_features
        self.feature_dims = feature_dims
        self.embedding_dims = embedding_dims
        self.l2_reg = l2_reg
        if mask_mode not in ("reference", "valid"):
            raise ValueError("mask_mode must be 'reference' or 'valid'")
        self.mask_mode = mask_mode
        self.fused = fused
        self.embed = embedding_layer if embedding_layer is not None else Embedding(feature_dims, embedding_dims)
        D = len(behavior_series_features) * embedding_dims
        if fused:
            ops.sim_check_shape(D, None, None, num_heads, D)
        self.dien_layer = dien_layer if dien_layer is not None else DIENLayer(stage="inference")
        self.dien_layer.set_stage("inference")
        self.dien_layer.requires_grad_(False)
        self.dien_layer.eval()
        dien_width = self.dien_layer.mlp.layers[0].kernel.shape[0]          # the width of DIEN's X_combined
        self.mlp = make_mlp_layer([200, 80], activation=activation, softmax_units=2, input_dim=dien_width + D)
        self.padding_index = padding_index
        self.mha = MultiHeadAttention(num_heads=num_heads, key_dim=D, input_dim=D)

    def train(self, mode=True):
        super().train(mode)
        self.dien_layer.eval()                               # Keras: trainable = False also means inference mode
        return self

    def head(self, inputs, X_item, extracted_series, series_mask):
        """everything after the item lookup: X_item [B,D] -> the layer's output"""
        with torch.no_grad():
            dien_output = self.dien_layer(inputs)["X_combined"]
        attend = series_mask if self.mask_mode == "reference" else ~series_mask
        mha_interest = self.mha(X_item.unsqueeze(1), extracted_series, attention_mask=attend.unsqueeze(1),
                                fused=self.fused).squeeze(1)
        X_combined = ConcatCols.apply(dien_output, mha_interest)
        return self.mlp(X_combined)

    def forward(self, inputs):
        X_item = assemble_index(inputs, self.item_categorical_features)
        flag = ops.new_flag(X_item.device) if self.check_ids else None
        q = self.embed(X_item, flag)
        self._raise_if_oob(flag)
        series_mask = inputs["series_mask"].to(device=X_item.device, dtype=torch.bool)
        x = inputs["extracted_series"].to(device=X_item.device, dtype=torch.float32)
        return {"output": self.head(inputs, q.reshape(q.shape[0], -1), x, series_mask)}


class SIMLayer(Layer):
    """7.SIM/CustomLayers.py:203-282, search-based interest model: the general search unit's pooling head, the soft
    search for the ``k`` behaviours that score highest against the candidate (a padded step ranks as -inf; ties go to the
    lower index, tf.argsort's order), and the exact search unit over them.  One shared table: ``embed``,
    ``gsu_layer.embed`` and ``esu_layer.embed`` are the same module.  ``forward`` returns ``{'gsu_logits',
    'esu_logits'}``, both [B,2] tensors -- in the reference 'esu_logits' is the ESU's result dict, which its own train
    loop cannot consume -- and does not write 'extracted_series' / 'series_mask' into the caller's ``inputs``, as the
    reference does.
    Extensions, after the reference's arguments: ``mask_mode`` and ``dien_layer`` are ESULayer's; ``fused`` = True makes
    ONE item lookup (the reference's three read the same rows), ONE search launch each way that yields the GSU pooling,
    the top k and their rows, and ONE attention launch; the series' gradient -- through the pooling and through the
    selected rows -- leaves through one buffer and one de-duplication plan shared with the item lookup.  False composes
    GSULayer(return_series=True), torch.sort(stable=True, descending=True), a gather and the composed attention."""

    def __init__(self, user_and_context_categorical_features=["uid", "utag1", "utag2", "utag3", "utag4"],
                 item_categorical_features=["i_goods_id", "i_shop_id", "i_cate_id"],
                 behavior_series_features=["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"],
                 feature_dims=1000, embedding_dims=16, activation="Dice", padding_index=0, k=3, l2_reg=0.01,
                 mask_mode="reference", fused=True, dien_layer=None):
        super().__init__()
        assert len(item_categorical_features) == len(behavior_series_features), \
            "Features to be interacted should match in item and behavior series"
        self.user_and_context_categorical_features = user_and_context_categorical_features
        self.item_categorical_features = item_categorical_features
        self.behavior_series_features = behavior_series_features
        self.embedding_dims = embedding_dims
        self.padding_index = padding_index
        self.fused = fused
        self.embed = Embedding(feature_dims, embedding_dims)
        self.gsu_layer = GSULayer(item_categorical_features=item_categorical_features,
                                  behavior_series_features=behavior_series_features, feature_dims=feature_dims,
                                  embedding_dims=embedding_dims, activation=activation, padding_index=padding_index,
                                  embedding_layer=self.embed, return_series=True)
        self.esu_layer = ESULayer(user_and_context_categorical_features=user_and_context_categorical_features,
                                  item_categorical_features=item_categorical_features,
                                  behavior_series_features=behavior_series_features, feature_dims=feature_dims,
                                  embedding_dims=embedding_dims, activation=activation, padding_index=padding_index,
                                  embedding_layer=self.embed, dien_layer=dien_layer, mask_mode=mask_mode, fused=fused)
        self.k = k

    def soft_index_search(self, X_item, X_series, valid_mask):
        inner_products = torch.einsum("be,ble->bl", X_item, X_series)
        inner_products = torch.where(valid_mask, inner_products, torch.full_like(inner_products, -math.inf))
        order = torch.sort(inner_products, dim=-1, descending=True, stable=True).indices[:, :self.k]
        top_k_embeddings = torch.gather(X_series, 1, order.unsqueeze(-1).expand(-1, -1, X_series.shape[2]))
        return top_k_embeddings, torch.gather(valid_mask, 1, order)

    def forward(self, inputs):
        X_item = assemble_index(inputs, self.item_categorical_features)
        flag = ops.new_flag(X_item.device) if self.check_ids else None
        if not self.fused:
            gsu_output = self.gsu_layer(inputs)
            q = self.embed(X_item, flag)
            q = q.reshape(q.shape[0], -1)
            self._raise_if_oob(flag)
            sel, sel_valid = self.soft_index_search(q, gsu_output["X_series"], gsu_output["valid_mask"])
            return {"gsu_logits": gsu_output["output"], "esu_logits": self.esu_layer.head(inputs, q, sel, ~sel_valid)}
        sink = self.embed.grad_sink(X_item)                  # the series lookup shares the item lookup's de-duplication
        q = self.embed(X_item, flag, sink)
        q = q.reshape(q.shape[0], -1)
        series = _stack_ids(inputs, self.behavior_series_features, X_item.device)
        ops.sim_check_shape(q.shape[1], series.shape[1], min(self.k, series.shape[1]), C=series.shape[2])
        pooled, sel, sel_valid, _, _ = Fn.SimSearch.apply(self.embed.embeddings, q, series, self.padding_index, self.k,
                                                          flag, sink)
        self._raise_if_oob(flag)
        gsu_logits = self.gsu_layer.mlp(ConcatCols.apply(q, pooled))
        return {"gsu_logits": gsu_logits, "esu_logits": self.esu_layer.head(inputs, q, sel, sel_valid == 0)}
