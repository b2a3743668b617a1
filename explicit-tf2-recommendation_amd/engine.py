"""Train-step engines: the reference's ``train_loop`` (2.FM/ModelManager.py:171-181) for one layer family as a
fixed sequence of C-ABI calls over preallocated device buffers.

    GradientTape -> model(inputs) -> BinaryCrossentropy -> tape.gradient -> (optionally) Adam.apply_gradients

Nothing is allocated and nothing synchronises inside a step, so a step can be captured once into a hipGraph
(``torch.cuda.CUDAGraph``) and replayed: the launch-bound chain of small kernels then costs one graph launch on
the host.  Gradients come out exactly as the autograd path of layers.py produces them (dense tensors for dense
parameters; (uniq_ids, rows, n_uniq) for the tables) -- tests/test_gpu_engine.py holds the two paths equal.
"""
import collections
import contextlib
import ctypes as C
import gc
import math
import operator
import weakref

import torch

from . import ops
from ._lib import lib, check, DeepFMLazyAdam


# Adam's constants: the defaults of tf.keras.optimizers.Adam, the reference's optimizer
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-7

# Stream captures use the thread-local error mode: with a process group alive, ProcessGroupNCCL's watchdog thread polls
# the events of finished collectives (hipEventQuery) whenever it likes, and in the default global mode such a call from
# ANOTHER thread during a capture invalidates the capture and terminates the process ("operation not permitted when
# stream is capturing") -- seen in bench.py --sharded, where graphs are captured after collectives have run.
CAPTURE_MODE = "thread_local"


@contextlib.contextmanager
def _no_cyclic_gc():
    """Collect what is dead now, then keep Python's cyclic collector off until the block ends.  For stream captures: a
    step that is no longer used is usually part of a reference cycle (a ModelManager and the closures it hands to its
    step), so its CUDAGraph dies whenever the collector happens to run -- in whichever thread allocates the object that
    trips its threshold, the autograd thread of a captured backward included.  Destroying a CUDAGraph is not a
    capture-safe operation (the ROCm build waits for the device in the destructor): with the collector firing inside
    the captured backward of a GraphedTrainStep, built after a few managers had been dropped, the process aborts.
    (torch.cuda.graph used to collect before every capture; it no longer does.)  Objects that die by reference
    counting inside the block are not affected.  A caller that has switched the collector off itself (a benchmark
    around its timed region) has already excluded the hazard: nothing is collected and nothing is changed then.
    gc.disable() / gc.enable() act on the whole process: the collector is off for every thread while a capture runs, and
    a thread that switches it off in the meantime finds it on again afterwards.  The train loops of this package drive
    their steps from one thread; a program that manages the collector from several must serialise that itself."""
    if not gc.isenabled():
        yield
        return
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        gc.enable()


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph(graph) in this module's capture mode, with the cyclic collector out of the way."""
    with _no_cyclic_gc():
        with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
            yield


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Program:
    """A recorded list of (name, fn, args) C-ABI calls; ``run(stream)`` enqueues them in order."""

    def __init__(self):
        self.calls = []

    def add(self, name, *args):
        self.calls.append((name, getattr(lib, name), args))

    def run(self, stream):
        for name, fn, args in self.calls:
            st = fn(*args, stream)
            if st != 0:
                check(st, name)


def _tables_share_rows(embed, w):
    """embed [V,E] and w [V,1] are the two strided views of one fused [V,ld] array (layers._FMTables.fuse_tables)."""
    E = embed.shape[1]
    return (embed.is_cuda and E % 4 == 0 and embed.stride(0) == w.stride(0) and embed.stride(0) % 4 == 0
            and embed.stride(0) >= E + 1 and w.data_ptr() == embed.data_ptr() + 4 * E and embed.data_ptr() % 16 == 0)


def _deepfm_dense(F, u1=32, u2=8, E=16):
    """The dense parameters of DeepFMRankingLayer, (name, shape) in the order every step keeps them: the order of
    ``g``, of the post launch's gradient array and of ShardedDeepFMStep's flat buffer."""
    return (("MLP_layer1.kernel_0", (F * E, u1)), ("MLP_layer1.bias_0", (u1,)), ("MLP_layer1.kernel_1", (u1, u2)),
            ("MLP_layer1.bias_1", (u2,)), ("MLP_layer2.kernel_0", (u2, 1)), ("MLP_layer2.bias_0", (1,)), ("bias", (1,)))


def _deepfm_ptr_arrays(layer, k0t, g):
    """The two host pointer arrays of the fused launches: the weights bias, K0, K0T, b0, K1, b1, K2, b2 of
    rec_deepfm_fused3_main_f32 and the gradients ``g`` of rec_deepfm_fused_post_f32.  Built once per step object:
    parameters, the transposed copy and gradients are updated in place."""
    params, names = dict(layer.named_parameters()), list(g)
    w = [params["bias"], params[names[0]], k0t.buf] + [params[n] for n in names[1:6]]
    return (C.c_void_p * 8)(*[t.data_ptr() for t in w]), (C.c_void_p * 7)(*[t.data_ptr() for t in g.values()])


def _deepfm_gradients(step):
    """Dense grads by parameter name + the two tables' (uniq_ids, rows, n_uniq)."""
    out = dict(step.g)
    out["embed.embeddings"] = (step.uniq_ids, step.g_embed_rows, step.n_uniq)
    out["w.embeddings"] = (step.uniq_ids, step.g_w_rows, step.n_uniq)
    return out


def _deepfm_host_adam(layer, g, state, uniq_ids, g_embed_rows, g_w_rows, n_uniq, side_e, side_w, optimizer, t, lr, st,
                      after_dense=None):
    """Adam on a DeepFM layer with the 1-based step ``t`` as a host scalar: the dense parameters one by one
    (``after_dense()`` runs behind them), then both tables -- 'keras_adam': the reference's dense sweep, as ONE sweep over
    the fused [embed | w | pad] rows where the tables share them; otherwise the touched rows only."""
    b1, b2, eps = ADAM_B1, ADAM_B2, ADAM_EPS
    params = dict(layer.named_parameters())
    for name, grad in g.items():
        m, v = state[name]
        check(lib.rec_adam_dense_f32(_p(params[name]), _p(m), _p(v), _p(grad), grad.numel(), t, lr, b1, b2, eps, st),
              "rec_adam_dense_f32")
    if after_dense is not None:
        after_dense()
    n = uniq_ids.numel()
    pe, pw = params["embed.embeddings"], params["w.embeddings"]
    V, E = pe.shape
    if optimizer == "keras_adam" and _tables_share_rows(pe, pw):
        (me, ve), (mw, vw) = state["embed.embeddings"], state["w.embeddings"]
        check(lib.rec_adam_sparse_keras_pair_f32(_p(pe), pe.stride(0), _p(me), _p(ve), _p(mw), _p(vw), V, E, _p(uniq_ids),
                                                 _p(g_embed_rows), _p(g_w_rows), _p(n_uniq), n, _p(side_e), _p(side_w), t,
                                                 lr, b1, b2, eps, st), "rec_adam_sparse_keras_pair_f32")
        return
    for p, rows, side in ((pe, g_embed_rows, side_e), (pw, g_w_rows, side_w)):
        m, v = state["embed.embeddings" if p is pe else "w.embeddings"]
        if optimizer == "keras_adam":
            check(lib.rec_adam_sparse_keras_f32(_p(p), p.stride(0), _p(m), _p(v), V, p.shape[1], _p(uniq_ids), _p(rows),
                                                _p(n_uniq), n, _p(side), t, lr, b1, b2, eps, st),
                  "rec_adam_sparse_keras_f32")
        else:
            check(lib.rec_adam_rows_f32(_p(p), p.stride(0), _p(m), _p(v), V, p.shape[1], _p(uniq_ids), _p(rows),
                                        _p(n_uniq), n, t, lr, b1, b2, eps, st), "rec_adam_rows_f32")


class _ColPlanRing:
    """``nbuf`` per-column de-duplication plans (csrc/colsort.hip): perm, col_uid [F,B], col_seg [F,B+1], col_nu [F] and
    -- ``dloc`` -- the inverse view the direct mode of the fused step reads.  ``plans[buf]`` holds a buffer's views by
    those names, ``a_plan[buf]`` the addresses of the first four as a ctypes tuple.  Consecutive buffers are contiguous,
    so ONE sort call builds the plans of up to ``group`` batches as group*F columns (one workgroup per column, 256 column
    pointers per launch; the sort kernels are latency-bound at < 1 wave per SIMD: two batches cost ~1.2x one).
    ``ws_per_buf``: a sort workspace per buffer (sorts that run on a second stream) instead of one."""

    def __init__(self, nbuf, group, B, F, V, field_offsets, max_key, dev, dloc, ws_per_buf):
        self.nbuf, self.GROUP, self.B, self.F, self.V, self.max_key = nbuf, group, B, F, V, max_key
        i32 = dict(dtype=torch.int32, device=dev)
        self.col_lo_rep = torch.tensor([int(o) for o in field_offsets] * group, dtype=torch.int64, device=dev)
        self.bad_ids = torch.zeros(1, **i32)
        arrays = dict(perm=torch.empty((nbuf, F, B), **i32),
                      col_uid=torch.empty((nbuf, F, B), dtype=torch.int64, device=dev),
                      col_seg=torch.empty((nbuf, F, B + 1), **i32), col_nu=torch.zeros((nbuf, F), **i32))
        if dloc:
            arrays["dloc"] = torch.empty((nbuf, F, B), **i32)
        self.plans = [{k: a[b] for k, a in arrays.items()} for b in range(nbuf)]
        self.a_plan = [(_p(pl["perm"]), _p(pl["col_uid"]), _p(pl["col_seg"]), _p(pl["col_nu"])) for pl in self.plans]
        self._entry = "rec_colsort_plan_dest_i64" if dloc else "rec_colsort_plan_i64"
        self.sort_ws = [torch.empty(lib.rec_colsort_workspace_bytes(B, F * group), dtype=torch.uint8, device=dev)
                        for _ in range(nbuf if ws_per_buf else 1)]

    def sort_group(self, cols_list, first_buf, st, arr=None):
        """Plans of len(cols_list) <= GROUP batches into the consecutive buffers first_buf, first_buf + 1, ... as one
        sort call over len*F columns on stream handle ``st`` (``arr``: their pointer array, where the caller keeps one)."""
        k, F = len(cols_list), self.F
        assert 1 <= k <= self.GROUP and first_buf + k <= self.nbuf
        if arr is None:
            arr = (C.c_void_p * (k * F))(*[c.data_ptr() for cols in cols_list for c in cols])
        pl = self.plans[first_buf]
        dloc = (_p(pl["dloc"]),) if "dloc" in pl else ()
        ws = self.sort_ws[first_buf % len(self.sort_ws)]
        check(getattr(lib, self._entry)(arr, k * F, self.B, self.V, _p(self.col_lo_rep), self.max_key,
                                        *self.a_plan[first_buf], *dloc, _p(self.bad_ids), _p(ws), st), self._entry)


class _BatchReader:
    """The validated id columns (``names`` in order) and label of a batch dict.  ``cols_key`` caches them per dict: the
    26 dtype / device / size / stride checks and address reads of a batch were half of the host time of a fused-step
    call (which the GPU waits for whenever a call starts from an empty queue), so they run once per batch dict, and
    again only when a tensor of the dict was replaced (identity of the tensor objects, compared in C: itemgetter +
    map(id)).  ``cuda``: the tensors must live on the GPU (the kernels take raw device pointers)."""

    def __init__(self, names, B, cuda=True):
        self.names, self.B, self.cuda = list(names), int(B), cuda
        n0 = self.names[0]
        self._get = operator.itemgetter(*self.names) if len(self.names) > 1 else (lambda d: (d[n0],))
        self._cache = {}

    @staticmethod
    def key(cols):
        return tuple(c.data_ptr() for c in cols)

    def cols(self, inputs):
        """The columns of ``inputs``, validated (not cached)."""
        cols = list(self._get(inputs))
        for name, c in zip(self.names, cols):
            if c.dtype != torch.int64 or c.numel() != self.B or not c.is_contiguous() or (self.cuda and not c.is_cuda):
                raise ValueError("feature %r must be a contiguous int64 %stensor with %d ids"
                                 % (name, "CUDA " if self.cuda else "", self.B))
        return cols

    def cols_key(self, inputs):
        """(columns, their addresses) of ``inputs``."""
        ent = self._cache.get(id(inputs))
        if ent is not None and ent[2] is inputs and tuple(map(id, self._get(inputs))) == ent[3]:
            return ent[0], ent[1]
        cols = self.cols(inputs)
        if len(self._cache) > 256:
            self._cache.clear()
        key = self.key(cols)
        self._cache[id(inputs)] = (cols, key, inputs, tuple(map(id, cols)))
        return cols, key

    def label(self, inputs, name):
        """The label ``inputs[name]``: a contiguous float32 tensor of B entries (the BCE kernels read it as an array)."""
        y = inputs[name]
        if y.dtype != torch.float32 or y.numel() != self.B or not y.is_contiguous() or (self.cuda and not y.is_cuda):
            raise ValueError("label must be a contiguous float32 %stensor with %d entries"
                             % ("CUDA " if self.cuda else "", self.B))
        return y


class _GraphPolicy:
    """When a cached train step (DeepFMTrainStep, the fused steps, ShardedDeepFMStep.many) captures a call into a
    hipGraph, keeps it and replays it.  A subclass calls ``super().__init__()``, sets ``use_graph`` (False: every call
    eager), overrides ``_graphable`` where some calls must stay eager, and hands each call to ``_run``."""

    MAX_GRAPHS = 64     # captured hipGraphs kept (least recently used beyond that are dropped with the inputs they hold)
    use_graph = True

    def __init__(self):
        self._graphs = collections.OrderedDict()            # gkey -> (graph, inputs kept alive), LRU order
        self._seen = collections.OrderedDict()              # gkeys enqueued eagerly once (addresses only: nothing is held)

    def _graphable(self):
        return True

    def _run(self, gkey, enqueue_all, *keep):
        """The graph policy of a call with input addresses ``gkey``.  First sighting: plain eager enqueue, no device
        synchronisation, nothing retained -- an input pipeline that hands over fresh tensors every batch never gets past
        this branch, one that cycles staging buffers is captured on the next round.  Second sighting: enqueued eagerly
        -- that IS this call's work -- and then captured, without running, for the calls to come (with an optimizer in
        the step a warm-up followed by a replay would apply the update twice).  After that: replayed.  Every call thus
        does its work exactly once.  The last MAX_GRAPHS graphs used are kept, each with ``keep`` (the inputs whose
        addresses it holds)."""
        if not (self.use_graph and self._graphable()):
            enqueue_all()
            return
        ent = self._graphs.get(gkey)
        if ent is not None:
            self._graphs.move_to_end(gkey)
            ent[0].replay()
        elif gkey not in self._seen:
            enqueue_all()
            self._seen[gkey] = True
            if len(self._seen) > 8 * self.MAX_GRAPHS:
                self._seen.popitem(last=False)
        else:
            enqueue_all()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with _capture(g):
                enqueue_all()
            self._graphs[gkey] = (g,) + keep
            del self._seen[gkey]
            while len(self._graphs) > self.MAX_GRAPHS:
                self._graphs.popitem(last=False)             # least recently used: graph and retained inputs go

    def release(self):
        """Drop the captured graphs (and the inputs they hold)."""
        self._graphs.clear()
        self._seen.clear()


class DeepFMTrainStep(_GraphPolicy):
    """fwd + bwd (+ optimizer) of DeepFMRankingLayer (2.FM/CustomLayers.py:279-308) under the reference's loss.

    optimizer: None (gradients only -- the 'fwd+bwd' of the headline metric), 'keras_adam' (the reference's semantics:
    dense sweep over the tables) or 'lazy_adam' (touched rows only; NOT the reference's semantics).
    """

    def __init__(self, layer, batch_size, optimizer=None, lr=1e-3, use_graph=True):
        super().__init__()
        self.layer = layer
        self.B = B = int(batch_size)
        self.F = F = len(layer.feature_names)
        self.V, self.E = layer.embed.embeddings.shape
        E = self.E
        dev = layer.embed.embeddings.device
        self.dev = dev
        self.optimizer = optimizer
        self.lr = lr
        self.use_graph = use_graph
        self.t = 0
        f32 = dict(dtype=torch.float32, device=dev)
        n = B * F
        u1, u2 = layer.mlp_dims
        D = F * E
        self.X = torch.empty((B, F), dtype=torch.int64, device=dev)
        self.z_fm = torch.empty(B, **f32)
        self.rows = torch.empty((B, F, E), **f32)
        self.S = torch.empty((B, E), **f32)
        self.h1 = torch.empty((B, u1), **f32)
        self.h2 = torch.empty((B, u2), **f32)
        self.dnn = torch.empty((B, 1), **f32)
        self.prob = torch.empty((B, 1), **f32)
        self.loss = torch.empty(1, **f32)
        self.dz = torch.empty(B, **f32)
        self.dh2 = torch.empty((B, u2), **f32)
        self.dh1 = torch.empty((B, u1), **f32)
        self.drows = torch.empty((B, D), **f32)
        self.vals = torch.empty((n, E), **f32)
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        # gradients
        self.g = {name: torch.empty(shape, **f32) for name, shape in _deepfm_dense(F, u1, u2, E)}
        self.uniq_ids = torch.empty(n, dtype=torch.int64, device=dev)
        self.seg_start = torch.empty(n + 1, dtype=torch.int32, device=dev)
        self.perm = torch.empty(n, dtype=torch.int32, device=dev)
        self.n_uniq = torch.zeros(1, dtype=torch.int64, device=dev)
        self.g_embed_rows = torch.empty((n, E), **f32)
        self.g_w_rows = torch.empty((n, 1), **f32)
        self.dedup_bytes = lib.rec_dedup_workspace_bytes(n)
        self.dedup_ws = torch.empty(self.dedup_bytes, dtype=torch.uint8, device=dev)
        # split-K partials for the weight-gradient GEMMs (reduction over the batch)
        self.sk0 = ops.split_k_for(B, D, u1)
        self.sk1 = ops.split_k_for(B, u1, u2)
        self.sk2 = ops.split_k_for(B, u2, 1)
        self.ws0 = torch.empty((self.sk0, D, u1), **f32) if self.sk0 > 1 else None
        self.ws1 = torch.empty((self.sk1, u1, u2), **f32) if self.sk1 > 1 else None
        self.ws2 = torch.empty((self.sk2, u2, 1), **f32) if self.sk2 > 1 else None
        if optimizer is not None:
            self.state = {}
            for name, p in layer.named_parameters():
                self.state[name] = (torch.zeros(p.shape, **f32), torch.zeros(p.shape, **f32))   # dense m, v
            self.side_e = torch.empty((n, 3, E), **f32)
            self.side_w = torch.empty((n, 3, 1), **f32)
        self.colsum_ws = torch.empty(lib.rec_colsum_workspace_bytes(B, max(u1, u2)) // 4 + 1, **f32)
        self.segsum_ws = torch.empty(lib.rec_segment_sum_workspace_bytes(n, E) // 4, **f32)
        self._reader = _BatchReader(layer.feature_names, B)
        self._static_prog = self._build_static()

    # -- program construction ---------------------------------------------------------------------
    def _build_static(self):
        """Everything after index assembly; independent of where the input tensors live."""
        L = self.layer
        B, F, E, V = self.B, self.F, self.E, self.V
        u1, u2 = L.mlp_dims
        D = F * E
        emb, w, bias = L.embed.embeddings, L.w.embeddings, L.bias
        K0, b0 = L.MLP_layer1.kernel_0, L.MLP_layer1.bias_0
        K1, b1 = L.MLP_layer1.kernel_1, L.MLP_layer1.bias_1
        K2, b2 = L.MLP_layer2.kernel_0, L.MLP_layer2.bias_0
        P = _Program()
        # ---- forward
        P.add("rec_emb_fm_fwd_f32", _p(emb), emb.stride(0), _p(w), w.stride(0), _p(bias), V, E, _p(self.X), B, F,
              _p(self.z_fm), None, _p(self.rows), _p(self.S), _p(self.oob))
        P.add("rec_gemm_f32", 0, 0, B, u1, D, _p(self.rows), D, _p(K0), u1, _p(self.h1), u1, ops.EPI_BIAS_RELU, _p(b0),
              None, 0, None, 0, 1, None, None)
        P.add("rec_gemm_f32", 0, 0, B, u2, u1, _p(self.h1), u1, _p(K1), u2, _p(self.h2), u2, ops.EPI_BIAS_RELU, _p(b1),
              None, 0, None, 0, 1, None, None)
        P.add("rec_gemm_f32", 0, 0, B, 1, u2, _p(self.h2), u2, _p(K2), 1, _p(self.dnn), 1, ops.EPI_BIAS, _p(b2),
              None, 0, None, 0, 1, None, None)
        P.add("rec_act_fwd_f32", ops.ACT_SIGMOID, _p(self.dnn), _p(self.z_fm), _p(self.prob), B)
        self._loss_call_index = len(P.calls)
        P.add("rec_bce_fwd_bwd_f32", None, _p(self.prob), B, _p(self.loss), None, _p(self.dz))   # y bound per batch
        # ---- backward: MLP_layer2 (linear)
        g = self.g
        P.add("rec_gemm_f32", 1, 0, u2, 1, B, _p(self.h2), u2, _p(self.dz), 1, _p(g["MLP_layer2.kernel_0"]), 1,
              ops.EPI_NONE, None, None, 0, None, 0, self.sk2, _p(self.ws2), None)
        P.add("rec_colsum_f32", _p(self.dz), B, 1, 1, _p(g["MLP_layer2.bias_0"]), _p(self.colsum_ws))
        P.add("rec_gemm_f32", 0, 1, B, u2, 1, _p(self.dz), 1, _p(K2), 1, _p(self.dh2), u2, ops.EPI_NONE, None, None, 0,
              None, 0, 1, None, None)
        # ---- MLP_layer1 layer 1 (relu)
        P.add("rec_act_bwd_f32", ops.ACT_RELU, _p(self.h2), _p(self.dh2), _p(self.dh2), B * u2)
        P.add("rec_gemm_f32", 1, 0, u1, u2, B, _p(self.h1), u1, _p(self.dh2), u2, _p(g["MLP_layer1.kernel_1"]), u2,
              ops.EPI_NONE, None, None, 0, None, 0, self.sk1, _p(self.ws1), None)
        P.add("rec_colsum_f32", _p(self.dh2), B, u2, u2, _p(g["MLP_layer1.bias_1"]), _p(self.colsum_ws))
        P.add("rec_gemm_f32", 0, 1, B, u1, u2, _p(self.dh2), u2, _p(K1), u2, _p(self.dh1), u1, ops.EPI_NONE, None, None,
              0, None, 0, 1, None, None)
        # ---- MLP_layer1 layer 0 (relu)
        P.add("rec_act_bwd_f32", ops.ACT_RELU, _p(self.h1), _p(self.dh1), _p(self.dh1), B * u1)
        P.add("rec_gemm_f32", 1, 0, D, u1, B, _p(self.rows), D, _p(self.dh1), u1, _p(g["MLP_layer1.kernel_0"]), u1,
              ops.EPI_NONE, None, None, 0, None, 0, self.sk0, _p(self.ws0), None)
        P.add("rec_colsum_f32", _p(self.dh1), B, u1, u1, _p(g["MLP_layer1.bias_0"]), _p(self.colsum_ws))
        P.add("rec_gemm_f32", 0, 1, B, D, u1, _p(self.dh1), u1, _p(K0), u1, _p(self.drows), D, ops.EPI_NONE, None, None,
              0, None, 0, 1, None, None)
        # ---- tables: IndexedSlices values, de-duplication, segment sums
        P.add("rec_emb_fm_bwd_vals_f32", _p(emb), emb.stride(0), V, E, _p(self.X), B, F, _p(self.dz), _p(self.S),
              _p(self.rows), _p(self.drows), _p(self.vals))
        P.add("rec_dedup_plan_i64", _p(self.X), B * F, V, _p(self.uniq_ids), _p(self.seg_start), _p(self.perm),
              _p(self.n_uniq), _p(self.dedup_ws), self.dedup_bytes)
        P.add("rec_segment_sum_f32", _p(self.vals), E, _p(self.perm), _p(self.seg_start), B * F, 1,
              _p(self.g_embed_rows), _p(self.segsum_ws))
        P.add("rec_segment_sum_f32", _p(self.dz), 1, _p(self.perm), _p(self.seg_start), B * F, F, _p(self.g_w_rows),
              _p(self.segsum_ws))
        P.add("rec_colsum_f32", _p(self.dz), B, 1, 1, _p(g["bias"]), _p(self.colsum_ws))
        return P

    # -- execution ----------------------------------------------------------------------------------
    def _enqueue(self, cols, label, stream, t):
        F = self.F
        arr = (C.c_void_p * F)(*[c.data_ptr() for c in cols])
        check(lib.rec_index_pack_i64(arr, F, self.B, _p(self.X), F, 0, stream), "rec_index_pack_i64")
        calls = self._static_prog.calls
        name, fn, args = calls[self._loss_call_index]
        calls[self._loss_call_index] = (name, fn, (_p(label),) + args[1:])
        self._static_prog.run(stream)
        if self.optimizer is not None:
            _deepfm_host_adam(self.layer, self.g, self.state, self.uniq_ids, self.g_embed_rows, self.g_w_rows,
                              self.n_uniq, self.side_e, self.side_w, self.optimizer, t, self.lr, stream)

    def _graphable(self):
        return self.optimizer is None           # the optimizer's bias correction takes t as a host scalar: eager

    def __call__(self, inputs, label_name="label"):
        """One train_loop iteration.  Returns the device scalar loss (no synchronisation)."""
        cols, y = self._reader.cols(inputs), self._reader.label(inputs, label_name)
        self.t += 1
        t = self.t
        self._run(self._reader.key(cols) + (y.data_ptr(),),
                  lambda: self._enqueue(cols, y, C.c_void_p(torch.cuda.current_stream().cuda_stream), t), cols, y)
        return self.loss

    gradients = _deepfm_gradients


class _K0T:
    """Transposed copy K0^T [32, F*16] of layer 1's kernel for the fused kernel (csrc/deepfm_fused3.hip reads its K0
    operand as 16-byte pieces of K0^T), refreshed only when needed: the kernel reads it only when K0 does not fit in LDS
    beside the rows (F > 26), and only a changed parameter needs a new transpose."""

    def __init__(self, layer, F):
        self.layer, self.F = layer, F
        self.buf = torch.empty((32, F * 16), dtype=torch.float32, device=layer.MLP_layer1.kernel_0.device)
        self._ver = None

    def refresh(self, st=None, force=False):
        """Re-transpose if the parameter changed by torch (its version counter) -- or, ``force``, after an in-stream
        update through the C ABI, which the version counter does not see."""
        if self.F <= 26:
            return
        K0 = self.layer.MLP_layer1.kernel_0
        ver = (K0._version, K0.data_ptr())
        if force or ver != self._ver:
            if st is None:
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            check(lib.rec_deepfm_k0t_f32(_p(K0), self.F, _p(self.buf), st), "rec_deepfm_k0t_f32")
            if not force:
                self._ver = ver


def _bits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def _deepfm_fused_limits(B, field_dims, field_offsets, layer=None, sort_words=False):
    """What the fused DeepFM kernels are instantiated for.  ``layer``: embedding_dims 16, mlp_dims [32, 8], F <= 28,
    B <= 16384 and one (dim, offset) per feature (NotImplementedError).  ``sort_words``: ascending field offsets
    (ValueError: the DataGenerator contract) and in-field keys that fit the 32-bit words of the per-column plan sort
    beside the example index (NotImplementedError); returns the largest key."""
    if layer is not None:
        F = len(layer.feature_names)
        if layer.embed.embeddings.shape[1] != 16 or list(layer.mlp_dims) != [32, 8]:
            raise NotImplementedError("the fused DeepFM step covers embedding_dims=16, mlp_dims=[32,8]")
        if F > 28 or B > 16384 or len(field_dims) != F or len(field_offsets) != F:
            raise NotImplementedError("the fused DeepFM step: F <= 28, B <= 16384, one (dim, offset) per feature")
    if not sort_words:
        return None
    if any(field_offsets[i] >= field_offsets[i + 1] for i in range(len(field_offsets) - 1)):
        raise ValueError("field offsets must be ascending (DataGenerator contract)")
    max_key = max(int(d) for d in field_dims) - 1
    if _bits(max_key + 1) + _bits(B) > 32 or ((max_key << _bits(B)) | (B - 1)) >= 0xFFFFFFFF:
        raise NotImplementedError("field too wide for the 32-bit sort words at this batch size")
    return max_key


def _assign_plan_buffers(keys, n_then, prefetched, half, nhalf):
    """Plan buffers of one many() call.  The ring has two halves of ``nhalf`` buffers; the plans announced by the
    previous call (``prefetched``: batch key -> buffer) live in half ``half``.  A batch of this call that was announced
    reads its buffer (its first occurrence in the call: a repeat is planned again), every other batch takes the next
    free buffer of the same half and is planned inline.  The ``n_then`` batches announced for the next call go to the
    other half, which the next call then reads.
    Returns (bufs, inline, then_bufs, next_half): a buffer per batch, the indices of the batches planned inline, the
    announced batches' buffers and the half of the next call."""
    used = set(prefetched[k] for k in keys if k in prefetched)
    free = [half * nhalf + j for j in range(nhalf) if half * nhalf + j not in used]
    bufs, inline = [], []
    for i, k in enumerate(keys):
        if k in prefetched and prefetched[k] not in bufs:
            bufs.append(prefetched[k])
        else:
            bufs.append(free.pop(0))
            inline.append(i)
    other = (1 - half) * nhalf
    return bufs, inline, [other + j for j in range(n_then)], (1 - half if n_then else half)


class _FusedStep(_GraphPolicy):
    """Call machinery of the fused train steps (DeepFMFusedStep, DSSMFusedStep): batch reading, the ring of NBUF
    de-duplication plan buffers with the prefetch of announced batches, ``many()`` under the graph policy, and the
    device-side Adam clock.  A subclass sets B, calls ``super().__init__(names)`` (the id columns of a batch) and
    supplies ``_enqueue`` (the launches of one call), and where it differs ``_graphable``, ``_before_call`` and
    ``_after_call``."""

    NBUF = 64           # plan buffers: two halves of 32, many() alternates between them (a hipGraph launch leaves the GPU
                        # idle for ~30 us, so a call may hold up to 32 steps: ~1 us per step at that length)

    def __init__(self, names):
        super().__init__()
        self._reader = _BatchReader(names, self.B)
        self._prefetched, self._half = {}, 0     # plans announced by the previous call: id-tensor addresses -> buffer

    def _init_device_adam(self, names):
        """Adam with the step counter and the bias-corrected step size on the device (advanced by the fused launch): the
        train step holds no per-step host scalar, so it is captured and replayed like the gradient-only step.  The table
        holds lr_t of steps 1..N exactly as the host-side entry points compute it; beyond it the corrections are 1.0f.
        The rec_adam_dense_multi_f32 arguments of the dense parameters ``names`` are built once: parameters, moments and
        gradients are updated in place (and a captured graph holds their addresses anyway)."""
        N = 32768
        f32 = dict(dtype=torch.float32, device=self.dev)
        self._lr_tab = torch.tensor([lib.rec_adam_lr_t_f32(self.lr, ADAM_B1, ADAM_B2, t) for t in range(1, N + 1)], **f32)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._lr_t_dev = torch.zeros(1, **f32)
        params, k = dict(self.layer.named_parameters()), len(names)
        ptrs = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])     # noqa: E731
        self._multi = (k, ptrs(params[nm] for nm in names), ptrs(self.state[nm][0] for nm in names),
                       ptrs(self.state[nm][1] for nm in names), ptrs(self.g[nm] for nm in names),
                       (C.c_int64 * k)(*[self.g[nm].numel() for nm in names]))

    def _adam_dense_dev(self, st):
        """Adam on the dense parameters in ONE launch, with the step size of the device clock."""
        check(lib.rec_adam_dense_multi_f32(*self._multi, _p(self._lr_t_dev), ADAM_B1, ADAM_B2, ADAM_EPS, st),
              "rec_adam_dense_multi_f32")

    def _cols(self, inputs):
        return self._reader.cols(inputs)

    _key = staticmethod(_BatchReader.key)

    def _before_call(self):
        """Runs at the start of every call, outside any capture."""

    def _after_call(self, n, bufs):
        """Bookkeeping after a call of ``n`` steps that read plan buffers ``bufs``."""

    def __call__(self, inputs, label_name="label", next_inputs=None):
        """One train_loop iteration on `inputs`.  ``next_inputs`` (optional) = the batch of the NEXT call: its
        de-duplication plan is built behind this call's step (input-pipeline style prefetch: the plan depends on ids
        only).  Without it, or when the previous call did not announce this batch, the plan is built inside this call,
        in front of the fused kernel."""
        return self.many([inputs], label_name, then=next_inputs)

    def many(self, batches, label_name="label", then=None):
        """len(batches) <= NBUF / 2 consecutive train_loop iterations; with ``use_graph`` as ONE hipGraph replay (a
        launch-bound inner loop: one graph launch costs ~20 us of idle GPU).  ``then``: the batch, or the list of
        batches, of the NEXT call -- their de-duplication plans are built behind this call's steps, so that no fused
        kernel of the next call waits for a plan.  A batch of this call that no earlier call announced is planned in
        line.  Returns the last step's loss; ``loss_steps[i]`` holds step i's.  Results left in the buffers are the last
        step's; gradients are to be consumed by an optimizer in the same call or after single-step calls."""
        nhalf = self.NBUF // 2
        then_list = [] if then is None else [then] if isinstance(then, dict) else list(then)
        if not 1 <= len(batches) <= nhalf or len(then_list) > nhalf:
            raise ValueError("many(): 1 to %d batches per call (and at most %d per announcement)" % (nhalf, nhalf))
        rd = self._reader
        seq, keys = [], []
        for b in batches:
            cols, key = rd.cols_key(b)
            seq.append((cols, rd.label(b, label_name)))
            keys.append(key)
        then_cols, then_keys = [], []
        for b in then_list:
            cols, key = rd.cols_key(b)
            then_cols.append(cols)
            then_keys.append(key)
        bufs, inline, then_bufs, next_half = _assign_plan_buffers(keys, len(then_cols), self._prefetched, self._half,
                                                                  nhalf)
        gkey = (tuple(keys), tuple(y.data_ptr() for _, y in seq), tuple(then_keys), tuple(bufs), tuple(inline))
        t_base = self.t
        self._before_call()
        self._run(gkey, lambda: self._enqueue(seq, bufs, inline, then_cols, then_bufs, t_base), seq, then_cols)
        self.t = t_base + len(seq)
        self._after_call(len(seq), bufs)
        self._prefetched = dict(zip(then_keys, then_bufs))
        self._half = next_half
        return self.loss


class DeepFMFusedStep(_FusedStep):
    """The same train_loop iteration as DeepFMTrainStep in two launches on the main stream: the fused forward+backward
    kernel (csrc/deepfm_fused3.hip), then ONE launch (csrc/deepfm_fused.hip) for the fixed-order reduction of its partials
    and the segment sums -- plus, behind the steps of a call, the per-column LDS sort (csrc/colsort.hip) of the
    de-duplication plans of the batches announced for the next call (they depend only on the ids).  ``many()`` runs
    several iterations as one captured hipGraph (call forms and plan ring: _FusedStep; graph policy: _GraphPolicy).

    Requirements (checked; otherwise use DeepFMTrainStep): embedding_dims 16, mlp_dims [32,8], fused table layout,
    F <= 28, B <= 16384, and the DataGenerator id-space contract -- ``field_offsets[f]``/``field_dims[f]`` =
    ``data_info.json``'s offsets and dims (2.FM/DataGenerator.py:126-134); an id outside its field's range sets
    ``self.bad_ids`` (checked by ``check_flags()``).
    """

    def __init__(self, layer, batch_size, field_dims, field_offsets, optimizer=None, lr=1e-3, use_graph=True,
                 direct=True, want_prob=False):
        self.layer = layer
        self.direct = bool(direct)
        self.B = B = int(batch_size)
        self.F = F = len(layer.feature_names)
        emb, w = layer.embed.embeddings, layer.w.embeddings
        self.V, self.E = emb.shape
        if emb.stride(0) != 32 or w.stride(0) != 32 or w.data_ptr() != emb.data_ptr() + 64:
            raise NotImplementedError("the fused step needs the fused [embed|w|pad] table layout (layer.cuda())")
        self.max_key = _deepfm_fused_limits(B, field_dims, field_offsets, layer, sort_words=True)
        dev = emb.device
        self.dev = dev
        if optimizer not in (None, "keras_adam", "lazy_adam", "keras_adam_lazy"):
            raise ValueError("optimizer must be None, 'keras_adam', 'lazy_adam' or 'keras_adam_lazy', not %r" % (optimizer,))
        if optimizer == "keras_adam_lazy" and not self.direct:
            # ('lazy_adam' has a plan-after form: rec_adam_rows_f32 over the finished row sums -- the same touched-rows
            # arithmetic; the lazily EVALUATED Keras Adam only exists inside the direct-mode post launch)
            raise ValueError("optimizer 'keras_adam_lazy' applies its update inside the direct-mode post launch: direct=True")
        self.optimizer, self.lr, self.use_graph, self.t = optimizer, lr, use_graph, 0
        f32 = dict(dtype=torch.float32, device=dev)
        n = B * F
        self.gz = torch.empty(B, **f32)
        self.vals = torch.empty((n, 16), **f32)
        # per-step results of a many() call (a caller that keeps metrics reads them after the call): loss_steps[i] and --
        # want_prob -- prob_steps[i] of the i-th batch; `loss` / `prob` are views of the LAST step's entries
        self.loss_steps = torch.zeros(self.NBUF // 2, **f32)
        self.prob_steps = torch.empty((self.NBUF // 2, B), **f32) if want_prob else None
        self.loss = self.loss_steps[:1]
        self.prob = self.prob_steps[0] if want_prob else None
        self._row = 0                                                # row of the step being enqueued
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        self.g = {name: torch.empty(shape, **f32) for name, shape in _deepfm_dense(F)}
        self.ws = torch.empty(lib.rec_deepfm_fused_workspace_bytes(B, F), dtype=torch.uint8, device=dev)
        # NBUF plan buffers: the de-duplication plan depends on the ids only, so the plans of the NEXT call's batches are
        # built behind the steps of this call.  Every batch of a call has a buffer of its own (two halves of NBUF / 2 used
        # alternately: one is read by this call's steps while the other is filled for the next call).  256 // F batches per
        # sort launch: a CU holds ONE sort workgroup (98 KB of LDS) -- 17 batches per launch, 442 workgroups, were measured
        # slower than 9
        self._ring = _ColPlanRing(self.NBUF, max(1, 256 // F), B, F, self.V, field_offsets, self.max_key, dev, dloc=True,
                                  ws_per_buf=False)
        self.plans, self.GROUP, self.bad_ids = self._ring.plans, self._ring.GROUP, self._ring.bad_ids
        super().__init__(layer.feature_names)
        self.uniq_ids = torch.empty(n, dtype=torch.int64, device=dev)
        self.g_embed_rows = torch.empty((n, 16), **f32)
        self.g_w_rows = torch.empty((n, 1), **f32)
        self.n_uniq = torch.zeros(1, dtype=torch.int64, device=dev)
        # (the plan sorts run on the caller's stream behind the steps of a call.  A second stream was tried at every
        # priority the device offers -- the range is (0, -1), the default 0 is the lowest, and a step enqueued on a
        # priority -1 stream ran 2.5x SLOWER from its graphs: a sort workgroup cannot share a CU with a fused-kernel
        # workgroup, so concurrency only moved the wait into one fused launch in eight)
        if optimizer is not None:
            self.state = {name: (torch.zeros(p.shape, **f32), torch.zeros(p.shape, **f32))
                          for name, p in layer.named_parameters()}
            self.side_e = torch.empty((n, 3, 16), **f32)
            self.side_w = torch.empty((n, 3, 1), **f32)
        if self._fused_lazy():
            # optimizer state packed beside the rows: [m 16 | v 16] of a row is ONE 128-byte line, m_w / v_w live in
            # floats 17 / 18 of the fused table row (its padding) -- a touched row costs two line requests instead of
            # five or six (table row, m_e, v_e, m_w, v_w).  state[...] stays a pair of (strided) views
            fused = getattr(layer, "_fused_storage", None)
            if fused is not None and fused.shape[1] == 32:
                # floats 17 / 18 of every fused table row are RESERVED for this step's m_w / v_w: the storage must still be
                # what embed.embeddings views, and only one step may own it (a second one would wipe the first one's state)
                if fused.data_ptr() != emb.data_ptr():
                    raise ValueError("layer._fused_storage no longer aliases embed.embeddings")
                owner = getattr(layer, "_fused_state_owner", None)
                if owner is not None and owner() is not None and owner() is not self:
                    raise ValueError("another DeepFMFusedStep already keeps its optimizer state in this layer's table "
                                     "padding (floats 17/18 of the fused rows): one lazy-optimizer step per layer")
                layer._fused_state_owner = weakref.ref(self)
                self._mv = torch.zeros((self.V, 32), **f32)
                fused[:, 17:19].zero_()
                self.state["embed.embeddings"] = (self._mv[:, :16], self._mv[:, 16:])
                self.state["w.embeddings"] = (fused[:, 17:18], fused[:, 18:19])
            self._last = (torch.zeros(self.V, dtype=torch.int32, device=dev)
                          if optimizer == "keras_adam_lazy" else None)    # the step every row holds
            self._init_device_adam(list(self.g))
        # K0^T for the fused kernel, refreshed whenever the parameter changed -- by torch or by this step's own optimizer
        # launches (which re-transpose in the same stream)
        self._k0t = _K0T(layer, F)
        # the two launches' argument lists, built once: every address in them is fixed for the life of the step.  The
        # per-call entries (None here) are the column pointers, label and prob row of the main launch, the loss row of
        # the post launch and the plan buffer of both
        lazy = self._fused_lazy()
        w_arr, g_arr = _deepfm_ptr_arrays(layer, self._k0t, self.g)
        clock = ((_p(self._step_dev), _p(self._lr_tab), self._lr_tab.numel(), _p(self._lr_t_dev)) if lazy
                 else (None, None, 0, None))
        self._a_main = [_p(emb), emb.stride(0), self.V, None, F, B, w_arr, None, _p(self.gz), _p(self.vals), None,
                        _p(self.oob), _p(self.ws), None, None, _p(self.g_embed_rows) if self.direct else None, *clock]
        self._a_plan_main = [(_p(pl["dloc"]), a[3]) if self.direct else (None, None)
                             for pl, a in zip(self.plans, self._ring.a_plan)]
        self._adam = None
        if lazy:
            (me, ve), (mw, vw) = self.state["embed.embeddings"], self.state["w.embeddings"]
            # (table, ld, V, m_e, v_e, ld_state, m_w, v_w, ld_wstate, last, step_dev, lr_table, n_table, b1, b2, eps)
            self._a_catchup = (_p(emb), emb.stride(0), self.V, _p(me), _p(ve), me.stride(0), _p(mw), _p(vw), mw.stride(0),
                               _p(self._last), *clock[:3], ADAM_B1, ADAM_B2, ADAM_EPS)
            ptr = lambda t: t.data_ptr() if t is not None else None     # noqa: E731
            self._adam = DeepFMLazyAdam(ptr(emb), emb.stride(0), self.V, ptr(me), ptr(ve), ptr(mw), ptr(vw), me.stride(0),
                                        mw.stride(0), ptr(self._lr_t_dev), ADAM_B1, ADAM_B2, ADAM_EPS, ptr(self._last),
                                        ptr(self._step_dev))
        self._a_post = [F, B, _p(self.gz), _p(self.vals), g_arr, None, _p(self.ws), None, None, None, None,
                        _p(self.uniq_ids), _p(self.g_embed_rows), _p(self.g_w_rows), _p(self.n_uniq), None,
                        int(self.direct), self._adam]

    def _sort(self, cols, buf, stream):
        self._ring.sort_group([cols], buf, C.c_void_p(stream.cuda_stream))

    def _ploss(self):
        return C.c_void_p(self.loss_steps.data_ptr() + 4 * self._row)

    def _pprob(self):
        return C.c_void_p(self.prob_steps.data_ptr() + 4 * self.B * self._row) if self.prob_steps is not None else None

    def _launch_main(self, cols, label, st, buf):
        """The fused kernel.  Direct mode: the plan in buffer ``buf`` is complete, so the value row of every run's first
        member goes straight to its slot of g_embed_rows (with gz and the id)."""
        if self._adam is not None and self._last is not None:
            # Keras Adam, lazily: the rows this batch reads replay the sweeps they skipped (steps last+1 .. now)
            pl = self._ring.a_plan[buf]
            check(lib.rec_adam_keras_catchup_f32(pl[1], pl[3], self.B, self.F, *self._a_catchup, st),
                  "rec_adam_keras_catchup_f32")
        self._k0t.refresh(st)
        # (lazy optimizers: the optimizer's device-side step counter advances inside this launch -- the kernel reads
        # neither word: the catch-up above saw the old step, the post launch and the dense update below see the new one)
        a = self._a_main
        a[3], a[7], a[10] = (C.c_void_p * self.F)(*[c.data_ptr() for c in cols]), _p(label), self._pprob()
        a[13:15] = self._a_plan_main[buf]
        check(lib.rec_deepfm_fused3_main_f32(*a, st), "rec_deepfm_fused3_main_f32")

    def _fused_lazy(self):
        """optimizer 'lazy_adam' / 'keras_adam_lazy' in direct mode: the touched-rows update of both tables rides in the
        post launch ('keras_adam_lazy': and the rows a batch is about to read first replay the dense sweeps they
        skipped -- Keras' Adam, bit for bit, without sweeping the table every step; flush() before reading parameters)"""
        return self.optimizer in ("lazy_adam", "keras_adam_lazy") and self.direct

    def _launch_post(self, buf, st, t=0):
        """reduction of the workgroup partials side by side with the segment sums (direct mode: with what is left of
        them -- runs of more than one lookup and the padded tail) in ONE launch"""
        a = self._a_post
        a[5] = self._ploss()
        a[7:11] = self._ring.a_plan[buf]
        check(lib.rec_deepfm_fused_post_f32(*a, st), "rec_deepfm_fused_post_f32")

    def _optimizer(self, t, st):
        if self._fused_lazy():
            # the tables were updated inside the post launch; the dense parameters follow in ONE launch, with the
            # step size the post launch used (device memory)
            self._adam_dense_dev(st)
            self._k0t.refresh(st, force=True)
            return
        _deepfm_host_adam(self.layer, self.g, self.state, self.uniq_ids, self.g_embed_rows, self.g_w_rows, self.n_uniq,
                          self.side_e, self.side_w, self.optimizer, t, self.lr, st,
                          after_dense=lambda: self._k0t.refresh(st, force=True))

    def _graphable(self):
        # (the non-lazy optimizers take the step as a host scalar: enqueued eagerly)
        return self.optimizer is None or self._fused_lazy()

    def _before_call(self):
        self._k0t.refresh()                                      # outside any capture: a replayed graph reads K0T

    def _enqueue(self, seq, bufs, inline, then_cols, then_bufs, t_base):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in inline:                                         # not announced: sorted in line
            self._ring.sort_group([seq[i][0]], bufs[i], st)
        for i, (cols, y) in enumerate(seq):
            self._row = i
            self._launch_main(cols, y, st, bufs[i])
            t = t_base + i + 1                                   # 1-based step (host scalar of the non-graphed optimizers)
            self._launch_post(bufs[i], st, t)
            if self.optimizer is not None:
                self._optimizer(t, st)
        # the plans of the batches announced for the NEXT call: GROUP batches (consecutive buffers) per sort launch, on the
        # main stream BEHIND this call's steps.  (They used to run on a second stream beside the steps -- but a sort
        # workgroup cannot share a CU with a fused-kernel workgroup (LDS), so "beside" meant that one fused launch in
        # eight waited for the sort: serial on one stream is 0.7 us per step faster at K = 200, the same at K = 20, and
        # the graph has no fork / join.)
        m_ = len(then_cols)
        if m_:
            nl = -(-m_ // self.GROUP)                            # as few launches as the column limit allows, evenly filled
            per = -(-m_ // nl)
            for j in range(0, m_, per):
                self._ring.sort_group(then_cols[j:j + per], then_bufs[j], st)

    def _after_call(self, n, bufs):
        self.loss = self.loss_steps[n - 1:n]                     # the last step's
        if self.prob_steps is not None:
            self.prob = self.prob_steps[n - 1]

    def flush(self):
        """optimizer 'keras_adam_lazy': bring EVERY row of the tables up to the current step (the dense sweeps the rows
        skipped) -- before the parameters are read from outside the step (evaluation, checkpoint)."""
        if not (self._fused_lazy() and self._last is not None):
            return
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.rec_adam_keras_flush_f32(*self._a_catchup, st), "rec_adam_keras_flush_f32")

    def release(self):
        """Give up the optimizer state kept in the layer's table padding (lazy optimizers) and the captured graphs, so
        that another step may be built on the same layer."""
        owner = getattr(self.layer, "_fused_state_owner", None)
        if owner is not None and owner() is self:
            self.layer._fused_state_owner = None
        super().release()

    def check_flags(self):
        if int(self.oob.item()) != 0:
            raise IndexError("embedding id out of range [0, feature_dims)")
        if int(self.bad_ids.item()) != 0:
            raise ValueError("an id lies outside its field's [offset, offset+dim) range (DataGenerator contract)")

    gradients = _deepfm_gradients


class DSSMFusedStep(_FusedStep):
    """train_loop iteration of DSSMTwoTowerRetrievalLayer (2.FM/CustomLayers.py:208-239 under 2.FM/ModelManager.py:
    171-177) in two launches on the main stream: the fused kernel (csrc/dssm_fused.hip: gather, both tower MLPs, score,
    Keras BCE and the whole backward) and the post launch (fixed-order reduction of its partials side by side with the
    segment sums of both towers' gradient rows).  The de-duplication plans (rec_dedup_plan_i64 of each tower's flat
    [B*F] ids) of the batches announced for the next call are built behind the steps of this call.  Call forms and plan
    ring: _FusedStep; graph policy: _GraphPolicy.

    Requirements (checked; otherwise keep GraphedTrainStep, raises NotImplementedError): plain (unsharded) tables with
    the same embedding_dims E in {8, 16, 32, 64} in both towers, mlp_dims [64, 32], final_dim 8, 1 <= F <= 8 features
    per tower.  optimizer: None (gradients only) or 'lazy_adam' (touched rows of both tables + Adam on the dense
    parameters, step size on the device, so it is captured with the step; NOT the reference's dense-sweep semantics).
    """

    DENSE = ("mlp.kernel_0", "mlp.bias_0", "mlp.kernel_1", "mlp.bias_1", "final.kernel_0", "final.bias_0")

    def __init__(self, layer, batch_size, optimizer=None, lr=1e-3, use_graph=True, want_outputs=False):
        from . import layers as CL
        if not isinstance(layer, CL.DSSMTwoTowerRetrievalLayer):
            raise NotImplementedError("DSSMFusedStep covers layers.DSSMTwoTowerRetrievalLayer only")
        if optimizer == "keras_adam":
            raise ValueError("optimizer 'keras_adam' is Keras' dense sweep: every row of both tables moves every step "
                             "(25.6 GB read and written per step at 100M x 64d); use 'lazy_adam' (touched rows) or "
                             "optimizer=None with an optimizer of your own")
        if optimizer not in (None, "lazy_adam"):
            raise ValueError("optimizer must be None or 'lazy_adam', not %r" % (optimizer,))
        self.layer = layer
        self.towers = (layer.u_tower, layer.i_tower)
        self.B = B = int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        Es = []
        for tw in self.towers:
            if not isinstance(tw.embed, CL.Embedding):
                raise NotImplementedError("the fused DSSM step needs plain (unsharded) Embedding tables")
            if list(tw.mlp.units) != [64, 32] or list(tw.final.units) != [8]:
                raise NotImplementedError("the fused DSSM step covers mlp_dims=[64,32] and final_dim=8 only")
            if tw.mlp.activation != "relu" or tw.final.activation is not None or not tw.mlp.use_bias \
                    or not tw.final.use_bias or tw.mlp.is_batch_norm or tw.final.is_batch_norm:
                raise NotImplementedError("the fused DSSM step covers the reference's towers (relu MLP with biases)")
            if not 1 <= len(tw.feature_names) <= 8:
                raise NotImplementedError("the fused DSSM step covers 1 to 8 features per tower")
            Es.append(tw.embed.embeddings.shape[1])
        if Es[0] != Es[1]:
            raise NotImplementedError("the fused DSSM step needs the same embedding_dims in both towers")
        self.E = E = Es[0]
        if E not in (8, 16, 32, 64):
            raise NotImplementedError("the fused DSSM step covers embedding_dims in {8, 16, 32, 64}")
        self.F = tuple(len(tw.feature_names) for tw in self.towers)
        self.V = tuple(tw.embed.embeddings.shape[0] for tw in self.towers)
        for tw, V in zip(self.towers, self.V):
            t = tw.embed.embeddings
            if not t.is_cuda or t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
                raise NotImplementedError("tables must be float32 CUDA arrays with 16-byte aligned rows")
            if V > (1 << 32):
                raise NotImplementedError("the de-duplication plan sorts 32-bit ids: at most 2^32 rows per table")
        self.dev = dev = layer.u_tower.embed.embeddings.device
        self.optimizer, self.lr, self.use_graph, self.t = optimizer, lr, use_graph, 0
        f32 = dict(dtype=torch.float32, device=dev)
        Fu, Fi = self.F
        nu, ni = B * Fu, B * Fi
        self.vals = (torch.empty((nu, E), **f32), torch.empty((ni, E), **f32))
        self.rows = (torch.empty((nu, E), **f32), torch.empty((ni, E), **f32))
        self.loss_steps = torch.zeros(self.NBUF // 2, **f32)
        self.loss = self.loss_steps[0]
        self.outputs = None
        if want_outputs:
            self.outputs = {"user_embedding": torch.zeros((B, 8), **f32), "item_embedding": torch.zeros((B, 8), **f32),
                            "score": torch.zeros(B, **f32)}
        self._row = 0
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        self.names = ["u_tower." + n for n in self.DENSE] + ["i_tower." + n for n in self.DENSE]
        params = dict(layer.named_parameters())
        self.g = {n: torch.empty(params[n].shape, **f32) for n in self.names}
        self._g_arr = (C.c_void_p * 12)(*[self.g[n].data_ptr() for n in self.names])
        self.ws_bytes = lib.rec_dssm_fused_workspace_bytes(B, E, Fu, Fi)
        if self.ws_bytes == 0:
            raise NotImplementedError("rec_dssm_fused_workspace_bytes: unsupported shape")
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        # NBUF plan buffers per tower: packed ids [B*F], uniq_ids, seg_start, perm, n_uniq (rec_dedup_plan_i64).  The plan
        # depends on the ids only, so the plans of the NEXT call's batches are built behind the steps of this call (two
        # halves of NBUF / 2 used alternately: one is read by this call's steps while the other is filled)
        NB = self.NBUF
        self.plans = []
        for n in (nu, ni):
            self.plans.append(dict(ids=torch.empty((NB, n), dtype=torch.int64, device=dev),
                                   uniq=torch.empty((NB, n), dtype=torch.int64, device=dev),
                                   seg=torch.empty((NB, n + 1), dtype=torch.int32, device=dev),
                                   perm=torch.empty((NB, n), dtype=torch.int32, device=dev),
                                   nu=torch.zeros((NB, 1), dtype=torch.int64, device=dev)))
        self.dedup_ws_bytes = lib.rec_dedup_workspace_bytes(max(nu, ni))
        self.dedup_ws = torch.empty(self.dedup_ws_bytes, dtype=torch.uint8, device=dev)
        self._last_buf = 0
        # a batch's columns: the user tower's features, then the item tower's
        super().__init__([n for tw in self.towers for n in tw.feature_names])
        if optimizer is not None:
            self.state = {name: (torch.zeros(p.shape, **f32), torch.zeros(p.shape, **f32))
                          for name, p in params.items()}
            self._init_device_adam(self.names)

    # ---- plans
    def _plan(self, cols, buf, st):
        """rec_index_pack_i64 + rec_dedup_plan_i64 of both towers' ids (``cols``: user columns, then item columns) into
        plan buffer ``buf``."""
        Fu = self.F[0]
        for t, tcols in enumerate((cols[:Fu], cols[Fu:])):
            F, pl = self.F[t], self.plans[t]
            n = self.B * F
            arr = (C.c_void_p * F)(*[c.data_ptr() for c in tcols])
            ids = pl["ids"][buf]
            check(lib.rec_index_pack_i64(arr, F, self.B, _p(ids), F, 0, st), "rec_index_pack_i64")
            check(lib.rec_dedup_plan_i64(_p(ids), n, self.V[t], _p(pl["uniq"][buf]), _p(pl["seg"][buf]),
                                         _p(pl["perm"][buf]), _p(pl["nu"][buf]), _p(self.dedup_ws), self.dedup_ws_bytes,
                                         st), "rec_dedup_plan_i64")

    # ---- the two launches
    def _launch_main(self, y, buf, st):
        params = dict(self.layer.named_parameters())
        w = (C.c_void_p * 12)(*[params[n].data_ptr() for n in self.names])
        (tu, ti) = (tw.embed.embeddings for tw in self.towers)
        o = self.outputs
        adv = (_p(self._step_dev), _p(self._lr_tab), self._lr_tab.numel(), _p(self._lr_t_dev)) \
            if self.optimizer is not None else (None, None, 0, None)
        check(lib.rec_dssm_fused_main_f32(
            _p(tu), tu.stride(0), self.V[0], _p(self.plans[0]["ids"][buf]), self.F[0],
            _p(ti), ti.stride(0), self.V[1], _p(self.plans[1]["ids"][buf]), self.F[1],
            self.E, 64, 32, 8, self.B, w, _p(y), _p(self.vals[0]), _p(self.vals[1]),
            _p(o["user_embedding"]) if o else None, _p(o["item_embedding"]) if o else None, _p(o["score"]) if o else None,
            _p(self.oob), _p(self.ws), self.ws_bytes, *adv, st), "rec_dssm_fused_main_f32")

    def _launch_post(self, buf, st):
        pu, pi = self.plans
        adam, lr_t = None, None
        (tu, ti) = (tw.embed.embeddings for tw in self.towers)
        if self.optimizer is not None:
            (mu, vu), (mi, vi) = self.state["u_tower.embed.embeddings"], self.state["i_tower.embed.embeddings"]
            adam = (C.c_void_p * 6)(*[x.data_ptr() for x in (tu, mu, vu, ti, mi, vi)])
            lr_t = _p(self._lr_t_dev)
        check(lib.rec_dssm_fused_post_f32(
            self.B, self.E, self.F[0], self.F[1], _p(self.ws), self.ws_bytes, self._g_arr,
            C.c_void_p(self.loss_steps.data_ptr() + 4 * self._row),
            _p(self.vals[0]), _p(pu["perm"][buf]), _p(pu["seg"][buf]), _p(pu["uniq"][buf]), _p(pu["nu"][buf]),
            _p(self.rows[0]),
            _p(self.vals[1]), _p(pi["perm"][buf]), _p(pi["seg"][buf]), _p(pi["uniq"][buf]), _p(pi["nu"][buf]),
            _p(self.rows[1]),
            adam, tu.stride(0), self.V[0], ti.stride(0), self.V[1], lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, st),
            "rec_dssm_fused_post_f32")
        if self.optimizer is not None:
            self._adam_dense_dev(st)

    def _enqueue(self, seq, bufs, inline, then_cols, then_bufs, t_base):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for i in inline:                                         # not announced: planned in line
            self._plan(seq[i][0], bufs[i], st)
        for i, (_, y) in enumerate(seq):
            self._row = i
            self._launch_main(y, bufs[i], st)
            self._launch_post(bufs[i], st)
        for cols, b in zip(then_cols, then_bufs):                # the next call's plans, behind this call's steps
            self._plan(cols, b, st)

    def _after_call(self, n, bufs):
        self._last_buf = bufs[n - 1]
        self.loss = self.loss_steps[n - 1]

    def check_flags(self):
        if int(self.oob.item()) != 0:
            raise IndexError("embedding id out of range [0, feature_dims)")

    def gradients(self):
        """The last step's gradients: dense tensors by parameter name; (uniq_ids, rows [n,E], n_uniq) per table."""
        out = dict(self.g)
        b = self._last_buf
        for t, name in enumerate(("u_tower.embed.embeddings", "i_tower.embed.embeddings")):
            pl = self.plans[t]
            out[name] = (pl["uniq"][b], self.rows[t], pl["nu"][b])
        return out


def exchange_capacity(field_dims, field_offsets, batch_size, rows_per_shard, n_shard):
    """Slots per owner of a fixed-capacity exchange: the most unique ids ONE batch can hold for one owner =
    max over owners of the sum over the fields that intersect the owner's block of min(B, overlap) (a field contributes
    at most one id per example).  Rounded up to a multiple of 8."""
    cap = 1
    for o in range(n_shard):
        lo, hi = o * rows_per_shard, (o + 1) * rows_per_shard
        c = 0
        for d, off in zip(field_dims, field_offsets):
            ov = min(hi, int(off) + int(d)) - max(lo, int(off))
            if ov > 0:
                c += min(int(batch_size), ov)
        cap = max(cap, c)
    return (cap + 7) // 8 * 8


class HipStepBackend:
    """Device-side pieces of ShardedDeepFMStep, all HIP kernels on preallocated buffers of constant size.  The CPU gloo
    test (tests/test_sharded.py) injects an oracle-backed stand-in with the same methods to exercise the exchange logic
    without a GPU; the product never does.

    The host issues ~10 C-ABI calls and 4 collectives per step and must stay ahead of the GPU, so nothing here looks up
    torch's current stream or builds pointer arrays more than once: `begin()` caches the stream handles of a step, the
    per-plan pointer arrays are built at construction, nothing is allocated per step and nothing is read back."""

    def __init__(self, step, field_dims, field_offsets):
        # the step owns its backend: a strong reference back would make the pair a reference cycle, which only the
        # cyclic GC frees -- whenever it happens to run, in a process forked later (multiprocessing) too, where
        # destroying the communicators, streams and graphs the step holds crashes the child
        self.step = weakref.proxy(step)
        B, F, P, cap = step.B, step.F, step.P, step.cap
        dev = step.dev
        n = B * F
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        i64 = dict(dtype=torch.int64, device=dev)
        m = P * cap                                        # rows of every exchange buffer
        self.o_ws_bytes = lib.rec_dedup_workspace_bytes(m)
        # NPL plan buffers.  The eager step alternates between the first two (the plan of batch k+1 is built beside step
        # k); many() gives every batch of its cycle a buffer of its own and sorts GROUP batches per launch (a sort
        # workgroup cannot share a CU with a fused-kernel workgroup -- LDS --, so a 32-us sort per step was 32 us on the
        # step's critical path; eight batches per launch cost ~36).  A sort workspace per buffer: the sorts run on a
        # second stream
        self.NPL = NPL = 16
        self._ring = _ColPlanRing(NPL, max(1, min(8, 256 // F)), B, F, step.V, field_offsets,
                                  _deepfm_fused_limits(B, field_dims, field_offsets, sort_words=True), dev, dloc=False,
                                  ws_per_buf=True)
        self.plans, self.GROUP, self.bad_ids = self._ring.plans, self._ring.GROUP, self._ring.bad_ids
        self.o_ws = [torch.empty(self.o_ws_bytes, dtype=torch.uint8, device=dev) for _ in range(NPL)]
        # the exchange fields of a plan; every pointer below is fixed for the life of the step: the ctypes argument
        # tuples are built once
        for buf, pl in enumerate(self.plans):
            pl.update(msg=torch.zeros((P, cap + 2), **i64), msg_theirs=torch.zeros((P, cap + 2), **i64),
                      uidx=torch.empty((F, B), **i64), slot_map=torch.zeros(n, **i32), n_uniq=torch.zeros(1, **i64),
                      # owner side: union of the P lists that arrive (depends on ids only: built with the plan)
                      o_uniq=torch.empty(m, **i64), o_seg=torch.empty(m + 1, **i32), o_perm=torch.empty(m, **i32),
                      o_nu=torch.zeros(1, **i64))
            pl["uidx_arr"] = (C.c_void_p * F)(*[pl["uidx"][f].data_ptr() for f in range(F)])
            pl["a_plan"] = self._ring.a_plan[buf]
            pl["a_map"] = (*pl["a_plan"], B, F, step.rows_per_shard, P, cap, _p(pl["msg"]), _p(pl["uidx"]),
                           _p(pl["slot_map"]), _p(pl["n_uniq"]), _p(step.oob))
            pl["a_owner"] = (P, cap, step.rows_per_shard, _p(pl["o_uniq"]), _p(pl["o_seg"]), _p(pl["o_perm"]),
                             _p(pl["o_nu"]), _p(self.o_ws[buf]), self.o_ws_bytes)
        self.gz = torch.empty(B, **f32)
        self.vals = torch.empty((n, 16), **f32)
        # rows travel as [embed 16 | w | pad 3] = 80 bytes, not as the 128-byte lines they are stored in (C2 -37 %)
        self.rows_out = torch.zeros((m, 20), **f32)        # owner-side gather result           -> C2
        self.rows_local = torch.zeros((m, 20), **f32)      # C2 ->  the batch's rows, [owner, slot]
        self.grows = torch.zeros((m, 20), **f32)           # [embed 16 | w | pad 3] per unique id -> C3
        self.rows_theirs = torch.zeros((m, 20), **f32)     # C3 ->
        self.o_rows = torch.empty((m, 20), **f32)
        self.o_sws = torch.empty(lib.rec_segment_sum_workspace_bytes(m, 20), dtype=torch.uint8, device=dev)
        self.ws = torch.empty(lib.rec_deepfm_fused_workspace_bytes(B, F), dtype=torch.uint8, device=dev)
        self.side = torch.cuda.Stream(device=dev)
        self.side_ctx = torch.cuda.stream(self.side)
        self.side_st = C.c_void_p(self.side.cuda_stream)
        self.main, self.st = None, None
        self._arr_cache = {}
        # the fused launches' pointer arrays: parameters and gradients are updated in place, their addresses stay
        self._k0t = _K0T(step.layer, F)
        self._w_arr, self._g_arr = _deepfm_ptr_arrays(step.layer, self._k0t, step.g)

    # -- streams: the plan of the next batch depends on ids only and is built beside the current step
    def begin(self):
        self.main = torch.cuda.current_stream()
        self.st = C.c_void_p(self.main.cuda_stream)

    def fork(self):
        self.side.wait_stream(self.main)

    def side_context(self):
        return self.side_ctx

    def join(self):
        self.main.wait_stream(self.side)

    def _col_arr(self, cols):
        key = tuple(c.data_ptr() for c in cols)
        arr = self._arr_cache.get(key)
        if arr is None:
            if len(self._arr_cache) > 64:
                self._arr_cache.clear()
            arr = self._arr_cache[key] = (C.c_void_p * len(cols))(*key)
        return arr

    def plan(self, cols, buf, on_side=False):
        """Per-column sort + unique (rec_colsort_plan_i64), then the fixed-capacity exchange map
        (rec_colsort_shard_map_fixed_i64): the id message, the slot of every lookup and of every unique id."""
        self.plan_group([cols], buf, on_side)
        return self.plans[buf]

    def plan_group(self, cols_list, first_buf, on_side=False):
        """The plans of len(cols_list) <= GROUP batches into the consecutive buffers first_buf, first_buf + 1, ...: ONE
        per-column sort over all their columns, then the exchange map of each."""
        st = self.side_st if on_side else self.st
        self._ring.sort_group(cols_list, first_buf, st, self._col_arr([c for cols in cols_list for c in cols]))
        for j in range(len(cols_list)):
            check(lib.rec_colsort_shard_map_fixed_i64(*self.plans[first_buf + j]["a_map"], st),
                  "rec_colsort_shard_map_fixed_i64")

    def owner_plan(self, pl, buf, on_side=False):
        """Union of the P ascending id lists that arrived (rank merge) as a segment plan over the payload rows."""
        st_ = self.step
        st = self.side_st if on_side else self.st
        check(lib.rec_dedup_plan_sorted_slabs_i64(_p(pl["msg_theirs"]), *pl["a_owner"], st),
              "rec_dedup_plan_sorted_slabs_i64")

    def gather(self, table, pl):
        """Owner-side gather of the 128-byte fused rows for the ids every rank asked for."""
        st_ = self.step
        check(lib.rec_emb_gather_lists_f32(_p(table), table.shape[0], 20, 32, _p(pl["msg_theirs"]), st_.P, st_.cap,
                                           _p(self.rows_out), _p(st_.oob), self.st), "rec_emb_gather_lists_f32")
        return self.rows_out

    def rows_step(self, pl, rows_local, y):
        """The fused forward+backward kernel on the exchanged rows: the local [P*cap,32] buffer is the "table" and
        the ids are the slots uidx.  Returns (vals [n,16], gz [B]); the dense gradients follow in local_grad (the
        reduction shares its launch with the segment sums)."""
        st_ = self.step
        self._k0t.refresh(self.st)
        check(lib.rec_deepfm_fused3_main_f32(_p(rows_local), 20, rows_local.shape[0], pl["uidx_arr"], st_.F, st_.B,
                                             self._w_arr, _p(y), _p(self.gz), _p(self.vals), None, _p(st_.oob),
                                             _p(self.ws), None, None, None, None, None, 0, None, self.st),
              "rec_deepfm_fused3_main_f32")
        return self.vals, self.gz

    def local_grad(self, pl, vals, gz):
        """Reduction of the workgroup partials (fills step.g / step.loss) and, in the same launch, this batch's
        gradient per unique id as rows [embed 16 | w | 0 0 0] in the id's slot of the [P*cap,20] send buffer."""
        st_ = self.step
        check(lib.rec_deepfm_fused_post_f32(st_.F, st_.B, _p(gz), _p(vals), self._g_arr, _p(st_.loss), _p(self.ws),
                                            *pl["a_plan"], None, _p(self.grows), None, None, _p(pl["slot_map"]), 0, None,
                                            self.st), "rec_deepfm_fused_post_f32")
        return self.grows

    def owner_reduce(self, pl, rows_theirs, scale):
        """Row sums in the order of the owner plan, times ``scale``.  Returns (uniq local ids, embed rows [.,16], w rows
        [.,1] -- views of one [P*cap,20] buffer that the next step overwrites --, n_uniq); entries past n_uniq are
        padding (a valid id, zero rows)."""
        m = rows_theirs.shape[0]
        st = self.st
        check(lib.rec_segment_sum_f32(_p(rows_theirs), 20, _p(pl["o_perm"]), _p(pl["o_seg"]), m, 1, _p(self.o_rows),
                                      _p(self.o_sws), st), "rec_segment_sum_f32")
        rows = self.o_rows
        if scale != 1.0:
            check(lib.rec_axpby_f32(scale, _p(rows), 0.0, _p(rows), rows.numel(), st), "rec_axpby_f32")
        return pl["o_uniq"], rows[:, :16], rows[:, 16:17], pl["o_nu"]

    def check_flags(self):
        if int(self.bad_ids.item()) != 0:
            raise ValueError("an id lies outside its field's [offset, offset+dim) range (DataGenerator contract)")


class ShardedDeepFMStep(_GraphPolicy):
    """DeepFM train_loop iteration with the fused [embed|w|pad] table ROW-SHARDED over the ranks of a process group
    (SURVEY.md section 8e): data-parallel batch (every rank its own B examples), block partition
    ``owner = id // ceil(V/P)``.  De-duplicate first, then exchange -- in FIXED-CAPACITY slabs: the field layout bounds
    the unique ids one batch can hold for one owner (exchange_capacity), so every exchange has constant split sizes:
    no count exchange, nothing read back by the host, every buffer allocated once.

        plan (ids only; built for batch k+1 on a second stream while batch k is differentiated)
            per-column sort + unique  ->  the batch's unique ids, ascending = already grouped by owner; every owner's
            ids go to its slab of the id message [P, 2+cap] (word 0 = how many)
            C1  all-to-all of the id messages on its OWN communicator (own RCCL stream: it does not queue behind
                the payload collectives), then the owner's union of the P lists that arrived (rank merge)
        --  owner-side gather of the fused rows' 80 used bytes into [P, cap, 20] (HIP, ids ascending per list)
        C2  all-to-all of the rows back -> a local [P*cap, 20] table, row = owner*cap + slot: no permutation anywhere
        --  the fused forward+backward kernel on those rows (it gathers by the slot of each lookup), then the
            per-unique-id segment sums of the row gradients (embed 16 + w 1) written to the ids' slots
        C3  all-to-all of the summed row gradients ([P*cap,20]) to the owners, who add them in the order of the union
        C4  one flat all-reduce (SUM) of the dense gradients and the loss, divided by P

    The loss is the mean over the GLOBAL batch of P*B examples (2.FM/ModelManager.py:171-177 on the concatenated
    batch): every rank's kernel scales by 1/B, so dense gradients are averaged over ranks and owner-side row sums
    are multiplied by 1/P.  Same kernels as the single-GPU path; at world_size 1 it reproduces DeepFMFusedStep and at
    world_size 2 (gloo) the global-batch result (tests/test_sharded.py).
    ``table_shard`` [rows_per_shard, 32] holds global rows [rank*rows_per_shard, ...).
    """

    def __init__(self, layer, batch_size, field_dims, field_offsets, group=None, backend=None, comm=None):
        from . import sharded
        super().__init__()
        self.comm = comm if comm is not None else sharded.DistComm(group, separate_count_channel=True)
        self.P, self.rank = self.comm.world, self.comm.rank
        self.layer = layer
        self.B = B = int(batch_size)
        self.F = F = len(layer.feature_names)
        emb, w = layer.embed.embeddings, layer.w.embeddings
        V = emb.shape[0]
        _deepfm_fused_limits(B, field_dims, field_offsets, layer)
        fused = getattr(layer, "_fused_storage", None)      # [V,32] rows = [embed | w | pad] (layers._FMTables)
        if fused is None:                                   # layer not on the GPU (CPU exchange-logic test)
            fused = torch.zeros((V, 32), dtype=torch.float32, device=emb.device)
            fused[:, :16].copy_(emb.data)
            fused[:, 16:17].copy_(w.data)
        self.V = V
        self.rows_per_shard = -(-V // self.P)
        self.cap = exchange_capacity(field_dims, field_offsets, B, self.rows_per_shard, self.P)
        lo = min(V, self.rank * self.rows_per_shard)
        hi = min(V, lo + self.rows_per_shard)
        self.row_range = (lo, hi)
        self.dev = dev = emb.device
        f32 = dict(dtype=torch.float32, device=dev)
        # this rank's block of the fused table (a real deployment would never hold the full table anywhere)
        self.table_shard = torch.zeros((self.rows_per_shard, 32), **f32)
        self.table_shard[: hi - lo].copy_(fused[lo:hi])
        self.n = B * F
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)
        # the dense gradients and the loss are views of ONE flat buffer: C4 is a single in-place all-reduce, no
        # concatenation before it and no copies after it (every view starts on a 16-byte boundary)
        views, total = {}, 0
        for name, shp in _deepfm_dense(F) + (("loss", (1,)),):
            views[name] = (total, shp)
            total += (math.prod(shp) + 3) // 4 * 4
        self.flat = torch.zeros(total, **f32)
        views = {name: self.flat[off:off + math.prod(shp)].view(shp) for name, (off, shp) in views.items()}
        self.loss = views.pop("loss")
        self.g = views
        self.be = (backend or HipStepBackend)(self, field_dims, field_offsets)
        self._reader = _BatchReader(layer.feature_names, B, cuda=isinstance(self.be, HipStepBackend))
        self._next = None               # (key, buffer, plan) announced by the previous call
        self.table_grad = None          # (local uniq ids, embed rows [.,16], w rows [.,1], n_uniq) after a step

    def _plan(self, cols, buf, on_side):
        """Plan + C1 + the owner's union of what arrived: everything that depends on the ids alone."""
        pl = self.be.plan(cols, buf, on_side=on_side)
        pl["msg_theirs"] = self.comm.exchange_ids(pl["msg"], pl["msg_theirs"])
        self.be.owner_plan(pl, buf, on_side=on_side)
        return pl

    def __call__(self, inputs, label_name="label", next_inputs=None):
        be, comm = self.be, self.comm
        be.begin()
        cols, key = self._reader.cols_key(inputs)
        y = self._reader.label(inputs, label_name)
        if self._next is not None and self._next[0] == key:
            _, buf, pl = self._next
            be.join()                                        # the plan was built on the second stream
        else:
            buf = 0
            pl = self._plan(cols, buf, False)
        self._next = None
        if next_inputs is not None:
            next_cols, next_key = self._reader.cols_key(next_inputs)
            be.fork()
            with be.side_context():                          # C1 of the next batch: own communicator, second stream
                nxt = self._plan(next_cols, 1 - buf, True)
            self._next = (next_key, 1 - buf, nxt)
        return self._body(pl, y)

    def _body(self, pl, y):
        """What of a step needs the batch's plan to be complete: owner gather, C2, fused kernel, local sums, C3, owner sums,
        C4."""
        be, comm = self.be, self.comm
        rows_out = be.gather(self.table_shard, pl)                             # owner-side gather of 128-B rows
        rows_local = comm.exchange(rows_out, be.rows_local)                    # C2: [P*cap, 32], row = owner*cap + slot
        vals, gz = be.rows_step(pl, rows_local, y)
        grows = be.local_grad(pl, vals, gz)
        rows_theirs = comm.exchange(grows, be.rows_theirs)                     # C3
        self.table_grad = be.owner_reduce(pl, rows_theirs, 1.0 / self.P)
        # C4: dense gradients and the loss, one flat all-reduce (mean over ranks = the global-batch gradient)
        if self.P > 1:
            comm.all_reduce_sum(self.flat)
            self.flat /= self.P
        return self.loss

    def many(self, batches, label_name="label"):
        """A cycle of steps over resident batches as ONE captured hipGraph (RCCL collectives included: every exchange
        has constant sizes and nothing is read back, so the sequence is a fixed program).  The plan of the first batch
        is built inside the graph on the main stream, the plans of the following ones on the second stream beside the
        step before.  Every rank must call it with the same number of batches.  Under the graph policy every call runs
        the cycle exactly once, eager or replayed, so ranks whose graph caches differ still issue the same collectives.
        ``release()`` the graphs before the process group is destroyed: they hold RCCL kernels.  Returns the loss of the
        last step."""
        rd = self._reader
        ck = [rd.cols_key(b) for b in batches]
        colss = [cols for cols, _ in ck]
        ys = [rd.label(b, label_name) for b in batches]
        grouped = isinstance(self.be, HipStepBackend) and len(batches) <= self.be.NPL

        def enqueue_all():
            self._next = None
            if not grouped:
                for i, b in enumerate(batches):
                    self(b, label_name, next_inputs=batches[i + 1] if i + 1 < len(batches) else None)
                return
            # every plan of the cycle on the second stream, GROUP batches per sort launch (ids only: nothing of the
            # steps is needed), each followed by its C1 and the owner's merge; step i waits for plan i alone
            be, comm = self.be, self.comm
            be.begin()
            be.fork()
            evs = []
            with be.side_context():
                for j0 in range(0, len(batches), be.GROUP):
                    be.plan_group(colss[j0:j0 + be.GROUP], j0, on_side=True)
                for i in range(len(batches)):
                    pl = be.plans[i]
                    pl["msg_theirs"] = comm.exchange_ids(pl["msg"], pl["msg_theirs"])
                    be.owner_plan(pl, i, on_side=True)
                    ev = torch.cuda.Event()
                    ev.record(be.side)
                    evs.append(ev)
            for i in range(len(batches)):
                be.main.wait_event(evs[i])
                self._body(be.plans[i], ys[i])
            be.join()
        key = tuple(k for _, k in ck) + tuple(y.data_ptr() for y in ys)          # every column and label address
        self._run(key, enqueue_all, colss, ys)
        return self.loss

    def check_flags(self):
        if int(self.oob.item()) != 0:
            raise IndexError("embedding id out of range [0, feature_dims), or more unique ids for one owner than the "
                             "exchange capacity")
        self.be.check_flags()


class GraphedTrainStep:
    """Any layer of layers.py under the reference's loss as ONE replayed hipGraph: forward, KerasBCE and the whole
    autograd backward (every kernel goes through the C ABI on torch's current stream, nothing synchronises, all
    intermediates come from the graph's private pool), for the families that have no hand-fused step (DSSM towers, DCN,
    DIN).  The eager path costs ~0.5-1 ms of Python and launch overhead per iteration whatever the batch; a replay
    costs one graph launch.

        step = GraphedTrainStep(layer, example_batch, label_name="label")
        loss = step(batch)            # copies the batch into the static input buffers, replays; .grad of every parameter
                                      # is a tensor of the graph (dense, or sparse COO rows for tables) valid until the
                                      # next replay

    ``label_name`` may be a sequence of names (a multi-task layer): the target is then [B, T], one column per name.
    ``output_fn(layer, inputs) -> tensor`` replaces ``layer(inputs)["output"]`` for a layer whose result has no such key.

    The debug-mode bounds check of the layers (one host read per call) is switched off on this layer's modules: a host
    read cannot be captured.  Out-of-range ids then read as zero rows, as the kernels guarantee (no fault).
    """

    def __init__(self, layer, example_batch, label_name="label", loss_fn=None, warmup=3, extra_loss_fn=None,
                 output_fn=None):
        from . import functional as Fn
        from . import layers as CL
        self.layer = layer
        self.label_name = label_name
        self.label_names = (label_name,) if isinstance(label_name, str) else tuple(label_name)
        self.output_fn = output_fn
        self.extra_loss_fn = extra_loss_fn                   # (inputs dict) -> scalar added to the loss (DIN's L2 term)
        self.out = None                                      # the layer's output of the last replay (graph pool tensor)
        self.static = {k: v.clone() for k, v in example_batch.items() if isinstance(v, torch.Tensor)}
        self.loss_fn = loss_fn or (lambda out, y: Fn.KerasBCE.apply(out, y))
        for m in layer.modules():
            if isinstance(m, CL.Layer):
                m.check_ids = False                          # a host read of the bounds flag cannot be captured
        self.params = [p for p in layer.parameters() if p.requires_grad]
        # the warm-up passes run the layer in its training mode, and a module may update a buffer in place on every
        # forward (BatchNormalization folds the batch statistics into its moving averages): building the step must leave
        # the layer as it found it, so the buffers are saved here and written back -- in place, the capture records
        # their addresses -- before the capture.  Capturing executes nothing: the first replay is the first fold.
        # (This takes the layer to be BUILT: a module that registers a buffer on its first forward would have it created
        # and folded by the warm-up with nothing to restore it from -- checked below.)
        buffers = list(layer.buffers())
        saved = [b.clone() for b in buffers]
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._fwd_bwd()
        cur.wait_stream(side)
        if [id(b) for b in layer.buffers()] != [id(b) for b in buffers]:
            raise RuntimeError("GraphedTrainStep: the layer registered or replaced a buffer during the warm-up passes; "
                               "build every module (input_dim=...) or run one forward before the step is built")
        with torch.no_grad():
            for b, s in zip(buffers, saved):
                b.copy_(s)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        for p in self.params:
            p.grad = None
        with _capture(self.graph):
            self.loss = self._fwd_bwd()
        self.grads = [p.grad for p in self.params]           # tensors of the graph's pool: refreshed by every replay

    def _target(self, out):
        if not isinstance(self.label_name, str):             # one column per task
            return torch.stack([self.static[n].to(torch.float32).reshape(-1) for n in self.label_names], dim=1)
        y = self.static[self.label_name].to(torch.float32)
        if out.dim() == 2 and out.shape[1] > 1 and y.reshape(-1).numel() == out.shape[0]:
            y = y.reshape(-1, 1).expand(-1, out.shape[1])
        return y.contiguous()

    def _fwd_bwd(self):
        for p in self.params:
            p.grad = None
        ins = {k: v for k, v in self.static.items() if k not in self.label_names}
        out = self.output_fn(self.layer, ins) if self.output_fn is not None else self.layer(ins)["output"]
        loss = self.loss_fn(out, self._target(out))
        if self.extra_loss_fn is not None:
            loss = loss + self.extra_loss_fn(ins)
        loss.backward()
        self.out = out.detach()
        return loss.detach()

    def __call__(self, batch):
        # one multi-tensor copy per dtype instead of one tiny copy per feature column (26 + label for DeepFM)
        groups = {}
        for k, v in self.static.items():
            src = batch[k]
            if src.dtype == v.dtype and src.device == v.device and src.shape == v.shape:
                groups.setdefault(v.dtype, ([], []))
                groups[v.dtype][0].append(v)
                groups[v.dtype][1].append(src)
            else:
                v.copy_(src, non_blocking=True)
        for dsts, srcs in groups.values():
            torch._foreach_copy_(dsts, srcs)
        self.graph.replay()
        for p, g in zip(self.params, self.grads):
            p.grad = g
        return self.loss
