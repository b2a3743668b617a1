"""CPU checks of the fused DSSM two-tower step: the three C-ABI entry points are exported and refuse invalid (-1) or
unsupported (-2) arguments on the host, before anything is enqueued; engine.DSSMFusedStep refuses the layers it does not
cover with NotImplementedError (callers then keep GraphedTrainStep) and Keras' dense-sweep Adam with ValueError."""
import ctypes

import pytest


def _ptrs(k):
    """k distinct non-null, 16-byte aligned host addresses: never dereferenced by a call that is refused."""
    buf = (ctypes.c_float * (4 * k + 4))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return buf, [ctypes.c_void_p(base + 16 * j) for j in range(k)]


def test_symbols_exported():
    from explicit_tf2_recommendation_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("rec_dssm_fused_workspace_bytes", "rec_dssm_fused_main_f32", "rec_dssm_fused_post_f32"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES


def test_workspace_bytes():
    from explicit_tf2_recommendation_amd._lib import lib
    assert lib.rec_dssm_fused_workspace_bytes(8192, 64, 2, 3) > 0
    assert lib.rec_dssm_fused_workspace_bytes(1, 8, 1, 1) > 0
    assert lib.rec_dssm_fused_workspace_bytes(8192, 12, 2, 3) == 0      # E not in {8,16,32,64}
    assert lib.rec_dssm_fused_workspace_bytes(8192, 64, 9, 3) == 0      # F > 8
    assert lib.rec_dssm_fused_workspace_bytes(0, 64, 2, 3) == 0


def _main(lib, P, W, **kw):
    a = dict(u_table=P[0], u_ld=64, u_V=100, u_ids=P[1], F_u=2, i_table=P[2], i_ld=64, i_V=100, i_ids=P[3], F_i=3, E=64,
             h1=64, h2=32, d_out=8, B=16, weights=W, label=P[4], u_vals=P[5], i_vals=P[6], user_emb=None,
             item_emb=None, score=None, oob=P[7], ws=P[8], ws_bytes=1 << 30, step_dev=None, lr_table=None, n_table=0,
             lr_t_dev=None, stream=None)
    a.update(kw)
    return lib.rec_dssm_fused_main_f32(*a.values())


def _post(lib, P, G, **kw):
    a = dict(B=16, E=64, F_u=2, F_i=3, ws=P[0], ws_bytes=1 << 30, grads=G, loss=P[1], u_vals=P[2], u_perm=P[3],
             u_seg=P[4], u_uniq=P[5], u_nu=P[6], u_rows=P[7], i_vals=P[8], i_perm=P[9], i_seg=P[10], i_uniq=P[11],
             i_nu=P[12], i_rows=P[13], adam=None, u_ld=64, u_V=100, i_ld=64, i_V=100, lr_t=None, b1=0.9, b2=0.999,
             eps=1e-7, stream=None)
    a.update(kw)
    return lib.rec_dssm_fused_post_f32(*a.values())


def test_invalid_and_unsupported_arguments_need_no_gpu():
    from explicit_tf2_recommendation_amd._lib import lib
    keep, P = _ptrs(16)
    W = (ctypes.c_void_p * 12)(*[p.value for p in P[:12]])
    # main: invalid (-1)
    assert _main(lib, P, W, u_table=None) == -1
    assert _main(lib, P, W, label=None) == -1
    assert _main(lib, P, W, B=0) == -1
    assert _main(lib, P, W, u_ld=32) == -1                              # ld < E
    assert _main(lib, P, W, i_ld=66) == -1                              # ld not a multiple of 4
    assert _main(lib, P, W, weights=(ctypes.c_void_p * 12)(*([None] + [p.value for p in P[1:12]]))) == -1
    assert _main(lib, P, W, step_dev=P[9]) == -1                        # step counter without its table
    # main: unsupported (-2)
    assert _main(lib, P, W, E=12, u_ld=12, i_ld=12) == -2
    assert _main(lib, P, W, F_u=9) == -2
    assert _main(lib, P, W, h1=32) == -2
    assert _main(lib, P, W, h2=16) == -2
    assert _main(lib, P, W, d_out=16) == -2
    # post
    assert _post(lib, P, W, u_perm=None) == -1
    assert _post(lib, P, W, B=0) == -1
    assert _post(lib, P, W, adam=(ctypes.c_void_p * 6)(*[p.value for p in P[:6]])) == -1      # Adam without lr_t
    assert _post(lib, P, W, E=24) == -2
    assert _post(lib, P, W, F_i=0) == -2


def _layer(**kw):
    from explicit_tf2_recommendation_amd import layers
    a = dict(u_feature_names=["u1", "u2"], i_feature_names=["i1", "i2", "i3"], u_feature_dims=50, i_feature_dims=60)
    a.update(kw)
    return layers.DSSMTwoTowerRetrievalLayer(**a)


@pytest.mark.parametrize("kw,reason", [
    (dict(u_mlp_dims=[32, 32]), "mlp_dims"),
    (dict(i_mlp_dims=[64, 16]), "mlp_dims"),
    (dict(final_dim=4), "final_dim"),
    (dict(u_embedding_dims=16, i_embedding_dims=8), "same embedding_dims"),
    (dict(u_embedding_dims=12, i_embedding_dims=12), "embedding_dims in"),
    (dict(u_feature_names=["u%d" % j for j in range(9)]), "1 to 8 features"),
])
def test_unsupported_layers_raise_not_implemented(kw, reason):
    from explicit_tf2_recommendation_amd import engine
    with pytest.raises(NotImplementedError, match=reason):
        engine.DSSMFusedStep(_layer(**kw), 64)


def test_sharded_and_foreign_layers_raise_not_implemented():
    import torch
    from explicit_tf2_recommendation_amd import engine, layers
    layer = _layer()
    layer.i_tower.embed = torch.nn.Module()          # stands in for a sharded table (not a plain layers.Embedding)
    with pytest.raises(NotImplementedError, match="unsharded"):
        engine.DSSMFusedStep(layer, 64)
    with pytest.raises(NotImplementedError, match="DSSMTwoTowerRetrievalLayer"):
        engine.DSSMFusedStep(layers.DeepFMRankingLayer(feature_names=["a", "b"], feature_dims=10), 64)


def test_keras_dense_sweep_adam_is_refused():
    from explicit_tf2_recommendation_amd import engine
    with pytest.raises(ValueError, match="dense sweep"):
        engine.DSSMFusedStep(_layer(), 64, optimizer="keras_adam")
    with pytest.raises(ValueError):
        engine.DSSMFusedStep(_layer(), 64, optimizer="sgd")
