#!/usr/bin/env python3
"""One SHA-256 per tensor returned by the operators whose launch path or slot reduction the shared launch support
(csrc/common.h, csrc/slot_sum.hip) touches, at fixed seeds: the shapes of bench_configs X, FB (all three bilinear
types), AI, AF, a CrossNet vector stack, DIN's config E, a top-k scan and a panel-path GEMM, plus one small odd shape
each.  Run it on two builds and compare the JSON files: every digest must be equal (the sums are fixed-order, so equal
means bit-identical).  Usage: launch_support_digest.py OUT.json"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from explicit_tf2_recommendation_amd import ops  # noqa: E402

GEN = torch.Generator().manual_seed(20240517)
OUT = {}


def rnd(*shape, scale=1.0):
    return (torch.randn(shape, generator=GEN) * scale).cuda()


def ids(hi, *shape):
    return torch.randint(0, hi, shape, generator=GEN).cuda()


def put(name, tensors):
    for i, t in enumerate(tensors):
        if isinstance(t, (list, tuple)):
            put("%s.%d" % (name, i), t)
        elif t is not None:
            OUT["%s.%d" % (name, i)] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def cin(tag, B, F, E, sizes):
    x0 = rnd(B, F, E, scale=0.3)
    hs = [F] + sizes
    Ws = [rnd(1, F * hs[k], hs[k + 1], scale=0.1) for k in range(len(sizes))]
    part, states = ops.cin_fwd(x0, Ws)
    put(tag + ".cin_fwd", (part, states))
    put(tag + ".cin_bwd", ops.cin_bwd(x0, states, rnd(B, sum(sizes)), Ws))


def fibinet(tag, B, F, E, C, mid, kind):
    x, xc = rnd(B, F, E, scale=0.5), rnd(B, C)
    S0, S1 = rnd(F, mid, scale=0.5).abs(), rnd(mid, F, scale=0.5).abs()      # keep both ReLUs open
    W = rnd(ops.fibinet_num_weights(F, kind), E, E, scale=0.2)
    code = ops.FIBINET_TYPES[kind]
    dnn, A, H1 = ops.fibinet_fwd(x, xc, S0, S1, W, code)
    put("%s.%s.fibinet_fwd" % (tag, kind), (dnn, A, H1))
    put("%s.%s.fibinet_bwd" % (tag, kind), ops.fibinet_bwd(x, rnd(*dnn.shape), A, H1, S0, S1, W, code))


def autoint(tag, B, Fc, C, E, H, res):
    x, xc, ce = rnd(B, Fc, E, scale=0.5), rnd(B, C), rnd(C, E, scale=0.5)
    Wq, Wk, Wv, Wr = (rnd(E, E, scale=0.3) for _ in range(4))
    kw = dict(x_cont=xc, cemb=ce) if C else {}
    y, stats, o = ops.autoint_fwd(x, Wq, Wk, Wv, Wr, H, res, True, want_o=True, **kw)
    put(tag + ".autoint_fwd", (y, stats, o))
    put(tag + ".autoint_bwd", ops.autoint_bwd(x, Wq, Wk, Wv, Wr, y, rnd(B, Fc + C, E), stats, H, res, True, **kw))


def afm(tag, B, F, E, A, V):
    table, X = rnd(V, E, scale=0.3), ids(V, B, F)
    Wa, ba, hv, bh = rnd(E, A, scale=0.5), rnd(A, scale=0.1), rnd(A, 1, scale=0.5), rnd(1, scale=0.1)
    o, stats, _ = ops.emb_afm_fwd(table, X, Wa, ba, hv, bh)
    put(tag + ".emb_afm_fwd", (o, stats))
    put(tag + ".emb_afm_bwd", ops.emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, rnd(B, E)))


def crossnet(tag, B, D, L):
    x0, w, b = rnd(B, D, scale=0.5), rnd(L, D, scale=0.05), rnd(L, D, scale=0.05)
    y, xs = ops.crossnet_vec_fwd(x0, w, b)
    put(tag + ".crossnet_vec_fwd", (y, xs))
    put(tag + ".crossnet_vec_bwd", ops.crossnet_vec_bwd(x0, w, xs, rnd(B, D)))


def din(tag, B, T, C, E, H, V):
    D = C * E
    embed = rnd(V, E, scale=0.05)
    series = ids(V - 1, B, T, C) + 1
    lens = torch.randint(1, T + 1, (B,), generator=GEN).cuda()
    series[torch.arange(T, device="cuda")[None, :] >= lens[:, None]] = 0
    Wcat, Wkd, bext = ops.din_prepare(rnd(3 * D + D * D, H, scale=0.05), rnd(H, scale=0.05), D, H)
    Mext = ops.gemm(rnd(B, D, scale=0.1), Wcat, epi=ops.EPI_BIAS, bias=bext)
    alpha, mean, var = rnd(H, scale=0.1), rnd(H, scale=0.1), rnd(H, scale=0.1).abs() + 0.5
    args = (embed, series, Mext, Wkd, ops.DACT_DICE, alpha, mean, var, rnd(H, scale=0.1), rnd(1, scale=0.1), 0, 0)
    scores, pooled = ops.din_attn_fwd(*args)
    put(tag + ".din_attn_fwd", (scores, pooled))
    put(tag + ".din_attn_bwd", ops.din_attn_bwd(*args, scores, rnd(B, D)))


def topk(tag, nq, n, d, k):
    put(tag + ".topk_l2", ops.topk_l2(rnd(nq, d), rnd(n, d), k))


def gemm_panel(tag, M, N, K):
    put(tag + ".gemm", (ops.gemm(rnd(M, K, scale=0.1), rnd(K, N, scale=0.1)),))       # M >= 8192, 64 < N: the row panels


def main():
    cin("X", 16384, 10, 16, [16, 32, 64])
    for kind in ("all", "each", "interaction"):
        fibinet("FB", 16384, 10, 16, 3, 3, kind)
    autoint("AI", 16384, 10, 3, 8, 2, 2)
    afm("AF", 16384, 10, 16, 3, 100_000)
    crossnet("cross", 8192, 339, 3)
    din("E", 4096, 100, 3, 32, 36, 100_000)
    topk("topk", 1024, 1_000_000, 8, 20)
    gemm_panel("panel", 8192, 835, 835)
    # one small odd shape each
    cin("odd", 37, 5, 7, [3, 9])
    fibinet("odd", 19, 5, 9, 0, 2, "each")
    autoint("odd", 33, 4, 1, 6, 3, 1)
    autoint("odd0", 33, 5, 0, 6, 2, 0)
    afm("odd", 21, 3, 5, 2, 97)
    crossnet("odd", 77, 65, 2)
    din("odd", 5, 7, 2, 8, 36, 50)
    topk("odd", 3, 1000, 5, 7)
    gemm_panel("odd", 8200, 70, 33)
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        json.dump(OUT, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(OUT), sys.argv[1]))


if __name__ == "__main__":
    main()
