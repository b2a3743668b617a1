#!/usr/bin/env python3
"""Time the FiBiNet interaction kernels alone (csrc/fibinet.hip, through ops.fibinet_fwd / ops.fibinet_bwd) at configs FB
and FB26 (E = 16, 3 continuous columns, 'interaction'; F = 10, B = 16384 / F = 26, B = 8192), against the HBM bound of
the bytes each must move (8 TB/s), next to the same interaction written in torch on the GPU the way the reference
writes it (per-pair tensordots on the raw and the SENet-scaled embeddings, concats; autograd backward).
Prints one JSON line per config.  Usage: python scripts/exp/fibinet_time.py [FB FB26]"""
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from explicit_tf2_recommendation_amd import ops  # noqa: E402

HBM = 8.0e12


def timed(fn, warmup=5, iters=30):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def torch_fibinet(x, xc, S0, S1, Ws):
    F = x.shape[1]
    A = torch.relu(torch.relu(x.mean(-1) @ S0) @ S1)
    sen = x * A.unsqueeze(2)

    def bil(v):
        fl = torch.split(v, 1, dim=1)
        return torch.cat([torch.tensordot(fl[i], w, dims=([2], [0])) * fl[j]
                          for (i, j), w in zip(itertools.combinations(range(F), 2), Ws)], dim=1)
    return torch.cat([torch.cat([bil(x), bil(sen)], dim=1).reshape(x.shape[0], -1), xc], dim=1)


def run(name):
    F, B = (10, 16384) if name == "FB" else (26, 8192)
    E, C, mid = 16, 3, max(1, F // 3)
    P = F * (F - 1) // 2
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((B, F, E), device="cuda", generator=g)
    xc = torch.rand((B, C), device="cuda", generator=g)
    S0 = torch.rand((F, mid), device="cuda", generator=g) / F
    S1 = torch.rand((mid, F), device="cuda", generator=g) / mid
    W = torch.randn((P, E, E), device="cuda", generator=g) / 4
    D = 2 * P * E + C
    gout = torch.rand((B, D), device="cuda", generator=g)
    out, A, H1 = ops.fibinet_fwd(x, xc, S0, S1, W, 2)
    fwd_bytes = 4.0 * (B * F * E + B * C + B * D + B * (F + mid))
    bwd_bytes = 4.0 * (B * 2 * P * E + B * F * E + B * F * E + B * (F + mid))
    t_fwd = timed(lambda: ops.fibinet_fwd(x, xc, S0, S1, W, 2))
    t_bwd = timed(lambda: ops.fibinet_bwd(x, gout, A, H1, S0, S1, W, 2))
    xr, s0r, s1r = x.clone().requires_grad_(), S0.clone().requires_grad_(), S1.clone().requires_grad_()
    wr = [w.clone().requires_grad_() for w in W]
    t_tf = timed(lambda: torch_fibinet(xr, xc, s0r, s1r, wr), 2, 10)

    def torch_step():
        o = torch_fibinet(xr, xc, s0r, s1r, wr)
        torch.autograd.grad(o, [xr, s0r, s1r] + wr, gout)
    t_tstep = timed(torch_step, 2, 10)
    o_t = torch_fibinet(x, xc, S0, S1, list(W))
    err = float((out - o_t).abs().max() / o_t.abs().max())
    return {"config": name, "B": B, "F": F, "E": E, "P": P, "dnn_in_mb": B * D * 4 / 1e6,
            "hip_fwd_us": t_fwd * 1e6, "hip_bwd_us": t_bwd * 1e6, "hip_step_us": (t_fwd + t_bwd) * 1e6,
            "fwd_bound_us": fwd_bytes / HBM * 1e6, "bwd_bound_us": bwd_bytes / HBM * 1e6,
            "hip_fwd_frac_bound": fwd_bytes / HBM / t_fwd, "hip_bwd_frac_bound": bwd_bytes / HBM / t_bwd,
            "torch_fwd_us": t_tf * 1e6, "torch_step_us": t_tstep * 1e6, "max_rel_diff_vs_torch": err}


if __name__ == "__main__":
    for n in sys.argv[1:] or ["FB", "FB26"]:
        print(json.dumps(run(n)), flush=True)
