#!/usr/bin/env python3
"""Time the AutoInt attention (csrc/autoint.hip) at configs AI (10 cat + 3 cont fields, E = 8, H = 2, B = 16384) and
AI26 (26 cat + 3 cont, E = 16, H = 2, B = 8192), two layers as AutoIntLayer runs them (the continuous fields assembled
in layer 1): the forward, and the forward + backward of both layers.  Next to it, in the same process and alternating
with it region by region, the torch formulation of the same ops on the GPU (tests/autoint_ref.py's transcription on
CUDA tensors: tensordot, split/stack, matmul, softmax over the batch axis, residual, ReLU; autograd backward).  Each
figure is the median over 15 timed regions of 10 calls, after a warm-up.  Bounds from shapes: HBM bytes at 8 TB/s
(X read by every pass, Y written, dY read) and fp32 FLOP at 157.3 TFLOP/s (VALU).
Prints one JSON line per config.  Usage: python scripts/exp/autoint_time.py [AI AI26]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import functional as Fn  # noqa: E402
from tests import autoint_ref as AR  # noqa: E402

HBM, VALU = 8.0e12, 157.3e12
REGIONS, CALLS = 15, 10


def region(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3          # us per call


def run(name):
    B, Fc, E = (16384, 10, 8) if name == "AI" else (8192, 26, 16)
    C, H, L = 3, 2, 2
    F = Fc + C
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand((B, Fc, E), device="cuda", generator=g) - 0.5) / 10
    xc = torch.randn((B, C), device="cuda", generator=g)
    ce = ((torch.rand((C, E), device="cuda", generator=g) - 0.5) / 10)
    Ws = [(torch.randn((E, E), device="cuda", generator=g) * 0.05) for _ in range(3 * L)]
    dy = torch.rand((B, F, E), device="cuda", generator=g)
    leaves = [t.clone().requires_grad_() for t in [x, ce] + Ws]

    def hip_fwd():
        with torch.no_grad():
            y = Fn.AutoIntAttention.apply(x, xc, ce, Ws[0], Ws[1], Ws[2], None, H, 1, False)
            for k in range(1, L):
                y = Fn.AutoIntAttention.apply(y, None, None, Ws[3 * k], Ws[3 * k + 1], Ws[3 * k + 2], None, H, 1, False)
        return y

    def hip_step():
        lx, lce, *lw = leaves
        y = Fn.AutoIntAttention.apply(lx, xc, lce, lw[0], lw[1], lw[2], None, H, 1, False)
        for k in range(1, L):
            y = Fn.AutoIntAttention.apply(y, None, None, lw[3 * k], lw[3 * k + 1], lw[3 * k + 2], None, H, 1, False)
        torch.autograd.grad(y, leaves, dy)

    def torch_fwd():
        with torch.no_grad():
            y = AR.assemble_dense(x, ce, xc)
            for k in range(L):
                y = AR.attention_torch(y, Ws[3 * k], Ws[3 * k + 1], Ws[3 * k + 2], H)
        return y

    def torch_step():
        lx, lce, *lw = leaves
        y = AR.assemble_dense(lx, lce, xc)
        for k in range(L):
            y = AR.attention_torch(y, lw[3 * k], lw[3 * k + 1], lw[3 * k + 2], H)
        torch.autograd.grad(y, leaves, dy)

    fns = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_step": hip_step, "torch_step": torch_step}
    for fn in fns.values():                          # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REGIONS):                         # alternate the formulations region by region
        for k, fn in fns.items():
            times[k].append(region(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    diff = float((hip_fwd() - torch_fwd()).abs().max() / torch_fwd().abs().max())
    # per layer: forward reads X twice (stats, out) and writes Y; backward reads X, Y, dY twice and writes dX
    fe = 4.0 * B * F * E
    fwd_bytes, bwd_bytes = L * 3 * fe, L * 7 * fe
    qkv = 2.0 * B * F * E * E
    att = 2.0 * B * H * F * F * (E // H)
    fwd_flop = L * (2 * qkv + att + 3 * qkv + 2 * att)            # stats: Q, K, S; out: Q, K, V, S, PV
    bwd_flop = L * (3 * qkv + 2 * att + 3 * qkv + 6 * att + 3 * qkv + 3 * qkv)
    out = {"config": name, "B": B, "F": F, "E": E, "H": H, "layers": L}
    out.update({k + "_us": v for k, v in med.items()})
    out.update({"hip_bwd_us": med["hip_step"] - med["hip_fwd"],
                "fwd_hbm_bound_us": fwd_bytes / HBM * 1e6, "step_hbm_bound_us": (fwd_bytes + bwd_bytes) / HBM * 1e6,
                "fwd_flop_bound_us": fwd_flop / VALU * 1e6, "step_flop_bound_us": (fwd_flop + bwd_flop) / VALU * 1e6,
                "hip_step_speedup_vs_torch": med["torch_step"] / med["hip_step"],
                "hip_fwd_speedup_vs_torch": med["torch_fwd"] / med["hip_fwd"], "max_rel_diff_vs_torch": diff,
                "spread_hip_step_us": [min(times["hip_step"]), max(times["hip_step"])],
                "spread_torch_step_us": [min(times["torch_step"]), max(times["torch_step"])]})
    return out


if __name__ == "__main__":
    for n in sys.argv[1:] or ["AI", "AI26"]:
        print(json.dumps(run(n)), flush=True)
