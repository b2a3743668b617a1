#!/usr/bin/env python3
"""Time the fused FGCNN kernel pair (csrc/fgcnn.hip) at configs FG (10 fields, B = 16384) and FG26 (26 fields,
B = 8192), V = 10M, E = 16, filters [14,16], kernel_width [7,7], pooling_width [2,2]: the forward (ids + table -> rows
and every pooled map) and the forward + backward (-> IndexedSlices values and the conv gradients, from a gradient at
every pooled map and one straight onto the rows).  In the same process and alternating with them region by region:
  * the floor of the forward: emb_fm_fwd (the FM sum-square kernel) on the same ids and table -- it reads the same rows
    and writes less;
  * the torch formulation on the GPU: tests/fgcnn_ref.py's transcription up to and excluding the Dense layers (gather,
    pad + conv2d, tanh, max_pool2d, Flatten; autograd backward down to the gathered rows).
Every formulation is captured in a hipGraph after its warm-up and replayed (``graphed`` says which ones were; one that
cannot be captured is timed eagerly and says so).  Each figure is the median (with p10 / p90) over 15 timed regions of
10 replays, from device events.  Prints one JSON line per config.  Usage: python scripts/exp/fgcnn_time.py [FG FG26]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import ops  # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE  # noqa: E402
from tests import ccpm_ref as CR  # noqa: E402
from tests import fgcnn_ref as FR  # noqa: E402

HBM = 8.0e12
REGIONS, CALLS = 15, 10


def region(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3          # us per call


def graphed(fn):
    """Warm up on a side stream, capture, -> (replay, True); (fn, False) when the capture fails."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
            keep = fn()
        graph.replay()
        torch.cuda.synchronize()
    except RuntimeError:
        torch.cuda.synchronize()
        return fn, False
    graph.keep = keep
    return graph.replay, True


def run(name):
    B, F = (16384, 10) if name == "FG" else (8192, 26)
    V, E, filters, kw, pws = 10_000_000, 16, [14, 16], [7, 7], [2, 2]
    hs = ops.fgcnn_heights(F, pws)
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn((V, E), device="cuda", generator=g) * 0.5
    w = torch.randn((V, 1), device="cuda", generator=g) * 0.05
    bias = torch.zeros(1, device="cuda")
    X = torch.randint(0, V, (B, F), device="cuda", generator=g)
    params = CR.make_params(filters, kw, 1)
    flat = torch.from_numpy(CR.flat_params(params)).cuda()
    dps = [torch.rand((B, h * E * c), device="cuda", generator=g) * 2 - 1 for h, c in zip(hs, filters)]
    dd = torch.rand((B, F, E), device="cuda", generator=g) * 2 - 1
    leaves = [torch.from_numpy(a).cuda().requires_grad_() for kb in params for a in kb]

    def fm_fwd():
        return ops.emb_fm_fwd(table, w, bias, X, want_sum=True)

    def hip_fwd():
        return ops.emb_fgcnn_fwd(table, X, flat, filters, kw, pws)

    def hip_step():
        rows, pooled = ops.emb_fgcnn_fwd(table, X, flat, filters, kw, pws)
        return ops.emb_fgcnn_bwd(rows, flat, filters, kw, pws, dps, dd)

    def torch_fwd():
        with torch.no_grad():
            return FR.fgcnn_torch(table[X], leaves, pws)

    def torch_step():
        rows = table[X].requires_grad_()
        outs = FR.fgcnn_torch(rows, leaves, pws)
        return torch.autograd.grad(outs + [rows], [rows] + leaves, dps + [dd])

    eager = {"fm_fwd": fm_fwd, "hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_step": hip_step, "torch_step": torch_step}
    fns, was_graphed = {}, {}
    for k, fn in eager.items():
        fns[k], was_graphed[k] = graphed(fn)
    times = {k: [] for k in fns}
    for _ in range(REGIONS):                         # alternate the formulations region by region
        for k, fn in fns.items():
            times[k].append(region(fn))
    out = {"config": name, "B": B, "F": F, "E": E, "filters": filters, "kernel_width": kw, "pooling_width": pws, "V": V,
           "regions": REGIONS, "calls_per_region": CALLS, "graphed": was_graphed}
    for k, v in times.items():
        out[k + "_us"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)),
                          "p90": float(np.percentile(v, 90))}
    med = {k: float(np.median(v)) for k, v in times.items()}
    ot = torch_fwd()
    _, oh = hip_fwd()
    fwd_bytes = B * F * (8 + 8 * E) + sum(B * h * E * c * 4 for h, c in zip(hs, filters))
    out.update({"max_rel_diff_vs_torch": max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(oh, ot)),
                "fwd_algorithmic_bytes": fwd_bytes, "fwd_hbm_bound_us": fwd_bytes / HBM * 1e6,
                "hip_fwd_over_fm_floor": med["hip_fwd"] / med["fm_fwd"],
                "hip_fwd_speedup_vs_torch": med["torch_fwd"] / med["hip_fwd"],
                "hip_step_speedup_vs_torch": med["torch_step"] / med["hip_step"]})
    return out


if __name__ == "__main__":
    for n in sys.argv[1:] or ["FG", "FG26"]:
        print(json.dumps(run(n)), flush=True)
