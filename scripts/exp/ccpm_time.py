#!/usr/bin/env python3
"""Time the fused CCPM kernel pair (csrc/ccpm.hip) at configs CC (10 fields, B = 16384) and CC26 (26 fields, B = 8192),
V = 10M, E = 16, filters [4,6], kernel_width [4,2]: the forward (ids + table -> out [B, 3 E 6]) and the forward +
backward (-> IndexedSlices values and the conv gradients), each with the backward gathering the rows again and with the
rows saved by the forward.  In the same process and alternating with them region by region:
  * the floor of the forward: emb_fm_fwd (the FM sum-square kernel) on the same ids and table -- it reads the same rows
    and writes less;
  * the torch formulation on the GPU: tests/ccpm_ref.py's transcription (gather, pad + conv2d, tanh, sort, Flatten;
    autograd backward down to the gathered rows).
Each figure is the median (with p10 / p90) over 15 timed regions of 10 calls, after a warm-up, from device events.
Prints one JSON line per config.  Usage: python scripts/exp/ccpm_time.py [CC CC26]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import ops  # noqa: E402
from tests import ccpm_ref as CR  # noqa: E402

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


def run(name):
    B, F = (16384, 10) if name == "CC" else (8192, 26)
    V, E, filters, kw = 10_000_000, 16, [4, 6], [4, 2]
    ks = ops.ccpm_k(E, len(filters))
    g = torch.Generator(device="cuda").manual_seed(0)
    table = torch.randn((V, E), device="cuda", generator=g) * 0.5
    w = torch.randn((V, 1), device="cuda", generator=g) * 0.05
    bias = torch.zeros(1, device="cuda")
    X = torch.randint(0, V, (B, F), device="cuda", generator=g)
    params = CR.make_params(filters, kw, 1)
    flat = torch.from_numpy(CR.flat_params(params)).cuda()
    do = torch.rand((B, ks[-1] * E * filters[-1]), device="cuda", generator=g) * 2 - 1
    leaves = [torch.from_numpy(a).cuda().requires_grad_() for kb in params for a in kb]

    def fm_fwd():
        return ops.emb_fm_fwd(table, w, bias, X, want_sum=True)

    def hip_fwd():
        return ops.emb_ccpm_fwd(table, X, flat, filters, kw)[0]

    def hip_fwd_rows():
        return ops.emb_ccpm_fwd(table, X, flat, filters, kw, want_rows=True)[0]

    def hip_step():
        ops.emb_ccpm_fwd(table, X, flat, filters, kw)
        return ops.emb_ccpm_bwd(table, X, flat, filters, kw, do)

    def hip_step_rows():
        _, rows = ops.emb_ccpm_fwd(table, X, flat, filters, kw, want_rows=True)
        return ops.emb_ccpm_bwd(table, X, flat, filters, kw, do, rows)

    def torch_fwd():
        with torch.no_grad():
            return CR.ccpm_torch(table[X], leaves, ks)

    def torch_step():
        rows = table[X].requires_grad_()
        return torch.autograd.grad(CR.ccpm_torch(rows, leaves, ks), [rows] + leaves, do)

    fns = {"fm_fwd": fm_fwd, "hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_fwd_rows": hip_fwd_rows,
           "hip_step": hip_step, "torch_step": torch_step, "hip_step_rows": hip_step_rows}
    for fn in fns.values():                          # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(REGIONS):                         # alternate the formulations region by region
        for k, fn in fns.items():
            times[k].append(region(fn))
    out = {"config": name, "B": B, "F": F, "E": E, "filters": filters, "kernel_width": kw, "V": V, "regions": REGIONS,
           "calls_per_region": CALLS}
    for k, v in times.items():
        out[k + "_us"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)),
                          "p90": float(np.percentile(v, 90))}
    med = {k: float(np.median(v)) for k, v in times.items()}
    ot = torch_fwd()
    fwd_bytes = B * F * (8 + 4 * E) + B * ks[-1] * E * filters[-1] * 4
    out.update({"max_rel_diff_vs_torch": float((hip_fwd() - ot).abs().max() / ot.abs().max()),
                "fwd_algorithmic_bytes": fwd_bytes, "fwd_hbm_bound_us": fwd_bytes / HBM * 1e6,
                "hip_fwd_over_fm_floor": med["hip_fwd"] / med["fm_fwd"],
                "hip_fwd_speedup_vs_torch": med["torch_fwd"] / med["hip_fwd"],
                "hip_step_speedup_vs_torch": med["torch_step"] / med["hip_step"],
                "hip_step_rows_over_gather_again": med["hip_step_rows"] / med["hip_step"]})
    return out


if __name__ == "__main__":
    for n in sys.argv[1:] or ["CC", "CC26"]:
        print(json.dumps(run(n)), flush=True)
