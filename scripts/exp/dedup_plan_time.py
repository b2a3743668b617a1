#!/usr/bin/env python3
"""Time rec_dedup_plan_i64 on the flat ids of one DSSM tower at config D (n = B*F = 16384 user / 24576 item lookups,
uniform ids over 100M rows): 50 plans per captured hipGraph, 4 replays timed with events.  Prints one JSON line (us per
plan)."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from explicit_tf2_recommendation_amd._lib import lib, check  # noqa: E402

V = 100_000_000
res = {}
for n in (16384, 24576):
    ids = torch.randint(0, V, (n,), dtype=torch.int64, device="cuda")
    uniq = torch.empty(n, dtype=torch.int64, device="cuda")
    seg = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    nu = torch.empty(1, dtype=torch.int64, device="cuda")
    wb = lib.rec_dedup_workspace_bytes(n)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")

    def p(t):
        return C.c_void_p(t.data_ptr())

    def plan():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(lib.rec_dedup_plan_i64(p(ids), n, V, p(uniq), p(seg), p(perm), p(nu), p(ws), wb, st), "plan")
    for _ in range(20):
        plan()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(50):
            plan()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    res[n] = e0.elapsed_time(e1) / 200 * 1e3
print(json.dumps({"rec_dedup_plan_i64_us_graphed_uniform_V100M": res}))
