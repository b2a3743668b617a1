"""Forward + backward of the serial default MaskNet body (input stage + six mask blocks, no head) at B = 8192, F = 13,
E = 16, O = 32, two ways: (1) the fused entry points of csrc/masknet.hip (functional.EmbFieldLayerNorm / MaskBlock);
(2) composed from the entry points that existed before them -- rec_emb_gather_f32, rec_gemm_f32 with its epilogues,
rec_layernorm_*, rec_feat_act_* / rec_act_*, the dedup + segment sum, and torch for the elementwise multiplies and the
per-field slices.  Each path is captured in one hipGraph (so the figure is device time, not Python) and replayed; the
median and the min-max spread of REPS timed groups of INNER replays are printed with the kernel count of one
iteration, as one JSON line.  Usage: python profiles/masknet_body_time.py > profiles/masknet_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, Fc, Fk, E, O, NB, R, V = 8192, 10, 3, 16, 32, 6, 3, 160000
F, D = Fc + Fk, (Fc + Fk) * E
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda()
    p = {"table": n(V, E, std=0.5).requires_grad_(), "gamma": (1 + n(F, E, std=0.1)).requires_grad_(),
         "beta": n(F, E, std=0.1).requires_grad_(), "blocks": []}
    for k in range(NB):
        P = D if k == 0 else O
        lim = lambda a, b: (6.0 / (a + b)) ** 0.5
        u = lambda a, b: ((torch.rand(a, b, generator=g) * 2 - 1) * lim(a, b)).cuda().requires_grad_()
        p["blocks"].append([u(D, R * P), n(R * P, std=0.1).requires_grad_(), u(R * P, P), n(P, std=0.1).requires_grad_(),
                            u(P, O), n(O, std=0.1).requires_grad_(), (1 + n(O, std=0.1)).requires_grad_(),
                            n(O, std=0.1).requires_grad_()])
    X = torch.randint(0, V, (B, F), generator=g).cuda()
    values = n(B, Fk)
    dy = (torch.rand(B, O, generator=g) * 2 - 1).cuda()
    return p, X, values, dy


def leaves(p):
    return [p["table"], p["gamma"], p["beta"]] + [t for b in p["blocks"] for t in b]


def fused(p, X, values):
    x_emb, x_norm = Fn.EmbFieldLayerNorm.apply(p["table"], X, values, p["gamma"], p["beta"], None)
    sink = Fn.MaskDxSink(NB)
    x = x_norm
    for blk in p["blocks"]:
        x = Fn.MaskBlock.apply(x_emb, x, *blk, sink)
    return x


def composed(p, X, values):
    rows = Fn.Gather.apply(p["table"], X, None, None).reshape(B, F, E)
    scale = torch.cat([torch.ones(B, Fc, device="cuda"), values], dim=1).unsqueeze(-1)
    rows = rows * scale
    normed = torch.stack([Fn.LayerNorm.apply(rows[:, f, :], p["gamma"][f], p["beta"][f]) for f in range(F)], dim=1)
    x_emb, x = rows.reshape(B, D), normed.reshape(B, D)
    for W1, b1, W2, b2, W3, b3, g, be in p["blocks"]:
        h = Fn.LinearAct.apply(x_emb, W1, b1, ops.ACT_RELU)
        m = Fn.LinearAct.apply(h, W2, b2, ops.ACT_NONE)
        z = Fn.LinearAct.apply(x * m, W3, b3, ops.ACT_NONE)
        x = Fn.FeatAct.apply(Fn.LayerNorm.apply(z, g, be), ops.DACT_RELU, None, None, None)
    return x


def measure(body, p, X, values, dy):
    def step():
        for t in leaves(p):
            t.grad = None
        y = body(p, X, values)
        y.backward(dy)
        return y

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    kernels = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        y = step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / INNER * 1000.0)
    return y.detach().clone(), {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
                                "max_us": round(max(times), 1), "kernels": kernels}


def main():
    p, X, values, dy = make()
    yf, rf = measure(fused, p, X, values, dy)
    gf = p["blocks"][0][0].grad.clone()
    yc, rc = measure(composed, p, X, values, dy)
    gc = p["blocks"][0][0].grad
    agree = {"y": float((yf - yc).abs().max()), "dW1_rel": float((gf - gc).abs().max() / gc.abs().max())}
    print(json.dumps({"shape": {"B": B, "F": F, "E": E, "O": O, "NB": NB, "R": R}, "fused": rf, "composed": rc,
                      "fused_vs_composed": agree}))


if __name__ == "__main__":
    main()
