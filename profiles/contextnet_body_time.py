"""Forward + backward of the default ContextNet body (input stage + six pointwise blocks, no head) at B = 8192, F = 13,
E = 16, two ways: (1) the fused entry points of csrc/contextnet.hip (functional.EmbScaledLookup / ContextNetBlock);
(2) composed from the entry points that existed before them -- rec_emb_gather_f32, rec_gemm_f32 with its epilogues,
rec_layernorm_*, rec_feat_act_*, the dedup + segment sum, and torch for the elementwise multiplies, the residual and the
per-field slices and stack.  Each path is captured in one hipGraph (so the figure is device time, not Python) and
replayed; the median and the min-max spread of REPS timed groups of INNER replays are printed with the kernel count of
one iteration, as one JSON line.  The body is six blocks deep, so rounding differences between two fp32 paths grow
from block to block and flip relus; the line therefore also gives each path's distance from the same body in fp64
(plain torch on the device, not timed): max |difference| of y, and of two gradients relative to their largest entry.
Usage: python profiles/contextnet_body_time.py > profiles/contextnet_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, Fc, Fk, E, NB, R, V = 8192, 10, 3, 16, 6, 3, 160000
F, D = Fc + Fk, (Fc + Fk) * E
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda()
    p = {"table": n(V, E, std=0.5).requires_grad_(), "blocks": []}
    lim = lambda a, b: (6.0 / (a + b)) ** 0.5
    u = lambda a, b: ((torch.rand(a, b, generator=g) * 2 - 1) * lim(a, b)).cuda().requires_grad_()
    for _ in range(NB):
        p["blocks"].append([u(D, R * D), n(R * D, std=0.1).requires_grad_(), u(R * D, D), n(D, std=0.1).requires_grad_(),
                            n(F, E, E, std=(1.0 / E) ** 0.5).requires_grad_(),
                            n(F, E, E, std=(1.0 / E) ** 0.5).requires_grad_(), (1 + n(F, E, std=0.1)).requires_grad_(),
                            n(F, E, std=0.1).requires_grad_()])
    X = torch.randint(0, V, (B, F), generator=g).cuda()
    values = n(B, Fk)
    dy = (torch.rand(B, D, generator=g) * 2 - 1).cuda()
    return p, X, values, dy


def leaves(p):
    return [p["table"]] + [t for b in p["blocks"] for t in b]


def fused(p, X, values):
    x = Fn.EmbScaledLookup.apply(p["table"], X, values, None)
    for blk in p["blocks"]:
        x = Fn.ContextNetBlock.apply(x, *blk)
    return x


def composed(p, X, values):
    rows = Fn.Gather.apply(p["table"], X, None, None).reshape(B, F, E)
    scale = torch.cat([torch.ones(B, Fc, device="cuda"), values], dim=1).unsqueeze(-1)
    x = (rows * scale).reshape(B, D)
    for Wa, ba, Wb, bb, W1, W2, g, be in p["blocks"]:
        h = Fn.LinearAct.apply(x, Wa, ba, ops.ACT_RELU)
        m = Fn.LinearAct.apply(h, Wb, bb, ops.ACT_NONE)
        u = (x * m).reshape(B, F, E)
        outs = []
        for f in range(F):
            inp = u[:, f, :]
            a = Fn.FeatAct.apply(Fn.LinearAct.apply(inp, W1[f], None, ops.ACT_NONE), ops.DACT_RELU, None, None, None)
            outs.append(Fn.LayerNorm.apply(Fn.LinearAct.apply(a, W2[f], None, ops.ACT_NONE) + inp, g[f], be[f]))
        x = torch.stack(outs, dim=1).reshape(B, D)
    return x


def reference64(p, X, values, dy):
    """the body in fp64, plain torch autograd -> y, dWa and dW1 of the first block"""
    d = lambda t: t.detach().double().requires_grad_()
    x = p["table"].detach().double()[X]
    x = (x * torch.cat([torch.ones(B, Fc, device="cuda", dtype=torch.float64), values.double()], dim=1).unsqueeze(-1))
    x, first = x.reshape(B, D), None
    for blk in p["blocks"]:
        Wa, ba, Wb, bb, W1, W2, g, be = [d(t) for t in blk]
        first = first or (Wa, W1)
        u = (x * (torch.relu(x @ Wa + ba) @ Wb + bb)).reshape(B, F, E)
        r = torch.einsum("bfe,fej->bfj", torch.relu(torch.einsum("bfe,fej->bfj", u, W1)), W2) + u
        mean, var = r.mean(-1, keepdim=True), r.var(-1, unbiased=False, keepdim=True)
        x = ((r - mean) / torch.sqrt(var + 1e-3) * g + be).reshape(B, D)
    x.backward(dy.double())
    return x.detach(), first[0].grad, first[1].grad


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
    gf = [p["blocks"][0][0].grad.clone(), p["blocks"][0][4].grad.clone()]
    yc, rc = measure(composed, p, X, values, dy)
    gc = [p["blocks"][0][0].grad, p["blocks"][0][4].grad]
    gc = [t.clone() for t in gc]
    y64, a64, w64 = reference64(p, X, values, dy)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    dist = lambda y, g: {"y": float((y - y64).abs().max()), "dWa_rel": rel(g[0], a64), "dW1_rel": rel(g[1], w64)}
    agree = {"y": float((yf - yc).abs().max()), "dWa_rel": rel(gf[0], gc[0]), "dW1_rel": rel(gf[1], gc[1])}
    print(json.dumps({"shape": {"B": B, "F": F, "E": E, "NB": NB, "R": R, "mode": "pointwise"}, "fused": rf,
                      "composed": rc, "fused_vs_composed": agree, "fused_vs_fp64": dist(yf, gf),
                      "composed_vs_fp64": dist(yc, gc)}))


if __name__ == "__main__":
    main()
