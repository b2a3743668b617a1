"""Forward + backward of the lookup and the MMOE / ESMM body at B = 8192, F = 9, E = 16, three experts, two tasks, two
ways: (1) the gather and the fused entry points of csrc/mmoe.hip (functional.MMOEBody); (2) the same arithmetic composed
from the entry points that existed before them -- the gather, rec_gemm_f32 with its epilogues through
functional.LinearAct (one call per layer of every expert, gate and tower, as MLPLayer runs them), the dedup + segment
sum, and torch for the softmax, the gate multiply, the stack and the flatten.  Each path is captured in one hipGraph (so
the figure is device time, not Python) and replayed; the median and the min-max spread of REPS timed groups of INNER
replays are printed with the kernel count of one iteration, as one JSON line.  The line also gives the two paths'
distance from each other and from the same body in fp64 (plain torch on the device, not timed): max |difference| of the
output, and of two gradients relative to their largest entry.
Usage: python profiles/mmoe_body_time.py > profiles/mmoe_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, F, E, N, T, H1, O, H2, O2, V = 8192, 9, 16, 3, 2, 64, 8, 64, 8, 160000
D = F * E
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda().requires_grad_()
    lim = lambda a, b: (6.0 / (a + b)) ** 0.5
    u = lambda a, b: ((torch.rand(a, b, generator=g) * 2 - 1) * lim(a, b)).cuda().requires_grad_()
    mlp = lambda dims: [(u(a, b), n(b, std=0.1)) for a, b in zip(dims[:-1], dims[1:])]
    p = {"table": n(V, E, std=0.5), "experts": [mlp([D, H1, O]) for _ in range(N)],
         "gates": [mlp([D, H1, N]) for _ in range(T)], "towers": [mlp([N * O, H2, O2, 1]) for _ in range(T)]}
    X = torch.randint(0, V, (B, F), generator=g).cuda()
    dout = (torch.rand(B, T, generator=g) * 2 - 1).cuda()
    return p, X, dout


def leaves(p):
    return [p["table"]] + [t for k in ("experts", "gates", "towers") for m in p[k] for wb in m for t in wb]


def packed(p):
    first = p["experts"] + p["gates"]
    cat, stack = torch.cat, torch.stack
    return (cat([m[0][0] for m in first], dim=1), cat([m[0][1] for m in first]),
            stack([m[1][0] for m in p["experts"]]), stack([m[1][1] for m in p["experts"]]),
            stack([m[1][0] for m in p["gates"]]), stack([m[1][1] for m in p["gates"]]),
            stack([m[0][0] for m in p["towers"]]), stack([m[0][1] for m in p["towers"]]),
            stack([m[1][0] for m in p["towers"]]), stack([m[1][1] for m in p["towers"]]),
            stack([m[2][0].reshape(-1) for m in p["towers"]]), cat([m[2][1] for m in p["towers"]]))


def fused(p, X, passes, ctcvr):
    x = Fn.Gather.apply(p["table"], X, None, None).reshape(B, D)
    return Fn.MMOEBody.apply(x, passes, ctcvr, *packed(p))


def composed(p, X, passes, ctcvr):
    x = Fn.Gather.apply(p["table"], X, None, None).reshape(B, D)
    relu2 = lambda m, inp: Fn.LinearAct.apply(Fn.LinearAct.apply(inp, m[0][0], m[0][1], ops.ACT_RELU), m[1][0], m[1][1],
                                              ops.ACT_RELU)
    experts = torch.stack([relu2(m, x) for m in p["experts"]], dim=1)
    outs = []
    for gate, tower in zip(p["gates"], p["towers"]):
        g = relu2(gate, x)
        for _ in range(passes):
            g = torch.softmax(g, dim=-1)
        a = relu2(tower, (experts * g.unsqueeze(2)).reshape(B, N * O))
        outs.append(Fn.LinearAct.apply(a, tower[2][0], tower[2][1], ops.ACT_SIGMOID))
    if ctcvr:
        outs[1] = outs[0] * outs[1]
    return torch.cat(outs, dim=1)


def reference64(p, X, passes, ctcvr, dout):
    """the body in fp64, plain torch autograd -> out, the gradient of expert 0's first kernel and of tower 0's first"""
    d = lambda t: t.detach().double().requires_grad_()
    q = {k: [[(d(w), d(b)) for w, b in m] for m in p[k]] for k in ("experts", "gates", "towers")}
    x = p["table"].detach().double()[X].reshape(B, D)
    relu2 = lambda m, inp: torch.relu(torch.relu(inp @ m[0][0] + m[0][1]) @ m[1][0] + m[1][1])
    experts = torch.stack([relu2(m, x) for m in q["experts"]], dim=1)
    outs = []
    for gate, tower in zip(q["gates"], q["towers"]):
        g = relu2(gate, x)
        for _ in range(passes):
            g = torch.softmax(g, dim=-1)
        outs.append(torch.sigmoid(relu2(tower, (experts * g.unsqueeze(2)).reshape(B, N * O)) @ tower[2][0] + tower[2][1]))
    if ctcvr:
        outs[1] = outs[0] * outs[1]
    out = torch.cat(outs, dim=1)
    out.backward(dout.double())
    return out.detach(), q["experts"][0][0][0].grad, q["towers"][0][0][0].grad


def measure(body, p, X, passes, ctcvr, dout):
    def step():
        for t in leaves(p):
            t.grad = None
        y = body(p, X, passes, ctcvr)
        y.backward(dout)
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
    grads = [p["experts"][0][0][0].grad.clone(), p["towers"][0][0][0].grad.clone()]
    return y.detach().clone(), grads, {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
                                       "max_us": round(max(times), 1), "kernels": kernels}


def main():
    p, X, dout = make()
    res = {"shape": {"B": B, "F": F, "E": E, "experts": N, "tasks": T, "H1": H1, "O": O, "H2": H2, "O2": O2}}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for name, passes, ctcvr in (("mmoe", 1, False), ("esmm", 2, True)):
        yf, gf, rf = measure(fused, p, X, passes, ctcvr, dout)
        yc, gc, rc = measure(composed, p, X, passes, ctcvr, dout)
        y64, e64, t64 = reference64(p, X, passes, ctcvr, dout)
        dist = lambda y, g: {"out": float((y - y64).abs().max()), "dexpert0_kernel0_rel": rel(g[0], e64),
                             "dtower0_kernel0_rel": rel(g[1], t64)}
        res[name] = {"fused": rf, "composed": rc,
                     "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                     "fused_vs_composed": {"out": float((yf - yc).abs().max()), "dexpert0_kernel0_rel": rel(gf[0], gc[0]),
                                           "dtower0_kernel0_rel": rel(gf[1], gc[1])},
                     "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
