"""Forward + backward of the lookup and the PLE body at B = 8192, F = 9, E = 8, three tasks, 3 + 3 experts, two levels,
two ways: (1) the gather and the fused entry points of csrc/ple.hip (functional.PLELevel, one per level); (2) the same
arithmetic composed from the entry points that existed before them -- the gather, rec_gemm_f32 with its epilogues
through functional.LinearAct (one call per layer of every expert, gate and tower, as MLPLayer runs them), the dedup +
segment sum, and torch for the softmax, the stack, the gate multiply and the sum over the experts.  Each path is
captured in one hipGraph (so the figure is device time, not Python) and replayed; the median and the min-max spread of
REPS timed groups of INNER replays are printed with the kernel count of one iteration and the device time of every
kernel of one eager iteration of the fused path, as one JSON line.  The line also gives the two paths' distance from
each other and from the same body in fp64 (plain torch on the device, not timed): max |difference| of the output, and of
two gradients relative to their largest entry.
Usage: python profiles/ple_body_time.py > profiles/ple_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, F, E, T, S, SH, L, H1, O, OG, V = 8192, 9, 8, 3, 3, 3, 2, 64, 8, 8, 160000
D, NE, NS = F * E, T * S + SH, S + SH
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda().requires_grad_()
    he = lambda a, b: n(a, b, std=(2.0 / a) ** 0.5)
    mlp = lambda din: [(he(din, H1), n(H1, std=0.5)), (he(H1, O), n(O, std=0.5))]
    levels = []
    for lv in range(L):
        din, last = (D if lv == 0 else O), lv == L - 1
        levels.append({"experts": [mlp(din) for _ in range(NE)],
                       "gates": [mlp(din) + [he(OG, NS)] for _ in range(T)] + ([] if last else [mlp(din) + [he(OG, NE)]])})
    p = {"table": n(V, E, std=0.5), "levels": levels, "towers": [(he(O, 1), n(1, std=0.5)) for _ in range(T)]}
    X = torch.randint(0, V, (B, F), generator=g).cuda()
    dout = (torch.rand(B, T, generator=g) * 2 - 1).cuda()
    return p, X, dout


def leaves(p):
    out = [p["table"]] + [t for wb in p["towers"] for t in wb]
    for lv in p["levels"]:
        out += [t for m in lv["experts"] for wb in m for t in wb]
        out += [t for m in lv["gates"] for wb in m[:2] for t in wb] + [m[2] for m in lv["gates"]]
    return out


def packed(p, lv):
    last = lv == L - 1
    experts, gates = p["levels"][lv]["experts"], p["levels"][lv]["gates"]
    first = experts + gates
    cat, stack = torch.cat, torch.stack
    return (cat([m[0][0] for m in first], dim=1), cat([m[0][1] for m in first]),
            stack([m[1][0] for m in experts]), stack([m[1][1] for m in experts]),
            stack([m[1][0] for m in gates]), stack([m[1][1] for m in gates]), stack([m[2] for m in gates[:T]]),
            None if last else gates[T][2], stack([w.reshape(-1) for w, _ in p["towers"]]) if last else None,
            cat([b for _, b in p["towers"]]) if last else None)


def fused(p, X):
    y = Fn.Gather.apply(p["table"], X, None, None).reshape(B, 1, D)
    for lv in range(L - 1):
        y = Fn.PLELevel.apply(y, T, S, SH, False, *packed(p, lv))
    return Fn.PLELevel.apply(y, T, S, SH, True, *packed(p, L - 1))[1]


def _body(p, x, linear, softmax_dense):
    """the reference's op order over ``linear(inp, W, b, act)``"""
    relu2 = lambda m, inp: linear(linear(inp, m[0][0], m[0][1], "relu"), m[1][0], m[1][1], "relu")
    inputs = [x] * (T + 1)
    for lv in range(L):
        experts, gates = p["levels"][lv]["experts"], p["levels"][lv]["gates"]
        spec = [relu2(experts[i * S + j], inputs[i]) for i in range(T) for j in range(S)]
        shared = [relu2(experts[T * S + k], inputs[-1]) for k in range(SH)]
        outs = []
        for t in range(T):
            cur = torch.stack(spec[t * S:(t + 1) * S] + shared, dim=1)
            g = torch.softmax(softmax_dense(relu2(gates[t], inputs[t]), gates[t][2]), dim=-1)
            outs.append((cur * g.unsqueeze(-1)).sum(1))
        if lv < L - 1:
            cur = torch.stack(spec + shared, dim=1)
            g = softmax_dense(relu2(gates[T], inputs[-1]), gates[T][2])
            outs.append((cur * g.unsqueeze(-1)).sum(1))
        inputs = outs
    return torch.cat([linear(inputs[t], w, b, "sigmoid") for t, (w, b) in enumerate(p["towers"])], dim=1)


def composed(p, X):
    x = Fn.Gather.apply(p["table"], X, None, None).reshape(B, D)
    linear = lambda inp, W, b, act: Fn.LinearAct.apply(inp, W, b, ops.ACT_CODE[act])
    return _body(p, x, linear, lambda q, W: torch.softmax(Fn.LinearAct.apply(q, W, None, ops.ACT_NONE), dim=-1))


def reference64(p, X, dout):
    """the body in fp64, plain torch autograd -> out, the gradient of level 0's expert 0 first kernel and of the last
    level's task gate 0 dense kernel"""
    d = lambda t: t.detach().double().requires_grad_()
    q = {"levels": [{k: [[tuple(d(t) for t in wb) if isinstance(wb, tuple) else d(wb) for wb in m] for m in lv[k]]
                     for k in ("experts", "gates")} for lv in p["levels"]],
         "towers": [(d(w), d(b)) for w, b in p["towers"]]}
    act = {"relu": torch.relu, "sigmoid": torch.sigmoid}
    x = p["table"].detach().double()[X].reshape(B, D)
    out = _body(q, x, lambda inp, W, b, a: act[a](inp @ W + b), lambda g, W: torch.softmax(g @ W, dim=-1))
    out.backward(dout.double())
    return out.detach(), q["levels"][0]["experts"][0][0][0].grad, q["levels"][L - 1]["gates"][0][2].grad


def probe_grads(p):
    return [p["levels"][0]["experts"][0][0][0].grad.clone(), p["levels"][L - 1]["gates"][0][2].grad.clone()]


def measure(body, p, X, dout, breakdown=False):
    def step():
        for t in leaves(p):
            t.grad = None
        y = body(p, X)
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
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
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
    res = {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
           "max_us": round(max(times), 1), "kernels": len(dev)}
    if breakdown:                                         # device time per kernel name of the one eager iteration
        per = {}
        for e in dev:
            name = e.name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split(" ")[-1][-60:]
            cnt, us = per.get(name, (0, 0.0))
            per[name] = (cnt + 1, us + e.device_time)
        res["per_kernel_us"] = {k: {"launches": c, "us": round(us, 1)}
                                for k, (c, us) in sorted(per.items(), key=lambda kv: -kv[1][1])}
    return y.detach().clone(), probe_grads(p), res


def main():
    p, X, dout = make()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    yf, gf, rf = measure(fused, p, X, dout, breakdown=True)
    yc, gc, rc = measure(composed, p, X, dout)
    y64, e64, g64 = reference64(p, X, dout)
    dist = lambda y, g: {"out": float((y - y64).abs().max()), "dexpert0_kernel0_rel": rel(g[0], e64),
                         "dgate0_dense_rel": rel(g[1], g64)}
    res = {"shape": {"B": B, "F": F, "E": E, "tasks": T, "specific": S, "shared": SH, "levels": L, "H1": H1, "O": O,
                     "Og": OG, "V": V},
           "ple": {"fused": rf, "composed": rc, "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                   "fused_vs_composed": {"out": float((yf - yc).abs().max()), "dexpert0_kernel0_rel": rel(gf[0], gc[0]),
                                         "dgate0_dense_rel": rel(gf[1], gc[1])},
                   "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
