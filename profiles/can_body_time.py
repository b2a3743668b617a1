"""Forward + backward of the CAN co-action with its lookups at B = 8192, T = 50, E = 16, layer_unit_coef [1,1,1], order 3,
tanh, V = 160000, in both output modes (the list of per-order outputs; the sum over orders and positions), each two ways:
(1) the fused entry points of csrc/can.hip (functional.CoAction: both lookups are part of the kernel); (2) the same
arithmetic composed from what existed before them -- functional.Gather for the feed lookup and the three induction
lookups -- and torch for the powers, bmm, tanh, where and the sum.  Both deliver every table's gradient as de-duplicated
sparse rows through the same plan + segment sum.  Each path is captured in one hipGraph (so the figure is device time, not
Python) and replayed; the median and the min-max spread of REPS timed groups of INNER replays are printed with the kernel
count of one iteration, as one JSON line.  The line also gives each path's distance from the same body in fp64 (plain
torch on the device, not timed): max |difference| of the output, and of the feed table's gradient relative to its largest
entry.
Usage: python profiles/can_body_time.py > profiles/can_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, T, E, COEFS, ORDER, V = 8192, 50, 16, (1, 1, 1), 3, 160000
P = ops.can_row_floats(E, COEFS)
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda()
    p = {"feed": n(V, E, std=0.5).requires_grad_()}
    for o in range(ORDER):
        p["ind%d" % o] = n(V, P, std=E ** -0.5).requires_grad_()
    fid = torch.randint(1, V, (B, T), generator=g)
    n_valid = torch.randint(0, T + 1, (B,), generator=g)
    fid *= (torch.rand(B, T, generator=g).argsort(1) < n_valid[:, None])                 # padding anywhere in the row
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    d = {"fid": fid.cuda(), "iid": torch.randint(0, V, (B,), generator=g).cuda(), "gout": u(ORDER, B, T, E),
         "gpool": u(B, E)}
    return p, d


def co_action(f, vs, pad, pooled):
    """f [B,T,E] looked-up feed rows, vs the looked-up induction row [B,P] of every order: CoActionUnit.basic_call"""
    outs = []
    for o, v in enumerate(vs):
        x, at = f ** (o + 1), 0
        for _ in range(min(len(COEFS), ORDER)):
            W, Bv = v[:, at:at + E * E].reshape(-1, E, E), v[:, at + E * E:at + E * E + E]
            x = torch.tanh(torch.bmm(x, W) + Bv[:, None, :])
            at += E * E + E
        outs.append(torch.where(pad, torch.zeros((), dtype=x.dtype, device=x.device), x))
    return torch.cat(outs, dim=1).sum(1) if pooled else torch.stack(outs)


def fused(p, d, pooled):
    return Fn.CoAction.apply(p["feed"], d["iid"], d["fid"], COEFS, ORDER, ops.ACT_TANH, 0, pooled, None,
                             *[p["ind%d" % o] for o in range(ORDER)])


def composed(p, d, pooled):
    f = Fn.Gather.apply(p["feed"], d["fid"], None, None)
    vs = [Fn.Gather.apply(p["ind%d" % o], d["iid"][:, None], None, None).reshape(B, P) for o in range(ORDER)]
    return co_action(f, vs, (d["fid"] == 0)[:, :, None], pooled)


def loss_of(y, d, pooled):
    return (y * d["gpool" if pooled else "gout"]).sum()


def reference64(p, d, pooled):
    """the body in fp64, plain torch autograd -> (output, the feed table's dense gradient)"""
    feed = p["feed"].detach().double().requires_grad_()
    vs = [p["ind%d" % o].detach()[d["iid"]].double() for o in range(ORDER)]
    y = co_action(feed[d["fid"]], vs, (d["fid"] == 0)[:, :, None], pooled)
    loss_of(y, {k: v.double() if v.is_floating_point() else v for k, v in d.items()}, pooled).backward()
    return y.detach(), feed.grad


def measure(body, p, d, pooled):
    def step():
        for t in p.values():
            t.grad = None
        y = body(p, d, pooled)
        loss_of(y, d, pooled).backward()
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
    return y.detach().clone(), p["feed"].grad.to_dense(), {
        "median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
        "max_us": round(max(times), 1), "kernels": kernels}


def main():
    p, d = make()
    res = {"shape": {"B": B, "T": T, "E": E, "coefs": list(COEFS), "order": ORDER, "P": P, "V": V, "act": "tanh"}}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for name, pooled in (("unpooled", False), ("pooled", True)):
        y64, g64 = reference64(p, d, pooled)
        dist = lambda y, g: {"out": float((y - y64).abs().max()), "dfeed_rel": rel(g, g64)}
        yf, gf, rf = measure(fused, p, d, pooled)
        yc, gc, rc = measure(composed, p, d, pooled)
        res[name] = {"fused": rf, "composed": rc,
                     "spreads_overlap": not (rf["max_us"] < rc["min_us"] or rc["max_us"] < rf["min_us"]),
                     "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                     "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}
        del y64, g64, yf, gf, yc, gc
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
