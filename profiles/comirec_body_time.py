"""Forward + backward of the three ComiRec bodies with their lookups at B = 8192, T = 50, C = 3, E = 16, K = 4, R = 3,
Ns = 11, each two ways: (1) the fused entry points of csrc/comirec.hip (functional.ComiRecRouting, ComiRecSelfAttention,
ComiRecSelect: the lookup is part of the kernel); (2) the same arithmetic composed from what existed before them -- the
gather and the dedup + segment sum of functional.Gather -- and torch for the einsums, the masked softmax, the squash,
tanh, the argmax + gather and the log-sum-exp.  Each path is captured in one hipGraph (so the figure is device time, not
Python) and replayed; the median and the min-max spread of REPS timed groups of INNER replays are printed with the kernel
count of one iteration, as one JSON line.  The line also gives each path's distance from the same body in fp64 (plain
torch on the device, not timed): max |difference| of the output, and of one gradient relative to its largest entry.
The mask is the layer's default, the reference read literally: the PADDED positions take part.
Usage: python profiles/comirec_body_time.py > profiles/comirec_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, layers      # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, T, C, E, K, R, NS, V = 8192, 50, 3, 16, 4, 3, 11, 160000
D = DC = C * E
FMIN = torch.finfo(torch.float32).min
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda()
    glorot = lambda a, b: n(a, b, std=(2.0 / (a + b)) ** 0.5)
    p = {"table": n(V, E, std=0.5).requires_grad_(), "W": n(K, T, D, DC, std=D ** -0.5).requires_grad_(),
         "B0": n(K, T, std=0.05), "W1": glorot(D, DC).requires_grad_(), "W2": glorot(K, DC).requires_grad_(),
         "m": n(B, K, DC, std=0.5).requires_grad_(), "pos": layers.comirec_positional_table(T, D).cuda()}
    series = torch.randint(1, V, (B, T, C), generator=g)
    n_valid = torch.randint(0, T + 1, (B,), generator=g)
    series[:, :, 0] *= (torch.rand(B, T, generator=g).argsort(1) < n_valid[:, None])     # padding anywhere in the row
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).cuda()
    d = {"series": series.cuda(), "items": torch.randint(0, V, (B, NS, C), generator=g).cuda(), "gcaps": u(B, K, DC),
         "ginner": u(B, NS), "gloss": u(B), "gsel": u(B, NS, DC)}
    return p, d


def routing(x, part, W, B0):
    u = torch.einsum("bse,nsec->bnsc", x, W)
    L = B0[None].expand(x.shape[0], -1, -1)
    drop = torch.full_like(L, FMIN)
    for i in range(R):
        Cw = torch.softmax(torch.where(part[:, None, :], L, drop), dim=2)
        s = torch.einsum("bns,bnsc->bnc", Cw, u)
        n = torch.linalg.vector_norm(s, dim=2, keepdim=True)
        c = s * n / (1 + n * n)
        if i < R - 1:
            L = L + torch.einsum("bnc,bnsc->bns", c, u)
    return c


def attention(x, part, W1, W2, pos):
    mids = torch.tanh(torch.einsum("bse,ec->bsc", x + pos, W1))
    score = torch.einsum("bsc,nc->bns", mids, W2)
    score = torch.softmax(torch.where(part[:, None, :], score, torch.full_like(score, FMIN)), dim=-1)
    return torch.einsum("bsc,bns->bnc", mids, score)


def select(x, m):
    chosen = torch.einsum("bkd,bsd->bsk", m, x).argmax(-1)
    selected = torch.gather(m, 1, chosen[:, :, None].expand(-1, -1, m.shape[2]))
    inner = (selected * x).sum(-1)
    return selected, inner, torch.logsumexp(inner, dim=1) - inner[:, 0]


def looked_up(p, ids):
    n = ids.shape[1]
    return Fn.Gather.apply(p["table"], ids.reshape(B, n * C), None, None).reshape(B, n, D)


BODIES = {
    "routing": (lambda p, d: Fn.ComiRecRouting.apply(p["table"], d["series"], p["W"], p["B0"], R, 0, True, None),
                lambda p, d: routing(looked_up(p, d["series"]), d["series"][:, :, 0] == 0, p["W"], p["B0"]), "W"),
    "self_attention": (lambda p, d: Fn.ComiRecSelfAttention.apply(p["table"], d["series"], p["W1"], p["W2"], p["pos"], 0,
                                                                  True, None),
                       lambda p, d: attention(looked_up(p, d["series"]), d["series"][:, :, 0] == 0, p["W1"], p["W2"],
                                              p["pos"]), "W1"),
    "select": (lambda p, d: Fn.ComiRecSelect.apply(p["table"], d["items"], p["m"], None)[:3],
               lambda p, d: select(looked_up(p, d["items"]), p["m"]), "m")}


def loss_of(y, d):
    if not isinstance(y, tuple):
        return (y * d["gcaps"]).sum()
    return (y[0] * d["gsel"]).sum() + (y[1] * d["ginner"]).sum() + (y[2] * d["gloss"]).sum()


def reference64(p, d, name):
    """the body in fp64, plain torch autograd -> (outputs, the gradient of BODIES[name][2])"""
    q = {k: v.detach().double() for k, v in p.items()}
    w = q[BODIES[name][2]].requires_grad_()
    part = d["series"][:, :, 0] == 0
    if name == "routing":
        y = routing(q["table"][d["series"]].reshape(B, T, D), part, q["W"], q["B0"])
    elif name == "self_attention":
        y = attention(q["table"][d["series"]].reshape(B, T, D), part, q["W1"], q["W2"], q["pos"])
    else:
        y = select(q["table"][d["items"]].reshape(B, NS, D), q["m"])
    loss_of(y, {k: v.double() if v.is_floating_point() else v for k, v in d.items()}).backward()
    return [t.detach() for t in (y if isinstance(y, tuple) else (y,))], w.grad


def measure(body, p, d, grad_of):
    def step():
        for t in p.values():
            t.grad = None
        y = body(p, d)
        loss_of(y, d).backward()
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
    y = [t.detach().clone() for t in (y if isinstance(y, tuple) else (y,))]
    return y, p[grad_of].grad.clone(), {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
                                        "max_us": round(max(times), 1), "kernels": kernels}


def main():
    p, d = make()
    res = {"shape": {"B": B, "T": T, "C": C, "E": E, "K": K, "R": R, "Ns": NS, "V": V}}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for name, (fused, composed, grad_of) in BODIES.items():
        y64, g64 = reference64(p, d, name)
        dist = lambda y, g: {"out": max(float((a - b).abs().max()) for a, b in zip(y, y64)), "d%s_rel" % grad_of: rel(g, g64)}
        yf, gf, rf = measure(fused, p, d, grad_of)
        yc, gc, rc = measure(composed, p, d, grad_of)
        res[name] = {"fused": rf, "composed": rc, "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                     "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}
        del y64, g64, yf, gf, yc, gc
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
