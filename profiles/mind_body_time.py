"""Forward + backward of the two MIND bodies with their lookups at B = 8192, T = 50, C = 3, E = 16, K = 4, R = 3,
Ns = 11, each two ways: (1) the fused entry points of csrc/mind.hip (functional.CapsuleRouting, functional.
LabelAwareAttention: the lookup is part of the kernel); (2) the same arithmetic composed from the entry points that
existed before them -- the gather, rec_gemm_f32 through functional.LinearAct for x S, the dedup + segment sum -- and
torch for the masked softmax, the batched products of the rounds, the squash and the log-sum-exp.  Each path is captured
in one hipGraph (so the figure is device time, not Python) and replayed; the median and the min-max spread of REPS timed
groups of INNER replays are printed with the kernel count of one iteration, as one JSON line.  The line also gives the two
paths' distance from each other and from the same body in fp64 (plain torch on the device, not timed): max |difference|
of the output and of one gradient relative to their largest entry.
Usage: python profiles/mind_body_time.py > profiles/mind_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, T, C, E, K, R, NS, V = 8192, 50, 3, 16, 4, 3, 11, 160000
D = DC = C * E
FMIN = torch.finfo(torch.float32).min
REPS, INNER = 15, 20


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).cuda()
    p = {"table": n(V, E, std=0.5).requires_grad_(), "S": n(D, DC, std=D ** -0.5).requires_grad_(),
         "B0": n(K, T, std=0.05), "m": n(B, K, DC, std=0.5).requires_grad_(), "zero": torch.zeros(DC).cuda()}
    series = torch.randint(1, V, (B, T, C), generator=g)
    n_valid = torch.randint(0, T + 1, (B,), generator=g)
    series[:, :, 0] *= (torch.rand(B, T, generator=g).argsort(1) < n_valid[:, None])     # padding anywhere in the row
    d = {"series": series.cuda(), "items": torch.randint(0, V, (B, NS, C), generator=g).cuda(),
         "kv": (torch.arange(B) % (K + 1)).int().cuda(), "gcaps": (torch.rand(B, K, DC, generator=g) * 2 - 1).cuda(),
         "gout": (torch.rand(B, NS, generator=g) * 2 - 1).cuda(), "gloss": (torch.rand(B, generator=g) * 2 - 1).cuda()}
    return p, d


def rounds(u, valid, B0):
    L = B0[None].expand(u.shape[0], -1, -1)
    drop = torch.full_like(L, FMIN)
    for i in range(R):
        W = torch.softmax(torch.where(valid[:, None, :], L, drop), dim=2)
        s = W @ u
        n = torch.linalg.vector_norm(s, dim=2, keepdim=True)
        c = s * n / (1 + n * n)
        if i < R - 1:
            L = L + c @ u.transpose(1, 2)
    return c


def attention(x, m, kv):
    sc = torch.einsum("bck,bsk->bcs", m, x)
    mask = torch.arange(m.shape[1], device=m.device)[None, :, None] < kv[:, None, None]
    w = torch.softmax(torch.where(mask, sc, torch.full_like(sc, FMIN)), dim=1)
    out = (w * sc).sum(1)
    return out, torch.logsumexp(out, dim=1) - out[:, 0]


def routing_fused(p, d):
    return Fn.CapsuleRouting.apply(p["table"], d["series"], p["S"], p["B0"], R, 0, None)


def routing_composed(p, d):
    x = Fn.Gather.apply(p["table"], d["series"].reshape(B, T * C), None, None).reshape(B * T, D)
    u = Fn.LinearAct.apply(x, p["S"], p["zero"], ops.ACT_NONE).reshape(B, T, DC)
    return rounds(u, d["series"][:, :, 0] != 0, p["B0"])


def routing_loss(y, d):
    return (y * d["gcaps"]).sum()


def laa_fused(p, d):
    return Fn.LabelAwareAttention.apply(p["table"], d["items"], p["m"], d["kv"], None)


def laa_composed(p, d):
    x = Fn.Gather.apply(p["table"], d["items"].reshape(B, NS * C), None, None).reshape(B, NS, DC)
    return attention(x, p["m"], d["kv"])


def laa_loss(y, d):
    return (y[0] * d["gout"]).sum() + (y[1] * d["gloss"]).sum()


def reference64(p, d):
    """both bodies in fp64, plain torch autograd -> (capsules, dS), (out, loss, gm)"""
    tab, S, m = p["table"].detach().double(), p["S"].detach().double().requires_grad_(), \
        p["m"].detach().double().requires_grad_()
    caps = rounds(tab[d["series"]].reshape(B, T, D) @ S, d["series"][:, :, 0] != 0, p["B0"].double())
    (caps * d["gcaps"].double()).sum().backward()
    out, loss = attention(tab[d["items"]].reshape(B, NS, DC), m, d["kv"])
    ((out * d["gout"].double()).sum() + (loss * d["gloss"].double()).sum()).backward()
    return (caps.detach(), S.grad), (out.detach(), loss.detach(), m.grad)


def measure(body, loss_of, p, d, grad_of):
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
    (caps64, dS64), (out64, loss64, gm64) = reference64(p, d)
    yf, gf, rf = measure(routing_fused, routing_loss, p, d, "S")
    yc, gc, rc = measure(routing_composed, routing_loss, p, d, "S")
    dist = lambda y, g: {"out": float((y[0] - caps64).abs().max()), "dS_rel": rel(g, dS64)}
    res["routing"] = {"fused": rf, "composed": rc, "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                      "fused_vs_composed": {"out": float((yf[0] - yc[0]).abs().max()), "dS_rel": rel(gf, gc)},
                      "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}
    yf, gf, rf = measure(laa_fused, laa_loss, p, d, "m")
    yc, gc, rc = measure(laa_composed, laa_loss, p, d, "m")
    dist = lambda y, g: {"out": float((y[0] - out64).abs().max()), "loss": float((y[1] - loss64).abs().max()),
                         "gm_rel": rel(g, gm64)}
    res["attention"] = {"fused": rf, "composed": rc, "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
                        "fused_vs_composed": {"out": float((yf[0] - yc[0]).abs().max()), "gm_rel": rel(gf, gc)},
                        "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
