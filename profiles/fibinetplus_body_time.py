"""Forward + backward of the default FiBiNet++ input stage + body (no head) at B = 8192, F = 13 (10 categorical + 3 key
fields), E = 16, 'interaction' bilinear weights, 2 groups, V = 160000, two ways: (1) the fused entry points of
csrc/fibinetplus.hip (functional.EmbNormLookup / FiBiNetPlusBlock); (2) composed from the entry points that existed
before them -- rec_emb_gather_f32, rec_batchnorm_*, rec_layernorm_*, rec_gemm_f32 with its epilogues, rec_feat_act_*, the
dedup + segment sum, and torch for the elementwise products, the grouping, the slices and the stacks.  Each path is
captured in one hipGraph (so the figure is device time, not Python) and replayed; the median and the min-max spread of
REPS timed groups of INNER replays are printed with the kernel count of one iteration, as one JSON line.  The line also
gives each path's distance from the same mathematics in fp64 (plain torch on the device, not timed): max |difference| of
out, and of three gradients relative to their largest entry.
Usage: python profiles/fibinetplus_body_time.py > profiles/fibinetplus_body_time.json"""
import itertools
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import functional as Fn, ops          # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, Fc, Fk, E, G, RATIO, O, V = 8192, 10, 3, 16, 2, 3, 16, 160000
F, D = Fc + Fk, (Fc + Fk) * E
PAIRS = list(itertools.combinations(range(F), 2))
P, MID = len(PAIRS), max(1, 2 * G * F // RATIO)
REPS, INNER = 15, 20
NAMES = ["table", "g_bn", "b_bn", "g_ln", "b_ln", "W", "Wr", "br", "gq", "bq", "S0", "b0", "g0", "be0", "S1", "b1", "g1",
         "be1"]


def make():
    g = torch.Generator().manual_seed(0)
    n = lambda *s, std=1.0, mean=0.0: (torch.randn(*s, generator=g) * std + mean).cuda().requires_grad_()
    u = lambda a, b: (((torch.rand(a, b, generator=g) * 2 - 1) * (6.0 / (a + b)) ** 0.5).cuda().requires_grad_())
    p = {"table": n(V, E, std=0.5), "g_bn": n(E, std=0.1, mean=1.0), "b_bn": n(E, std=0.1),
         "g_ln": n(Fk, E, std=0.1, mean=1.0), "b_ln": n(Fk, E, std=0.1), "W": n(P, E, E, std=(1.0 / E) ** 0.5),
         "Wr": u(P, O), "br": n(O, std=0.1), "gq": n(O, std=0.1, mean=1.0), "bq": n(O, std=0.1),
         "S0": u(2 * G * F, MID), "b0": n(MID, std=0.1), "g0": n(MID, std=0.1, mean=1.0), "be0": n(MID, std=0.1),
         "S1": u(MID, D), "b1": n(D, std=0.1), "g1": n(D, std=0.1, mean=1.0), "be1": n(D, std=0.1)}
    X = torch.randint(0, V, (B, F), generator=g).cuda()
    values = torch.randn(B, Fk, generator=g).cuda()
    dout = (torch.rand(B, O + D, generator=g) * 2 - 1).cuda()
    return p, X, values, dout


def fused(p, X, values, mm, mv):
    x = Fn.EmbNormLookup.apply(p["table"], X, values, p["g_bn"], p["b_bn"], p["g_ln"], p["b_ln"], mm, mv, True, None)
    return Fn.FiBiNetPlusBlock.apply(x, p["Wr"], p["br"], p["gq"], p["bq"], p["S0"], p["b0"], p["g0"], p["be0"], p["S1"],
                                     p["b1"], p["g1"], p["be1"], G, 2, lambda ws: torch.stack(ws), *p["W"].unbind(0))


def composed(p, X, values, mm, mv):
    relu = lambda t: Fn.FeatAct.apply(t, ops.DACT_RELU, None, None, None)
    rows = Fn.Gather.apply(p["table"], X, None, None).reshape(B, F, E)
    cat = Fn.BatchNorm.apply(rows[:, :Fc].reshape(B * Fc, E), p["g_bn"], p["b_bn"], mm, mv, True, 1e-3, 0.99)
    keys = [Fn.LayerNorm.apply((rows[:, Fc + j] * values[:, j:j + 1]).contiguous(), p["g_ln"][j], p["b_ln"][j])
            for j in range(Fk)]
    x = torch.cat([cat.reshape(B, Fc, E), torch.stack(keys, dim=1)], dim=1)
    ps = [(Fn.LinearAct.apply(x[:, i].contiguous(), p["W"][t], None, ops.ACT_NONE) * x[:, j]).sum(dim=1)
          for t, (i, j) in enumerate(PAIRS)]
    q = Fn.LayerNorm.apply(Fn.LinearAct.apply(torch.stack(ps, dim=1).contiguous(), p["Wr"], p["br"], ops.ACT_NONE),
                           p["gq"], p["bq"])
    xg = x.reshape(B, F, G, E // G)
    s = torch.cat([xg.mean(dim=-1), xg.max(dim=-1).values], dim=-1).reshape(B, 2 * G * F).contiguous()
    h = relu(Fn.LayerNorm.apply(Fn.LinearAct.apply(s, p["S0"], p["b0"], ops.ACT_NONE), p["g0"], p["be0"]))
    A = relu(Fn.LayerNorm.apply(Fn.LinearAct.apply(h, p["S1"], p["b1"], ops.ACT_NONE), p["g1"], p["be1"]))
    return torch.cat([q, x.reshape(B, D) * A], dim=1)


def reference64(p, X, values, dout):
    """the same mathematics in fp64, plain torch autograd -> out, dW, dS1 and the dense dtable"""
    d = {k: t.detach().double().requires_grad_() for k, t in p.items()}
    ln = lambda z, g, b: (z - z.mean(-1, keepdim=True)) / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + 1e-3) * g + b
    rows = d["table"][X]
    cat = rows[:, :Fc]
    mean, var = cat.mean(dim=(0, 1)), cat.var(dim=(0, 1), unbiased=False)
    x = torch.cat([(cat - mean) / torch.sqrt(var + 1e-3) * d["g_bn"] + d["b_bn"],
                   ln(rows[:, Fc:] * values.double().unsqueeze(-1), d["g_ln"], d["b_ln"])], dim=1)
    ii, jj = [i for i, _ in PAIRS], [j for _, j in PAIRS]
    pp = torch.einsum("bpe,pek,bpk->bp", x[:, ii], d["W"], x[:, jj])
    q = ln(pp @ d["Wr"] + d["br"], d["gq"], d["bq"])
    xg = x.reshape(B, F, G, E // G)
    s = torch.cat([xg.mean(dim=-1), xg.max(dim=-1).values], dim=-1).reshape(B, 2 * G * F)
    h = torch.relu(ln(s @ d["S0"] + d["b0"], d["g0"], d["be0"]))
    A = torch.relu(ln(h @ d["S1"] + d["b1"], d["g1"], d["be1"]))
    out = torch.cat([q, x.reshape(B, D) * A], dim=1)
    out.backward(dout.double())
    return out.detach(), d["W"].grad, d["S1"].grad, d["table"].grad


def measure(body, p, X, values, dout):
    mm, mv = torch.zeros(E, device="cuda"), torch.ones(E, device="cuda")
    leaves = [p[k] for k in NAMES]

    def step():
        for t in leaves:
            t.grad = None
        y = body(p, X, values, mm, mv)
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
    grads = [p["W"].grad.detach().clone(), p["S1"].grad.detach().clone(), p["table"].grad.to_dense().clone()]
    return y.detach().clone(), grads, {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
                                       "max_us": round(max(times), 1), "kernels": kernels}


def main():
    p, X, values, dout = make()
    yf, gf, rf = measure(fused, p, X, values, dout)
    yc, gc, rc = measure(composed, p, X, values, dout)
    y64, *g64 = reference64(p, X, values, dout)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    keys = ("dW_rel", "dS1_rel", "dtable_rel")
    dist = lambda y, g: dict({"out": float((y - y64).abs().max())}, **{k: rel(a, b) for k, a, b in zip(keys, g, g64)})
    agree = dict({"out": float((yf - yc).abs().max())}, **{k: rel(a, b) for k, a, b in zip(keys, gf, gc)})
    print(json.dumps({"shape": {"B": B, "F": F, "Fk": Fk, "E": E, "G": G, "ratio": RATIO, "O": O, "V": V,
                                "type": "interaction"}, "fused": rf, "composed": rc, "fused_vs_composed": agree,
                      "fused_vs_fp64": dist(yf, gf), "composed_vs_fp64": dist(yc, gc)}))


if __name__ == "__main__":
    main()
