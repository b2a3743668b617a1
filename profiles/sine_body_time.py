"""The SINE body at B = 4096, T = 50, C = 3, E = 16, L = 100, K = 5, Ns = 11: the forward launch, the backward kernel by
kernel, and the layer's forward + backward (main_loss.sum() + aux_loss), next to the torch-ROCm eager run of the
tests/sine_ref.py transcription on the same GPU (the reference itself is TF and cannot run here: that is the only
baseline there is).  Everything is timed twice: on a UNIFORM batch, whose examples spread over the concepts, and on a
SKEWED one, where every example holds the same series row and so picks the same K concepts -- the case in which the
concept-major pass of the backward serialises.

The launches are timed with events around INNER calls (median and min-max of REPS groups); the layer and the eager
transcription are each captured in one hipGraph and replayed, so the figure is device time, not Python.  The backward's
kernels come from one profiled call.  One JSON line.
Usage: python profiles/sine_body_time.py > profiles/sine_body_time.json"""
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import layers, ops                   # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402
from tests import sine_ref as SR                                          # noqa: E402

B, T, C, E, L, K, NS, V = 4096, 50, 3, 16, 100, 5, 11, 160000
D = C * E
REPS, INNER = 11, 10


def make(skewed):
    g = torch.Generator().manual_seed(0)
    lay = layers.SINELayer(feature_dims=V, embedding_dims=E, L=L, K=K).cuda()
    lay.check_ids = False
    with torch.no_grad():                                       # the spread of the test generators, not of a fresh layer
        lay.embed.embeddings.copy_(torch.randn(V, E, generator=g) * 0.5)
        lay.interest_pool.copy_(torch.randn(L, D, generator=g) * 0.5)
        for name in ("W1", "W2", "Wk1", "Wk2", "W3", "W4"):
            q = getattr(lay, name)
            q.copy_(torch.randn(q.shape, generator=g) * D ** -0.5)
    series = torch.randint(1, V, (B, T, C), generator=g)
    n_valid = torch.randint(1, T + 1, (B,), generator=g)
    series[:, :, 0] *= (torch.rand(B, T, generator=g).argsort(1) < n_valid[:, None])
    if skewed:
        series[:] = series[0].clone()
    items = torch.randint(0, V, (B, NS, C), generator=g)
    batch = {n: series[:, :, i].contiguous().cuda() for i, n in enumerate(lay.behavior_series_features)}
    batch.update({n: items[:, :, i].contiguous().cuda() for i, n in enumerate(lay.item_categorical_features)})
    return lay, batch, series.cuda(), items.cuda()


def spread(times):
    return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1), "max_us": round(max(times), 1)}


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / INNER * 1000.0)
    return spread(times)


def graphed(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        step()
    return timed(graph.replay)


def kernels_of(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = collections.OrderedDict()
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            name = e.name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1]
            n, us = out.get(name, (0, 0.0))
            out[name] = (n + 1, us + (getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)))
    return {k: {"launches": n, "us": round(us, 1)} for k, (n, us) in out.items()}


def measure(skewed):
    lay, batch, series, items = make(skewed)
    tab = lay.embed.embeddings.detach()
    w = [q.detach() for q in (lay.interest_pool, lay.W1, lay.W2, lay.Wk1, lay.Wk2, lay.W3, lay.W4)]
    gout = (torch.rand(B, D, device="cuda") * 2 - 1)
    out, chosen = ops.sine_interest_fwd(tab, series, *w, K)
    res = {"concepts_chosen_by_anyone": int(chosen.unique().numel()),
           "most_examples_on_one_concept": int(torch.bincount(chosen.reshape(-1).long(), minlength=L).max())}
    res["forward_launch"] = timed(lambda: ops.sine_interest_fwd(tab, series, *w, K))
    bwd = lambda: ops.sine_interest_bwd(tab, series, *w, chosen, gout)
    res["backward_call"] = timed(bwd)
    res["backward_kernels"] = kernels_of(bwd)

    def layer_step():
        for q in lay.parameters():
            q.grad = None
        r = lay(batch)
        (r["main_loss"].sum() + r["aux_loss"]).backward()

    res["layer_fwd_bwd"] = graphed(layer_step)

    P = {k: q.detach().clone().requires_grad_() for k, q in lay.named_parameters()}
    wt = dict(P, pool=P["interest_pool"])
    padm = series[:, :, 0] == 0

    def eager_step():
        for q in P.values():
            q.grad = None
        t = P["embed.embeddings"]
        ui, _ = SR.sine_torch(t[series].reshape(B, T, D), padm, wt, K)
        inner = torch.einsum("bne,be->bn", t[items].reshape(B, NS, D), ui)
        ((torch.logsumexp(inner, dim=1) - inner[:, 0]).sum() + SR.aux_torch(P["interest_pool"])).backward()

    res["torch_eager_fwd_bwd"] = graphed(eager_step)
    res["torch_eager_fwd_bwd_kernels"] = sum(v["launches"] for v in kernels_of(eager_step).values())
    return res


def main():
    res = {"shape": {"B": B, "T": T, "C": C, "E": E, "L": L, "K": K, "Ns": NS, "V": V},
           "slab_examples": SR.slab_examples(B, D, K), "scratch_bytes": SR.scratch_bytes(B, D, K)}
    res["uniform"] = measure(False)
    torch.cuda.empty_cache()
    res["skewed"] = measure(True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
