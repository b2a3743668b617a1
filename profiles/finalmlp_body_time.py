"""Forward + backward of the three lookups and the FinalMLP body at the default model (Fu = Fi = 5, E = 16, gates [64],
streams [64, 64, 64] with BatchNorm, 8 heads), B = 8192, V = 160000, training mode, two ways: the fused path of
layers.FinalMLPLayer (functional.Gather + functional.FinalMLPBody over csrc/finalmlp.hip) and the composed path of the
SAME layer class (fused=False: Gather, Dense, BatchNormalization, Activation, torch for the gating and the head's
einsum), with the same parameters.  Each path is captured in one hipGraph (so the figure is device time, not Python) and
replayed; the median and the min-max spread of REPS timed groups of INNER replays are printed with the kernel count of
one iteration, as one JSON line.  The line also gives the two paths' distance from each other: max |difference| of the
output, and of three gradients relative to their largest entry.
Usage: python profiles/finalmlp_body_time.py > profiles/finalmlp_body_time.json"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explicit_tf2_recommendation_amd import layers                         # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, V = 8192, 160000
REPS, INNER = 15, 20
WATCH = ("fs_layer.mlp_gate1_hidden.layers.0.kernel", "mlp1.layers.0.kernel", "mlp2.layers.7.gamma", "interaction_layer.W_12")


def make(fused, state=None):
    lay = layers.FinalMLPLayer(fused=fused).cuda().train()
    lay.check_ids = False                                    # a host read of the bounds flag cannot be captured
    for m in lay.modules():
        m.check_ids = False
    if state is not None:
        lay.load_state_dict(state)
    return lay


def measure(lay, inputs, dout):
    start = {k: v.clone() for k, v in lay.state_dict().items() if "moving" in k}

    def step():
        for p in lay.parameters():
            p.grad = None
        y = lay(inputs)["output"]
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
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    top = {}
    for e in events:
        name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][-48:]
        top[name] = round(top.get(name, 0.0) + e.device_time, 1)
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
    lay.load_state_dict(start, strict=False)                 # one replay from the common statistics: comparable results
    graph.replay()
    torch.cuda.synchronize()
    grads = {k: dict(lay.named_parameters())[k].grad.clone() for k in WATCH}
    return y.detach().clone(), grads, {
        "median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1), "max_us": round(max(times), 1),
        "kernels": len(events),
        "largest_kernels_us": dict(sorted(top.items(), key=lambda kv: -kv[1])[:8])}


def main():
    g = torch.Generator().manual_seed(0)
    layers.set_init_seed(0)
    fused = make(True)
    composed = make(False, fused.state_dict())
    names = fused.user_features + fused.item_features
    inputs = {k: torch.randint(0, V, (B,), generator=g).cuda() for k in names}
    dout = (torch.rand(B, 1, generator=g) * 2 - 1).cuda()
    yf, gf, rf = measure(fused, inputs, dout)
    yc, gc, rc = measure(composed, inputs, dout)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    res = {"shape": {"B": B, "V": V, "user_fields": 5, "item_fields": 5, "E": 16, "gates": [64], "streams": [64, 64, 64],
                     "heads": 8, "training": True},
           "fused": rf, "composed": rc, "fused_slowest_below_composed_fastest": rf["max_us"] < rc["min_us"],
           "fused_vs_composed": dict({"out": float((yf - yc).abs().max())}, **{k: rel(gf[k], gc[k]) for k in WATCH})}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
