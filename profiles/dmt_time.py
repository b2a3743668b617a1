"""Forward + backward of the DMT family two ways, with the same parameters: the path of fused=True (the self-attention as
B T one-query attentions of csrc/sim.hip over a [B T, T, D] copy of the rows, the LayerNorm and GEMM ops, one
functional.Gather in DMTLayer) and the composed path of the SAME class (fused=False: einsum attention and torch ops), at
B = 4096, T = 6 and 16 and the reference's defaults (3 layers, d_model 48, 4 heads of key_dim 48, dff 32, E = 16, 3 item
features, a 160,000-row table): dmt.Encoder alone (the encoder stack of one series), dmt.DeepInterestTransformer with
the embedded inputs given, and dmt.DMTLayer(head='linear').  A series keeps a random valid prefix of at least a third of
its steps.  Each path is captured in one hipGraph (so the figure is device time, not Python) and replayed; the graphs are
timed in alternation, REPS groups of INNER replays each, and the median and min-max of the groups are printed with the
kernel count of one iteration and its largest kernels.  The two bias networks of the layer are also timed alone, in a
graph of their own, and set as a share of the fused layer's step.  One JSON line per T.  No kernel of csrc/ belongs to
this family alone, so there is no compiler report.
Usage: python profiles/dmt_time.py > profiles/dmt_time.json"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import dmt, layers                    # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, V, E, C = 4096, 160000, 16, 3
LAYERS, D, H, DFF = 3, 48, 4, 32
REPS, INNER = 9, 5


def warm_and_capture(step):
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
        res = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    return graph, res, {"kernels": len(events), "largest_kernels_us": dict(sorted(top.items(), key=lambda kv: -kv[1])[:6])}


def timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER * 1000.0


def summary(t):
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def prepare(lay, state=None):
    lay = lay.cuda().train()
    for m in lay.modules():
        m.check_ids = False                                  # a host read of the bounds flag cannot be captured
    if state is not None:
        lay.load_state_dict(state)
    return lay


def pair(make, run, leaves=()):
    """make(fused) -> module, run(module) -> output tensor, leaves: input tensors that take a gradient; -> the two graphs,
    their outputs and kernel counts"""
    layers.set_init_seed(0)
    fused = prepare(make(True))
    composed = prepare(make(False), fused.state_dict())
    out = []
    for lay in (fused, composed):
        def step(lay=lay):
            for p in list(lay.parameters()) + list(leaves):
                p.grad = None
            res = run(lay)
            res.sum().backward()
            return res
        out.append(warm_and_capture(step))
    return out, fused


def compare(graphs):
    (gf, rf, info_f), (gc, rc, info_c) = graphs
    tf, tc = [], []
    for _ in range(REPS):                                    # in alternation: a drift of the machine hits both alike
        tf.append(timed(gf))
        tc.append(timed(gc))
    return {"fused": dict(summary(tf), **info_f), "composed": dict(summary(tc), **info_c),
            "fused_slowest_below_composed_fastest": max(tf) < min(tc),
            "composed_over_fused": round(statistics.median(tc) / statistics.median(tf), 2),
            "output_distance": float((rf - rc).detach().abs().max())}, statistics.median(tf)


def shape_result(T):
    g = torch.Generator().manual_seed(0)
    keep = torch.arange(T)[None, :] < torch.randint(0, T + 1, (B, 1), generator=g).clamp(min=max(1, T // 3))
    enc_ids = (torch.randint(1, V, (B, T), generator=g) * keep).cuda()
    dec_ids = torch.randint(1, V, (B, 1), generator=g).cuda()
    x_enc = (torch.randn(B, T, D, generator=g) * 0.3).cuda().requires_grad_()
    x_dec = (torch.randn(B, 1, D, generator=g) * 0.3).cuda().requires_grad_()
    result = {"shape": {"B": B, "V": V, "T": T, "layers": LAYERS, "d_model": D, "heads": H, "key_dim": D, "dff": DFF,
                        "valid_positions": float(keep.float().mean())}}
    graphs, _ = pair(lambda f: dmt.Encoder(LAYERS, D, H, DFF, fused=f), lambda l: l(x_enc, True, enc_ids != 0), (x_enc,))
    result["encoder_stack"], _ = compare(graphs)
    graphs, _ = pair(lambda f: dmt.DeepInterestTransformer(LAYERS, D, H, DFF, input_vocab_size=8, fused=f),
                     lambda l: l(enc_ids, dec_ids, True, x_enc, x_dec), (x_enc, x_dec))
    result["deep_interest_transformer"], _ = compare(graphs)
    del graphs
    probe = dmt.DMTLayer(feature_dims=V, head="linear", fused=False)
    inputs = {k: torch.randint(1, V, (B,), generator=g).cuda()
              for k in probe.user_and_context_categorical_features + probe.item_categorical_features}
    for k in probe.continuous_features:
        inputs[k] = torch.rand(B, generator=g).cuda()
    for names in (probe.click_series_features, probe.cart_series_features, probe.order_series_features):
        keep = torch.arange(T)[None, :] < torch.randint(0, T + 1, (B, 1), generator=g).clamp(min=max(1, T // 3))
        for k in names:
            inputs[k] = (torch.randint(1, V, (B, T), generator=g) * keep).cuda()
    inputs["position"] = torch.randint(0, 400, (B,), generator=g).cuda()
    inputs["page"] = torch.randint(0, 100, (B,), generator=g).cuda()
    for k in probe.position_bias_features["neighbourhood_features"]:
        inputs[k] = torch.randint(0, V, (B, 7), generator=g).cuda()
    graphs, fused = pair(lambda f: dmt.DMTLayer(feature_dims=V, head="linear", fused=f),
                         lambda l: torch.cat(list(l(inputs).values()), 1))
    result["dmt_layer_linear_head"], layer_us = compare(graphs)

    def bias_step():
        for net in (fused.bias_network_ctr, fused.bias_network_cvr):
            for p in net.parameters():
                p.grad = None
        res = fused.bias_network_ctr(inputs) + fused.bias_network_cvr(inputs)
        res.sum().backward()
        return res
    gb, _, info_b = warm_and_capture(bias_step)
    tb = [timed(gb) for _ in range(REPS)]
    result["bias_networks_alone"] = dict(summary(tb), **info_b,
                                         share_of_the_fused_layer=round(statistics.median(tb) / layer_us, 3))
    return result


def main():
    for T in (6, 16):
        print(json.dumps(shape_result(T)), flush=True)


if __name__ == "__main__":
    main()
