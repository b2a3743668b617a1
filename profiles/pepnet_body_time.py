"""Forward + backward of layers.PEPNetLayer two ways, with the same parameters, at the reference's default shape (9 main and
2 personalisation fields, E = 8, gate hidden 16, 3 tasks of [64, 16, 1]) and B = 8192, V = 160000: the fused path
(functional.EmbEPNetLookup over csrc/epnet.hip + functional.PosoMLP over csrc/poso.hip) and the same computation
COMPOSED from what the project had before them -- two functional.Gather lookups, functional.LinearAct per gate layer and
per dense layer, torch elementwise products, sigmoid / relu through functional.LinearAct's epilogue or torch, stack /
flatten / cat / detach.  Both for chain_layers=False (the reference as written: the composed path, like the fused one,
computes only the layer that reaches the output) and chain_layers=True.  Each path is captured in one hipGraph (so the
figure is device time, not Python) and replayed; the two graphs are timed in alternation, REPS groups of INNER replays
each, and the median and min-max of the groups are printed with the kernel count of one iteration, as one JSON line.
The line also gives the two paths' distance from each other and the compiler's resource report of every kernel of the
two files (registers, scratch bytes per lane, occupancy), from a device-only compile for gfx950.
Usage: python profiles/pepnet_body_time.py > profiles/pepnet_body_time.json"""
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from explicit_tf2_recommendation_amd import functional as Fn              # noqa: E402
from explicit_tf2_recommendation_amd import layers, ops                    # noqa: E402
from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE            # noqa: E402

B, V = 8192, 160000
REPS, INNER = 15, 20
WATCH = ("embedding_layer.embeddings", "poso_gate_for_embedding.0.gate.layers.0.kernel",
         "poso_mlp_layers.0.gates.2.gate.layers.0.kernel", "poso_mlp_layers.2.dense_layers.2.kernel",
         "poso_mlp_layers.1.C_list.2")


def compiler_report():
    csrc = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")
    out = {}
    for src in ("epnet.hip", "poso.hip"):
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
               "-Wno-unused-result", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(csrc, src), "-o", os.devnull]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        name = None
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", m.group(1))
                name = re.sub(r"(kernel)(ILb(\d)E)?.*", lambda k: k.group(1) + ("<%s>" % k.group(3) if k.group(3) else ""),
                              name)
                out[name] = {}
            for key, label in (("vgprs", "VGPRs"), ("agprs", "AGPRs"), ("scratch_bytes_per_lane", "ScratchSize [bytes/lane]"),
                               ("occupancy_waves_per_simd", "Occupancy [waves/SIMD]")):
                m = re.search(re.escape(label) + r": (\d+)", line)
                if m and name:
                    out[name][key] = int(m.group(1))
    return out


def composed_forward(lay, inputs):
    """PEPNetLayer.call out of the kernels that existed before csrc/epnet.hip and csrc/poso.hip"""
    F, E = len(lay.categorical_features), lay.embedding_dims
    Xc = layers.assemble_index(inputs, lay.categorical_features)
    Xp = layers.assemble_index(inputs, lay.ppnet_input_features)
    main = lay.embedding_layer(Xc)
    pp = lay.embedding_layer(Xp).reshape(Xp.shape[0], -1)

    def gatenu(gate, v):
        l0, l1 = gate.gate.layers
        h = Fn.LinearAct.apply(v, l0.kernel, l0.bias, ops.ACT_RELU)
        return 2.0 * Fn.LinearAct.apply(h, l1.kernel, l1.bias, ops.ACT_SIGMOID)

    gates = torch.stack([gatenu(gt, pp) for gt in lay.poso_gate_for_embedding], dim=1)
    c = (gates * main).reshape(main.shape[0], F * E)
    g = torch.cat([c.detach(), pp], dim=1)
    outs = []
    for tw in lay.poso_mlp_layers:
        x = c
        for i in tw.live_layers():
            d = Fn.LinearAct.apply(x, tw.dense_layers[i].kernel, tw.dense_layers[i].bias, ops.ACT_NONE)
            z = tw.C_list[i] * (d * gatenu(tw.gates[i], g))
            x = torch.relu(z) if tw.activations[i] == "relu" else torch.sigmoid(z)
        outs.append(x)
    return torch.stack(outs, dim=1)


def make(chain, state=None):
    lay = layers.PEPNetLayer(feature_dims=V, chain_layers=chain).cuda().train()
    for m in lay.modules():
        m.check_ids = False                                  # a host read of the bounds flag cannot be captured
    if state is not None:
        lay.load_state_dict(state)
    return lay


def capture(lay, forward, inputs, dout):
    def step():
        for p in lay.parameters():
            p.grad = None
        out = forward(lay, inputs)
        (out * dout).sum().backward()
        return out

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
        out = step()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    return graph, out, {"kernels": len(events), "largest_kernels_us": dict(sorted(top.items(), key=lambda kv: -kv[1])[:8])}


def timed(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(INNER):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER * 1000.0


def mode_result(chain):
    g = torch.Generator().manual_seed(0)
    layers.set_init_seed(0)
    fused = make(chain)
    composed = make(chain, fused.state_dict())
    names = fused.categorical_features + fused.ppnet_input_features
    inputs = {k: torch.randint(0, V, (B, 1), generator=g).cuda() for k in names}
    dout = (torch.rand(B, 3, 1, generator=g) * 2 - 1).cuda()
    gf, of, info_f = capture(fused, lambda lay, ins: lay(ins), inputs, dout)
    gc, oc, info_c = capture(composed, composed_forward, inputs, dout)
    tf, tc = [], []
    for _ in range(REPS):                                    # in alternation: a drift of the machine hits both alike
        tf.append(timed(gf))
        tc.append(timed(gc))
    summary = lambda t: {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
    dense = lambda t: t.to_dense() if t.is_sparse else t
    rel = lambda a, b: float((dense(a) - dense(b)).abs().max() / dense(b).abs().max())
    pf, pc = dict(fused.named_parameters()), dict(composed.named_parameters())
    return {"shape": {"B": B, "V": V, "F": 9, "P": 2, "E": 8, "Hg": 16, "T": 3, "units": [64, 16, 1],
                      "chain_layers": chain},
            "fused": dict(summary(tf), **info_f), "composed": dict(summary(tc), **info_c),
            "fused_slowest_below_composed_fastest": max(tf) < min(tc),
            "fused_vs_composed": dict({"output": float((of - oc).abs().max())},
                                      **{k: rel(pf[k].grad, pc[k].grad) for k in WATCH})}


def main():
    res = {"as_written": mode_result(False), "chained": mode_result(True)}
    res["compiler"] = compiler_report()
    res["scratch_free"] = all(k["scratch_bytes_per_lane"] == 0 for k in res["compiler"].values())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
